"""CPU tests of the Q-less entry points (qrk_bd_factorize_rhs / qrk_bd_rhs_kernel_name): declared, exported, bound, and
argument checks that need no device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qrk_bd_factorize_rhs", "qrk_bd_rhs_kernel_name")


def test_symbols_are_declared_exported_and_bound():
    from qrkit_amd import _capi
    txt = open(os.path.join(ROOT, "include", "qrkit_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _capi.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/qrkit_amd.h"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        assert n in _capi.EXPORTS
    # the declaration the callers rely on: tiles, b, nrhs, r_vals, perm, hcoeffs, qtb, x, space
    decl = re.search(r"qrk_status\s+qrk_bd_factorize_rhs\s*\(([^)]*)\)", txt).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["plan", "tiles", "b", "nrhs", "r_vals", "perm", "hcoeffs", "qtb", "x", "space"]
    assert lib.qrk_bd_factorize_rhs.restype is C.c_int and len(lib.qrk_bd_factorize_rhs.argtypes) == 10
    assert lib.qrk_bd_rhs_kernel_name.restype is C.c_char_p


def test_null_plan_is_an_invalid_argument_without_a_device():
    from qrkit_amd import _capi
    lib = _capi.lib()
    for space in (_capi.MEM_DEVICE, _capi.MEM_HOST):
        assert lib.qrk_bd_factorize_rhs(None, None, None, 1, None, None, None, None, None, space) == _capi.STATUS_INVALID_ARGUMENT
    assert lib.qrk_bd_rhs_kernel_name(None, 1) == b""


def test_python_and_cpp_mirrors_have_the_methods():
    from qrkit_amd.solvers import BlockDiagonalSparseQR
    for m in ("factorizeAndSolve", "computeAndSolve", "rhsKernelName"):
        assert callable(getattr(BlockDiagonalSparseQR, m))
    hpp = open(os.path.join(ROOT, "include", "qrkit", "QRKit.hpp")).read()
    assert "Vector factorizeAndSolve(" in hpp and "Vector computeAndSolve(" in hpp and "qrk_bd_factorize_rhs(" in hpp
