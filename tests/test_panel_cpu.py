"""CPU tests of the panel entry points (qrk_bd_factorize_apply_qt / qrk_bd_panel_kernel_name): declared, exported, bound, the
argument checks that need no device, and the methods of the two mirrors."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qrk_bd_factorize_apply_qt", "qrk_bd_panel_kernel_name")


def test_symbols_are_declared_exported_and_bound():
    from qrkit_amd import _capi
    txt = open(os.path.join(ROOT, "include", "qrkit_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _capi.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/qrkit_amd.h"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        assert n in _capi.EXPORTS
    decl = re.search(r"qrk_status\s+qrk_bd_factorize_apply_qt\s*\(([^)]*)\)", txt).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["plan", "tiles", "c", "ldc", "ncols", "r_vals", "perm", "hcoeffs", "qtc", "ldq",
                                                                   "space"]
    f = lib.qrk_bd_factorize_apply_qt
    assert f.restype is C.c_int and len(f.argtypes) == 11
    assert [f.argtypes[i] for i in (3, 4, 9)] == [C.c_int64] * 3 and f.argtypes[10] is C.c_int
    decl = re.search(r"const\s+char\s*\*\s*qrk_bd_panel_kernel_name\s*\(([^)]*)\)", txt).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["plan", "ncols"]
    assert lib.qrk_bd_panel_kernel_name.restype is C.c_char_p and lib.qrk_bd_panel_kernel_name.argtypes[1] is C.c_int64


def test_null_plan_is_an_invalid_argument_without_a_device():
    from qrkit_amd import _capi
    lib = _capi.lib()
    for space in (_capi.MEM_DEVICE, _capi.MEM_HOST):
        assert lib.qrk_bd_factorize_apply_qt(None, None, None, 1, 1, None, None, None, None, 1, space) == _capi.STATUS_INVALID_ARGUMENT
        assert b"NULL plan" in lib.qrk_last_error(None)
    assert lib.qrk_bd_panel_kernel_name(None, 1) == b""


def test_python_and_cpp_mirrors_have_the_methods():
    from qrkit_amd.angular import BlockAngularSparseQR
    from qrkit_amd.solvers import BlockDiagonalSparseQR
    for m in ("factorizeApplyQtDevice", "panelKernelName"):
        assert callable(getattr(BlockDiagonalSparseQR, m))
    for m in ("factorizeAndSolve", "computeAndSolve"):
        assert callable(getattr(BlockAngularSparseQR, m))
    hpp = open(os.path.join(ROOT, "include", "qrkit", "QRKit.hpp")).read()
    assert "void factorizeApplyQtDevice(" in hpp and "panelKernelName(" in hpp and "qrk_bd_factorize_apply_qt(" in hpp
    angular = hpp[hpp.index("class BlockAngularSparseQR {"):hpp.index("class ShardedBlockAngularSparseQR")]
    assert "Vector factorizeAndSolve(" in angular and "Vector computeAndSolve(" in angular
