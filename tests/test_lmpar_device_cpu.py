"""CPU: the device-side lmpar of the C ABI (qrk_bd_lmpar_device) is declared with the argument order its callers rely on, exported,
bound, and rejects NULL arguments before it touches a device.  (Without a device there is no plan to pass: the NULL delta / par / x
cases run here next to a NULL plan, with every other argument a live address, and again on a real plan in
test_lmpar_device_gpu.py.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qrk_bd_lmpar_device"


def test_symbol_is_declared_exported_and_bound():
    from qrkit_amd import _capi
    txt = open(os.path.join(ROOT, "include", "qrkit_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _capi.lib()
    assert re.search(r"\b%s\s*\(" % NAME, txt), f"{NAME} is not declared in include/qrkit_amd.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported by the library"
    assert NAME in _capi.EXPORTS
    assert _capi.EXPORTS.index(NAME) == _capi.EXPORTS.index("qrk_bd_lmpar") + 1          # header order: next to qrk_bd_lmpar
    decl = re.search(r"qrk_status\s+%s\s*\(([^)]*)\)" % NAME, txt).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["plan", "r_vals", "perm", "y", "diag", "delta", "par", "x", "iters", "trace"]
    # delta and par are pointers (device memory), unlike qrk_bd_lmpar's double delta
    args = [a.strip() for a in decl.split(",")]
    assert args[5] == "const double* delta" and args[6] == "double* par"
    assert lib.qrk_bd_lmpar_device.restype is C.c_int and len(lib.qrk_bd_lmpar_device.argtypes) == 10


def test_null_arguments_are_rejected_without_a_gpu():
    from qrkit_amd import _capi
    lib = _capi.lib()
    I = _capi.STATUS_INVALID_ARGUMENT
    buf = (C.c_double * 40)()
    a = C.addressof(buf)
    assert lib.qrk_bd_lmpar_device(None, None, None, None, None, None, None, None, None, None) == I
    assert lib.qrk_bd_lmpar_device(None, a, a, a, a, a, a, a, a, a) == I                  # plan
    assert lib.qrk_bd_lmpar_device(None, a, a, a, a, None, a, a, a, a) == I               # delta
    assert lib.qrk_bd_lmpar_device(None, a, a, a, a, a, None, a, a, a) == I               # par
    assert lib.qrk_bd_lmpar_device(None, a, a, a, a, a, a, None, a, a) == I               # x
    assert all(v == 0.0 for v in buf)                                                     # nothing was written


def test_python_and_cpp_mirrors_have_the_method():
    from qrkit_amd.solvers import BlockDiagonalSparseQR
    assert callable(getattr(BlockDiagonalSparseQR, "lmparDevice"))
    hpp = open(os.path.join(ROOT, "include", "qrkit", "QRKit.hpp")).read()
    assert "Vector lmparDevice(" in hpp and "qrk_bd_lmpar_device(" in hpp
