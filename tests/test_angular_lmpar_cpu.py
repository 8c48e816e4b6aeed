"""CPU: the C ABI of the block-angular lmpar without a device -- the new symbols, their argument checks, the
workspace size, the host state machine of the scalar rule against tests/lm_reference.lmpar bit for bit -- and the numpy prototype
of the transposed chain (tests/angular_lmpar_reference.py) against the factor-free formulas."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import angular_lmpar_reference as ref
import lm_reference

NEW = ("qrk_bd_solve_rt", "qrk_bd_solve_rt_kernel_name", "qrk_dense_gemv_t_work", "qrk_dense_gemv_t", "qrk_dense_solve_rt",
       "qrk_dense_trmv_t", "qrk_lmpar_begin", "qrk_lmpar_next")


def test_new_symbols_are_declared_exported_and_bound():
    from qrkit_amd import _capi as capi
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qrkit_amd.h")).read()
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/qrkit_amd.h"
        assert name in capi.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name} has no ctypes signature"
    assert "qrk_lmpar_state" in header and C.sizeof(capi.LmparState) == 8 * 6 + 4 * 2 + 8 * 33


def test_null_and_invalid_arguments_are_rejected_without_a_gpu():
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    I = capi.STATUS_INVALID_ARGUMENT
    assert lib.qrk_bd_solve_rt(None, None, None, None, None) == I
    assert lib.qrk_bd_solve_rt(None, 8, 8, 8, None) == I
    assert lib.qrk_bd_solve_rt_kernel_name(None) == b""
    assert lib.qrk_dense_gemv_t(None, None, 0, 0, 0, None, None, 1.0, None, None, None) == I
    assert lib.qrk_dense_gemv_t(None, 8, 4, 4, 2, None, 8, 1.0, None, 8, 8) == I
    assert lib.qrk_dense_solve_rt(None, None, 0, 0, None) == I
    assert lib.qrk_dense_solve_rt(None, 8, 3, 3, 8) == I
    assert lib.qrk_dense_trmv_t(None, None, 0, 0, None, None) == I
    assert lib.qrk_dense_trmv_t(None, 8, 3, 3, 8, 8) == I
    st = capi.LmparState()
    assert lib.qrk_lmpar_begin(None, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_begin(C.byref(st), 0.0, 0.0, 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_begin(C.byref(st), -1.0, 0.0, 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_begin(C.byref(st), 1.0, -1.0, 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_begin(C.byref(st), float("nan"), 0.0, 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_begin(C.byref(st), 1.0, float("nan"), 1.0, 1.0, 0.0, 1.0) == -1
    assert lib.qrk_lmpar_next(None, 1.0, 1.0) == -1
    # a search that has stopped takes no further evaluation
    assert lib.qrk_lmpar_begin(C.byref(st), 10.0, 0.0, 1.0, 1.0, 0.0, 1.0) == 0 and st.par == 0.0 and st.iters == 0
    assert lib.qrk_lmpar_next(C.byref(st), 1.0, 1.0) == -1


def test_gemv_t_work_is_positive_and_monotone():
    from qrkit_amd import _capi as capi
    work = capi.lib().qrk_dense_gemv_t_work
    rows = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097, 10 ** 6, 10 ** 6 + 1]
    cols = [0, 1, 5, 6, 8, 9, 70, 384, 385]
    table = np.array([[work(r, c) for c in cols] for r in rows])
    assert np.all(table > 0)
    assert np.all(np.diff(table, axis=0) >= 0) and np.all(np.diff(table, axis=1) >= 0)
    assert table[-1, -1] > table[0, 0]


# ---- the host state machine against tests/lm_reference.lmpar ---------------------------------------------------------------------------

def run_state_machine(sfun, s2, gnorm2, delta, par0):
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    st = capi.LmparState()
    s0, s1 = sfun(0.0)
    rc = lib.qrk_lmpar_begin(C.byref(st), delta, par0, s0, s1, s2, gnorm2)
    evals = 1
    while rc == 1:
        assert evals <= 10
        s0, s1 = sfun(st.par)
        rc = lib.qrk_lmpar_next(C.byref(st), s0, s1)
        evals += 1
    assert rc == 0
    trace = np.array(st.trace[:]).reshape(11, 3)
    assert np.all(trace[st.iters + 1:] == 0.0)
    return st.par, st.iters, trace[:st.iters + 1]


def run_reference(monkeypatch, sfun, s2, gnorm2, delta, par0):
    monkeypatch.setattr(lm_reference, "solve", lambda tiles, diag, pv: (None, np.array(sfun(pv) + (s2,)), None))
    monkeypatch.setattr(lm_reference, "gradient", lambda tiles, diag: (None, gnorm2))
    par, _, iters, trace = lm_reference.lmpar(None, None, delta, par0)
    return par, iters, trace


def rational(a, d):
    """s0(par) = sum (a_k / (d_k + par))^2, s1(par) = sum a_k^2 / (d_k + par)^3: what a diagonal problem gives."""
    a, d = np.asarray(a, float), np.asarray(d, float)
    return lambda pv: (float(np.sum((a / (d + pv)) ** 2)), float(np.sum(a * a / (d + pv) ** 3)))


SCALAR_CASES = {
    # name: (sfun, s2, gnorm2, delta, par0, what the case must show)
    "accepted at par = 0": (rational([1.0, 2.0], [1.0, 3.0]), 0.0, 5.0, 5.0, 0.0, lambda par, it, tr: par == 0.0 and it == 0),
    "a plain search": (rational([1.0, 2.0, 0.5], [1.0, 3.0, 0.1]), 0.0, 5.25, 0.3, 0.0, lambda par, it, tr: 0 < it < 10),
    "the start value clipped to paru": (rational([1.0, 2.0], [1.0, 3.0]), 0.0, 5.0, 0.5, 1e9,
                                        lambda par, it, tr: tr[1, 0] == np.sqrt(5.0) / 0.5),
    # s2 > 0 makes parl = 0; pass 1 overshoots (fp < 0) and pass 2 does no better: the second stopping rule ends it
    "parl = 0 with the second stopping rule": (lambda pv: (4.0, 1.0) if pv == 0.0 else (0.25, 1.0), 1.0, 4.0, 1.0, 0.0,
                                               lambda par, it, tr: it == 2 and np.sqrt(tr[2, 1]) - 1.0 < -0.1),
    # gnorm = 0 and parl = 0: paru = DBL_MIN / min(delta, 0.1), par = gnorm / dxnorm = 0 -> max(DBL_MIN, 0.001 paru) = DBL_MIN
    "the DBL_MIN branches": (lambda pv: (4.0, 1.0) if pv < 1e-300 else (1.0, 1.0), 1.0, 0.0, 1.0, 0.0,
                             lambda par, it, tr: tr[1, 0] == np.finfo(np.float64).tiny and it == 2),
    # s0 never reaches the region: ten passes
    "the cap at 10 passes": (lambda pv: (100.0 + 1.0 / (1.0 + pv), 1.0 + pv), 0.0, 1e4, 1.0, 0.0, lambda par, it, tr: it == 10),
}


@pytest.mark.parametrize("name", sorted(SCALAR_CASES))
def test_state_machine_matches_the_reference_loop_bit_for_bit(monkeypatch, name):
    sfun, s2, gnorm2, delta, par0, shows = SCALAR_CASES[name]
    want_par, want_iters, want_trace = run_reference(monkeypatch, sfun, s2, gnorm2, delta, par0)
    par, iters, trace = run_state_machine(sfun, s2, gnorm2, delta, par0)
    print(f"{name}: par {par!r} after {iters} passes; trace pars {trace[:, 0].tolist()}")
    assert shows(want_par, want_iters, want_trace), "the case does not reach the branch it is here for"
    assert iters == want_iters
    assert np.float64(par).tobytes() == np.float64(want_par).tobytes()
    assert trace.tobytes() == np.ascontiguousarray(want_trace, dtype=np.float64).tobytes()


# ---- the numpy prototype of the chain against the factor-free formulas -------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ref.GAUSSIAN))
def test_prototype_chain_matches_the_factor_free_formulas(name):
    p = ref.problem(name)
    f = ref.KeptFactors(p)
    worst = 0.0
    for diag in (None, p.norms):
        g, gnorm = ref.chain_gradient(f, diag)
        want_g, want_gnorm = ref.free_gradient(p.J, p.b, diag)
        assert np.allclose(g, want_g) and np.isclose(gnorm, want_gnorm)
        for par in (0.0, 1e-3, 1.0, 1e3):
            x, s0, s1 = ref.chain_evaluate(f, diag, par)
            wx, ws0, ws1 = ref.free_evaluate(p.J, p.b, diag, par)
            worst = max(worst, abs(s1 - ws1) / ws1)
            assert np.allclose(x, wx) and np.isclose(s0, ws0)
    print(f"{name}: s1 of the chain against u^T (J^T J + par D^2)^-1 u: worst {worst:.2e}")
    assert worst <= 1e-10
