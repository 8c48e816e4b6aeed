"""CPU: the Levenberg-Marquardt entry points of the C ABI (qrk_bd_lm_solve, qrk_bd_lm_gradient, qrk_bd_r_col_norms, qrk_bd_lmpar,
qrk_bd_lm_kernel_name) reject NULL arguments before they touch a device; the judge of the GPU tests agrees with itself."""
import ctypes as C

import numpy as np


def test_null_arguments_are_rejected_without_a_gpu():
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    I = capi.STATUS_INVALID_ARGUMENT
    assert lib.qrk_bd_lm_solve(None, None, None, None, None, 0.0, None, None, capi.MEM_DEVICE) == I
    assert lib.qrk_bd_lm_solve(None, None, None, None, None, 0.0, None, None, capi.MEM_HOST) == I
    assert lib.qrk_bd_lm_gradient(None, None, None, None, None, None, None, capi.MEM_DEVICE) == I
    assert lib.qrk_bd_r_col_norms(None, None, None, None, capi.MEM_DEVICE) == I
    par = C.c_double(0.0)
    assert lib.qrk_bd_lmpar(None, None, None, None, None, 1.0, C.byref(par), None, None, None) == I
    assert lib.qrk_bd_lmpar(None, None, None, None, None, 1.0, None, None, None, None) == I
    assert lib.qrk_bd_lm_kernel_name(None) == b""
    for name in ("qrk_bd_lm_solve", "qrk_bd_lm_gradient", "qrk_bd_r_col_norms", "qrk_bd_lmpar", "qrk_bd_lm_kernel_name"):
        assert name in capi.EXPORTS


def test_the_judge_on_a_problem_with_a_known_answer():
    """lm_reference.py on one 2 x 2 tile worked by hand: R = [[2, 1], [0, 1]], perm = (1, 0), y = (2, 1), D = I.
    par = 0: z = R^-1 y = (0.5, 1), x = P z = (1, 0.5).  The normal equations (R^T R + par I) z = R^T y give the damped z."""
    import lm_reference as judge
    t = judge.Tiles([2], np.array([2.0, 1.0, 1.0]), [1, 0], [2.0, 1.0])
    x, s, _ = judge.solve(t, None, 0.0)
    np.testing.assert_allclose(x, [1.0, 0.5], rtol=1e-15)
    assert abs(s[0] - 1.25) < 1e-15 and s[2] == 0.0
    R = np.array([[2.0, 1.0], [0.0, 1.0]])
    assert abs(s[1] - np.sum(np.linalg.solve(R.T, [0.5, 1.0]) ** 2)) < 1e-15
    x, s, _ = judge.solve(t, None, 0.5)
    z = np.linalg.solve(R.T @ R + 0.5 * np.eye(2), R.T @ [2.0, 1.0])
    np.testing.assert_allclose(x, z[[1, 0]], rtol=1e-14)
    g, gn2 = judge.gradient(t, None)
    np.testing.assert_allclose(g, (R.T @ [2.0, 1.0])[[1, 0]])
    np.testing.assert_allclose(judge.col_norms(t), [np.sqrt(2.0), 2.0])
    # lmpar: a region of half the Gauss-Newton step is met within 10 %, one of twice the step needs no damping
    full = np.sqrt(1.25)
    par, x, iters, trace = judge.lmpar(t, None, 0.5 * full)
    assert par > 0 and 1 <= iters <= 5 and abs(np.linalg.norm(x) - 0.5 * full) <= 0.05 * full and len(trace) == iters + 1
    assert judge.lmpar(t, None, 2.0 * full)[0] == 0.0
    # a zero on the diagonal: the nsing rule
    t0 = judge.Tiles([2], np.array([2.0, 1.0, 0.0]), [0, 1], [2.0, 1.0])
    x, s, _ = judge.solve(t0, None, 0.0)
    np.testing.assert_allclose(x, [1.0, 0.0])
    assert s[1] == 0.0 and s[2] == 1.0
