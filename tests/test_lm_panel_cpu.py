"""CPU: the entry points of the block-angular damped solve (qrk_bd_lm_panel, qrk_bd_lm_panel_kernel_name, qrk_dense_lm_stack) reject
NULL arguments before they touch a device; the numpy judge of the GPU tests (lm_panel_reference.py) reproduces lstsq."""
import numpy as np


def test_null_arguments_are_rejected_without_a_gpu():
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    I = capi.STATUS_INVALID_ARGUMENT
    assert lib.qrk_bd_lm_panel(None, None, None, None, 0.0, None, 0, 0, None, None, None, 0, None, 0) == I
    assert lib.qrk_bd_lm_panel(None, None, None, None, 1.0, None, 4, 1, None, None, None, 4, None, 4) == I
    assert lib.qrk_dense_lm_stack(None, None, 0, 0, None, None, None, 0.0, 0, None, 0) == I
    assert lib.qrk_dense_lm_stack(None, None, 3, 3, None, None, None, 1.0, 2, None, 8) == I
    assert lib.qrk_bd_lm_panel_kernel_name(None, 1) == b""
    for name in ("qrk_bd_lm_panel", "qrk_bd_lm_panel_kernel_name", "qrk_dense_lm_stack"):
        assert name in capi.EXPORTS


def hand_sized_factors():
    """Two 3 x 1 tiles next to one dense column (m2 = 1), factorised with numpy in the layout the solver keeps: the first entry of
    every tile's Q_t^T rows at the tile's column, the others behind the m1 columns, then the QR of what lies below."""
    rng = np.random.default_rng(5)
    tiles = [rng.standard_normal((3, 1)) for _ in range(2)]
    J2, b = rng.standard_normal((6, 1)), rng.standard_normal(6)
    J = np.zeros((6, 3))
    J[0:3, 0:1], J[3:6, 1:2], J[:, 2:] = tiles[0], tiles[1], J2
    Rs, top, rest = [], [], []
    for t, T in enumerate(tiles):
        Q, R = np.linalg.qr(T, mode="complete")
        Rs.append(R[:1, :1])
        w = Q.T @ np.hstack([J2[3 * t:3 * t + 3], b[3 * t:3 * t + 3, None]])
        top.append(w[:1]); rest.append(w[1:])
    top, rest = np.vstack(top), np.vstack(rest)                     # m1 x (m2 + 1), (rows - m1) x (m2 + 1)
    Q2, R2 = np.linalg.qr(rest[:, :1], mode="complete")
    y2 = (Q2.T @ rest[:, 1])[:1]
    return J, b, Rs, top[:, :1], R2[:1, :1], top[:, 1], y2


def test_the_judge_reproduces_lstsq_on_a_hand_sized_problem():
    import lm_panel_reference as judge
    J, b, Rs, strip, R2, y1, y2 = hand_sized_factors()
    diag = np.linalg.norm(J, axis=0)
    for par in (0.0, 1e-3, 0.7, 1e3):
        for d in (None, diag):
            x = judge.damped_solve(Rs, [0, 1], strip, R2, [0], y1, y2, d, par)
            want = judge.damped_lstsq(J, b, d, par)
            err = np.linalg.norm(x - want) / np.linalg.norm(want)
            print(f"par {par:g} diag {'norms' if d is not None else 'none'}: {err:.2e}")
            assert err <= 1e-14


def test_the_judge_helpers():
    import lm_panel_reference as judge
    Rs = judge.unpack_tiles([1, 2], np.array([3.0, 2.0, 1.0, -4.0]))
    np.testing.assert_array_equal(Rs[0], [[3.0]])
    np.testing.assert_array_equal(Rs[1], [[2.0, 1.0], [0.0, -4.0]])
    C = np.array([[1.0, 2.0], [3.0, -1.0]])
    S, top, fill = judge.tile_step(Rs[1], np.array([1.0, 2.0]), 0.5, C)
    np.testing.assert_allclose(S.T @ S, Rs[1].T @ Rs[1] + 0.5 * np.diag([1.0, 4.0]), rtol=1e-14)
    np.testing.assert_allclose(top.T @ top + fill.T @ fill, C.T @ C, rtol=1e-14)
    S2, top2 = judge.match_signs(S, top, np.array([-1.0, 1.0]))
    assert S2[0, 0] < 0 and S2[1, 1] > 0
    np.testing.assert_allclose(np.abs(top2), np.abs(top))
