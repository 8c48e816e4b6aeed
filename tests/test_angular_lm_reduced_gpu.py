"""GPU: the reduced route of BlockAngularSparseQR.lmSolve / lmpar -- the fill reduced to one triangle by
qrk_dense_qless_r before the right stack is factorised -- and the DenseQlessR facade.

Judges: numpy.linalg.lstsq on [J; sqrt(par) D] from the ORIGINAL matrix (lm_panel_reference.damped_lstsq), 1e-9 on x and on
|| D x ||^2; the stacked route on a second object, 2e-9 (two device results); factorizeAndSolve()'s x at par = 0, 1e-9.  lmpar on
the two routes: the same passes, par and every trace entry within 1e-9 relative (K12's bounds; its judge's stop margins are
2.5e-3 delta), x = lmSolve(diag, par) of the same route bit for bit.

Problems: those of tests/angular_lmpar_reference.py (m2 = 5, 24, 9 take the reduced route under "auto", 300 x (7 x 2) with m2 = 70
the stacked one) and 700 x (2 x 1) with m2 = 5: m1 = 700 is three level-1 chunks of qrk_dense_qless_r and a second level.
"""
import ctypes as C

import numpy as np
import pytest

import angular_lmpar_reference as ref
import lm_panel_reference as judge
from helpers import rel_fro
from oracle import oracle as orc
from test_angular_lm_gpu import assert_clear_pivots

pytestmark = pytest.mark.gpu

PARS = [0.0, 1e-3, 1.0, 1e3]
NAMES = ["8x(2x1)", "64x(7x2)", "20x(8x6)", "300x(7x2)", "ellipse", "700x(2x1)"]
FACTORS = [0.02, 0.1, 0.5, 2.0]
TALL_SEED = 5


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


def problem(name):
    if name != "700x(2x1)":
        return ref.problem(name)
    p = ref.gaussian_problem(700, 2, 1, 5, 0, TALL_SEED)
    assert_clear_pivots(orc.ba_factorize(orc.BDProblem.uniform(700, 2, 1, p.tiles), p.J2))
    return p


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def expected_route(p):
    return "reduced" if p.m2 + 1 <= 32 else "stacked"


@pytest.mark.parametrize("name", NAMES)
def test_lm_solve_reduced_matches_lstsq_and_the_stacked_route(qa, name):
    p = problem(name)
    ba, other = qa.BlockAngularSparseQR(), qa.BlockAngularSparseQR()
    x0 = ba.computeAndSolve(p.mat(qa), p.b)
    other.computeAndSolve(p.mat(qa), p.b)
    other.setLmRoute("stacked")
    assert ba.lmRoute() == expected_route(p) and other.lmRoute() == "stacked"
    if p.m1 == 700:
        lr = (C.c_int64 * 4)()
        assert qa._capi.lib().qrk_dense_qless_r_levels(p.m1, p.m2 + 1, lr, None, 4) == 2 and lr[1] == 3 * (p.m2 + 1)
    R_before = ba.matrixR().toarray()
    worst = np.zeros(4)
    for mode in ("none", "norms"):
        diag = None if mode == "none" else p.norms
        for par in PARS:
            x, dx2 = ba.lmSolve(diag, par, returnDxNorm2=True)
            want = judge.damped_lstsq(p.J, p.b, diag, par)
            D = np.ones_like(want) if diag is None else diag
            e = [rel_fro(x, want), abs(dx2 - np.sum((D * want) ** 2)) / np.sum((D * want) ** 2), rel_fro(x, other.lmSolve(diag, par)),
                 rel_fro(x, x0) if par == 0.0 else 0.0]
            print(f"{name} diag {mode} par {par:g}: x vs lstsq {e[0]:.2e}  |Dx|^2 {e[1]:.2e}  vs stacked {e[2]:.2e}  vs factorizeAndSolve {e[3]:.2e}")
            worst = np.maximum(worst, e)
            assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 2e-9 and e[3] <= 1e-9
            np.testing.assert_array_equal(ba.lmSolve(diag, par), x)               # repeated calls: equal bytes
    print(f"{name} ({ba.lmRoute()}) worst: x {worst[0]:.2e}  |Dx|^2 {worst[1]:.2e}  vs stacked {worst[2]:.2e}  par = 0 {worst[3]:.2e}")
    if expected_route(p) == "reduced":
        G = ba._lm["G"]
        assert ba._lm["route"] == "reduced" and tuple(G.shape) == (3 * p.m2 + 1, p.m2 + 1), "the big stack was allocated on the reduced route"
        assert "stacked" not in ba._lm_routes
    np.testing.assert_array_equal(ba.matrixR().toarray(), R_before)
    np.testing.assert_array_equal(ba.computeAndSolve(p.mat(qa), p.b), x0)


@pytest.mark.parametrize("name", ["8x(2x1)", "64x(7x2)", "20x(8x6)", "ellipse", "700x(2x1)"])
def test_lmpar_on_both_routes(qa, name):
    p = problem(name)
    ba, other = qa.BlockAngularSparseQR(), qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), p.b)
    other.computeAndSolve(p.mat(qa), p.b)
    ba.setLmRoute("reduced")
    other.setLmRoute("stacked")
    worst = np.zeros(2)
    for mode in ("none", "norms"):
        diag = None if mode == "none" else p.norms
        D = np.ones(p.m1 + p.m2) if diag is None else diag
        dx0 = np.linalg.norm(D * ref.free_evaluate(p.J, p.b, diag, 0.0)[0])
        for f in FACTORS:
            delta = f * dx0
            x, par, iters, trace = ba.lmpar(diag, delta, returnTrace=True)
            xs, pars, iterss, traces = other.lmpar(diag, delta, returnTrace=True)
            assert iters == iterss and trace.shape == traces.shape
            e = [rel(par, pars), max(rel(a, b) for a, b in zip(trace.ravel(), traces.ravel()))]
            print(f"{name} diag {mode} f {f:g}: par {par:.6e} vs stacked {e[0]:.1e} after {iters} passes, trace {e[1]:.1e}")
            worst = np.maximum(worst, e)
            assert e[0] <= 1e-9 and e[1] <= 1e-9
            np.testing.assert_array_equal(x, ba.lmSolve(diag, par))
            np.testing.assert_array_equal(xs, other.lmSolve(diag, pars))
    print(f"{name} worst: par {worst[0]:.2e}  trace {worst[1]:.2e}")


def wide_problem(m2):
    """40 blocks of 3 x 2 next to m2 dense columns (m1 = 80 > m2)"""
    return ref.gaussian_problem(40, 3, 2, m2, m2 + 4, 9)


def test_the_edge_of_the_reduced_route(qa):
    p31, p32 = wide_problem(31), wide_problem(32)
    ba = qa.BlockAngularSparseQR()
    assert ba.lmRoute.__doc__ and ba._lm_route == "auto"
    with pytest.raises(RuntimeError, match="lmRoute"):
        ba.lmRoute()                                          # "auto" depends on m2: no kept factors yet
    with pytest.raises(ValueError):
        ba.setLmRoute("fastest")
    ba.computeAndSolve(p31.mat(qa), p31.b)
    assert ba.lmRoute() == "reduced"
    assert rel_fro(ba.lmSolve(p31.norms, 0.5), judge.damped_lstsq(p31.J, p31.b, p31.norms, 0.5)) <= 1e-9
    ba.computeAndSolve(p32.mat(qa), p32.b)
    assert ba.lmRoute() == "stacked"
    want = judge.damped_lstsq(p32.J, p32.b, p32.norms, 0.5)
    x_auto = ba.lmSolve(p32.norms, 0.5)
    assert rel_fro(x_auto, want) <= 1e-9
    ba.setLmRoute("reduced")
    assert ba.lmRoute() == "reduced"
    with pytest.raises(RuntimeError, match="reduced"):
        ba.lmSolve(p32.norms, 0.5)
    with pytest.raises(RuntimeError, match="reduced"):
        ba.lmpar(p32.norms, 1.0)
    ba.setLmRoute("stacked")
    np.testing.assert_array_equal(ba.lmSolve(p32.norms, 0.5), x_auto)
    ba.setLmRoute("auto")
    np.testing.assert_array_equal(ba.lmSolve(p32.norms, 0.5), x_auto)


def test_switching_routes_gives_each_route_its_own_bits(qa):
    p = problem("64x(7x2)")
    ba = qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), p.b)
    got = {}
    for route in ("reduced", "stacked", "auto", "stacked", "reduced"):
        ba.setLmRoute(route)
        name = ba.lmRoute()
        x = ba.lmSolve(p.norms, 0.25)
        xp, par, iters = ba.lmpar(p.norms, 0.1 * np.linalg.norm(p.norms * ba.lmSolve(p.norms, 0.0)))
        key = (x.tobytes(), xp.tobytes(), par, iters)
        assert got.setdefault(name, key) == key, f"{name}: other bits after switching"
    assert set(got) == {"reduced", "stacked"}
    assert rel_fro(np.frombuffer(got["reduced"][0]), np.frombuffer(got["stacked"][0])) <= 2e-9


def test_device_right_hand_side_on_the_reduced_route(qa):
    import torch
    p = problem("20x(8x6)")
    ba = qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), torch.from_numpy(p.b).to("cuda"))
    assert ba.lmRoute() == "reduced"
    x = ba.lmSolve(torch.from_numpy(p.norms).to("cuda"), 0.5)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    assert rel_fro(x.cpu().numpy(), judge.damped_lstsq(p.J, p.b, p.norms, 0.5)) <= 1e-9


def test_dense_qless_r_facade(qa):
    import torch
    ctx = qa.Context(0)
    rng = np.random.default_rng(4)
    q = qa.DenseQlessR(ctx)
    for rows, cols in ((700, 6), (700, 6), (4097, 17)):
        A = rng.standard_normal((rows + 3, cols))
        dA = torch.from_numpy(np.ascontiguousarray(A.T)).to(ctx.device).t()        # column-major (rows + 3) x cols
        work = q._work
        R = q.compute(dA[:rows]).matrixR().cpu().numpy()                           # a window: lda = rows + 3
        assert R.shape == (cols, cols) and (q.rows(), q.cols()) == (rows, cols) and not np.tril(R, -1).any()
        G = A[:rows].T @ A[:rows]
        assert np.max(np.abs(R.T @ R - G)) <= 1e-11 * max(1.0, np.max(np.abs(G)))
        if (rows, cols) == (700, 6) and work is not None:
            assert q._work is work, "the workspace is kept between calls of one shape"
    with pytest.raises(qa.QrkError):
        q.compute(torch.zeros(33, 64, dtype=torch.float64, device=ctx.device).t())  # 33 columns
