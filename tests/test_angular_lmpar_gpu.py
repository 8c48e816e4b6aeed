"""GPU: BlockAngularSparseQR.lmpar / lmGradient -- MINPACK's lmpar on the factors factorizeAndSolve() keeps.

The judge (tests/angular_lmpar_reference.py) uses no factor at all: lmpar's loop over x = lstsq on [J; sqrt(par) D],
s0 = || D x ||^2, s1 = u^T (J^T J + par D^2)^-1 u with u = D^2 x, and gnorm = || D^-1 J^T b ||, all from the ORIGINAL J and b.
Problems: the Gaussian block-angular matrices and the ellipse of tests/test_angular_lm_gpu.py (restated in the reference module)
plus 300 x (7 x 2) with m2 = 70, each with diag = None and with the column norms, at delta = f || D x0 ||, f in {0.02, 0.1, 0.5, 2}.

Required: the same number of passes; par and every trace row within 1e-9 relative; x within rel_fro 1e-9; | || D x || - delta | <=
0.1 delta whenever fewer than 10 passes ran; f = 2 gives par = 0, no pass and the undamped solution.  So that none of this rests on
a lucky radius every case first asserts that no stop decision of the judge lies within 1e-6 delta of its threshold 0.1 delta (on the
CPU the smallest margin over the 40 cases is 2.5e-3 delta, 300 x (7 x 2) without diag at f = 0.02; the ellipse's smallest is
5.6e-2 delta, so its radii are the same four).  The judge takes 0, 2 or 3 passes.
"""
import numpy as np
import pytest

import angular_lmpar_reference as ref
from helpers import rel_fro

pytestmark = pytest.mark.gpu

NAMES = ["8x(2x1)", "64x(7x2)", "20x(8x6)", "300x(7x2)", "ellipse"]
FACTORS = [0.02, 0.1, 0.5, 2.0]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


@pytest.mark.parametrize("name", NAMES)
def test_lmpar_matches_the_factor_free_judge(qa, name):
    p = ref.problem(name)
    ba = qa.BlockAngularSparseQR()
    x0 = ba.computeAndSolve(p.mat(qa), p.b)
    assert ba.info() == 0 and ba._lm_ready
    R_before = ba.matrixR().toarray()
    worst = np.zeros(5)
    for mode in ("none", "norms"):
        diag = None if mode == "none" else p.norms
        D = np.ones(p.m1 + p.m2) if diag is None else diag
        # lmGradient against J^T b
        g, gnorm = ba.lmGradient(diag)
        want_g, want_gnorm = ref.free_gradient(p.J, p.b, diag)
        eg, en = rel_fro(g, want_g), rel(gnorm, want_gnorm)
        worst[3:] = np.maximum(worst[3:], [eg, en])
        assert isinstance(g, np.ndarray) and eg <= 1e-11 and en <= 1e-11, (eg, en)
        dx0 = np.linalg.norm(D * ref.free_evaluate(p.J, p.b, diag, 0.0)[0])
        for f in FACTORS:
            delta = f * dx0
            want_par, want_x, want_iters, want_trace, margin = ref.free_lmpar(p.J, p.b, diag, delta)
            assert margin > 1e-6 * delta, f"a stop decision of the judge hangs on rounding (margin {margin / delta:.2e} delta): choose another f"
            x, par, iters, trace = ba.lmpar(diag, delta, returnTrace=True)
            e = [rel(par, want_par), max(rel(a, b) for a, b in zip(trace.ravel(), want_trace.ravel())) if iters == want_iters else np.inf,
                 rel_fro(x, want_x)]
            print(f"{name} diag {mode} f {f:g}: par {par:.6e} ({e[0]:.1e}) after {iters} passes (judge {want_iters}), trace {e[1]:.1e}, "
                  f"x {e[2]:.1e}, margin {margin / delta:.1e} delta")
            assert iters == want_iters and trace.shape == (iters + 1, 3)
            worst[:3] = np.maximum(worst[:3], e)
            assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 1e-9
            if iters < 10:
                assert abs(np.linalg.norm(D * x) - delta) <= 0.1 * delta or par == 0.0
            if f == 2.0:
                assert par == 0.0 and iters == 0 and rel_fro(x, x0) <= 1e-9
            else:
                assert par > 0.0 and abs(np.linalg.norm(D * x) - delta) <= 0.1 * delta
            # the step is lmSolve's at the returned par, bit for bit; a second call repeats everything to the bit
            np.testing.assert_array_equal(x, ba.lmSolve(diag, par))
            x2, par2, iters2, trace2 = ba.lmpar(diag, delta, returnTrace=True)
            assert par2 == par and iters2 == iters and trace2.tobytes() == trace.tobytes() and x2.tobytes() == x.tobytes()
            assert len(ba.lmpar(diag, delta)) == 3
    print(f"{name} worst: par {worst[0]:.2e}  trace {worst[1]:.2e}  x {worst[2]:.2e}  g {worst[3]:.2e}  gnorm {worst[4]:.2e}")
    # W is intact: the factors read the same, and the next factorisation gives the bits it gave before
    np.testing.assert_array_equal(ba.matrixR().toarray(), R_before)
    np.testing.assert_array_equal(ba.computeAndSolve(p.mat(qa), p.b), x0)


def test_lmsolve_is_unchanged_by_the_shared_evaluation(qa):
    """lmSolve()'s body moved into the evaluation lmpar() shares: interleaving the two does not change a bit of lmSolve()'s x, and
    a start value above the root is taken (par in, par out)."""
    p = ref.problem("64x(7x2)")
    ba, other = qa.BlockAngularSparseQR(), qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), p.b)
    other.computeAndSolve(p.mat(qa), p.b)
    dx0 = np.linalg.norm(p.norms * ba.lmSolve(p.norms, 0.0))
    for par in (0.0, 1e-3, 1.0, 1e3):
        before = other.lmSolve(p.norms, par)                         # an object that never ran lmpar()
        ba.lmpar(p.norms, 0.1 * dx0)
        ba.lmGradient(None)
        np.testing.assert_array_equal(ba.lmSolve(p.norms, par), before)
    x, par, iters = ba.lmpar(p.norms, 0.1 * dx0, par=1e9)            # clipped to paru, then the search
    assert par > 0.0 and 1 <= iters < 10 and abs(np.linalg.norm(p.norms * x) - 0.1 * dx0) <= 0.01 * dx0


def test_device_right_hand_side(qa):
    import torch
    p = ref.problem("20x(8x6)")
    ba = qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), torch.from_numpy(p.b).to("cuda"))
    dx0 = np.linalg.norm(p.norms * ref.free_evaluate(p.J, p.b, p.norms, 0.0)[0])
    x, par, iters = ba.lmpar(torch.from_numpy(p.norms).to("cuda"), 0.1 * dx0)
    g, gnorm = ba.lmGradient()
    assert isinstance(x, torch.Tensor) and x.is_cuda and isinstance(g, torch.Tensor) and g.is_cuda and isinstance(gnorm, float)
    want_par, want_x, want_iters, _, _ = ref.free_lmpar(p.J, p.b, p.norms, 0.1 * dx0)
    assert iters == want_iters and rel(par, want_par) <= 1e-9 and rel_fro(x.cpu().numpy(), want_x) <= 1e-9
    assert rel_fro(g.cpu().numpy(), p.J.T @ p.b) <= 1e-11


def test_refusals(qa):
    p = ref.problem("8x(2x1)")
    ba = qa.BlockAngularSparseQR()
    with pytest.raises(RuntimeError, match="lmpar"):
        ba.lmpar(None, 1.0)
    with pytest.raises(RuntimeError, match="lmGradient"):
        ba.lmGradient()
    ba.compute(p.mat(qa))                                            # the explicit route keeps no factors
    with pytest.raises(RuntimeError, match="lmpar"):
        ba.lmpar(None, 1.0)
    with pytest.raises(RuntimeError, match="lmGradient"):
        ba.lmGradient()
    ba.computeAndSolve(p.mat(qa), p.b)
    for delta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ba.lmpar(None, delta)
    for par in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            ba.lmpar(None, 1.0, par)
    assert len(ba.lmpar(None, 1.0)) == 3                             # still usable


def test_a_zero_diagonal_at_par_0_is_refused(qa):
    """Rank-deficient undamped factors are out of scope: a left tile whose column is zero raises a clear error."""
    p = ref.problem("8x(2x1)")
    tiles = p.tiles.copy()
    tiles[6:8] = 0.0                                                 # tile 3 is the zero column
    left = qa.SparseBlockDiagonal.fromTiles(np.full(8, 2, np.int32), np.full(8, 1, np.int32), tiles, rows=16)
    ba = qa.BlockAngularSparseQR()
    ba.computeAndSolve(qa.BlockMatrix1x2(left, p.J2), p.b)
    with pytest.raises(RuntimeError, match="zero on the diagonal"):
        ba.lmpar(None, 1.0)


class DeviceStepper:
    def __init__(self, qa):
        self.qa, self.ba = qa, qa.BlockAngularSparseQR()
        self.rows, self.cols = np.full(ref.NPTS, 2, np.int32), np.full(ref.NPTS, 1, np.int32)

    def factorize(self, tiles, J2, rhs):
        self.ba.computeAndSolve(self.qa.BlockMatrix1x2(self.qa.SparseBlockDiagonal.fromTiles(self.rows, self.cols, tiles), J2), rhs)

    def lmpar(self, diag, delta, par):
        x, par, _ = self.ba.lmpar(diag, delta, par)
        return x, par


@pytest.mark.parametrize("scale,budget", [(1.0, 10), (8.0, 20)])
def test_trust_region_fit_of_the_ellipse(qa, scale, budget):
    """A trust-region fit (reference module: trust_region_fit, the loop of tests/test_lmpar_gpu.py's fit with MINPACK's ratio test
    and radius update) with one computeAndSolve per accepted iterate and one lmpar per trial step, from ellipse_data()'s start and
    from a start eight times as far from the generating parameters.

    The same loop with the factor-free judge in place of the solver (run first, on the CPU) takes 7 trial steps on 7 factorisations
    from the start itself and 14 trial steps on 13 factorisations from the start scaled by 8, and ends at a cost below 1e-28 both
    times; the budgets of 10 and 20 trial steps come from those counts."""
    truth, pts, start = ref.ellipse_data()
    s = truth + scale * (start - truth)
    _, jcost, jfact, jtrials = ref.trust_region_fit(s, pts, ref.JudgeStepper(), budget)
    uv, cost, factorisations, trials = ref.trust_region_fit(s, pts, DeviceStepper(qa), budget)
    print(f"start x {scale:g}: cost {cost:.2e} after {trials} trial steps on {factorisations} factorisations "
          f"(judge: {jcost:.2e}, {jtrials} on {jfact})")
    assert jcost < 1e-20
    assert cost < 1e-20
    assert np.max(np.abs(uv[ref.NPTS:] - truth[ref.NPTS:])) < 1e-8
    assert factorisations <= trials <= budget
