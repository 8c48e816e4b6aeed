"""GPU: MINPACK's lmpar on the block-diagonal factors (qrk_bd_lmpar; BlockDiagonalSparseQR.lmpar) against the numpy loop of
lm_reference.py, fed the same R, permutation and Q^T b, and an end-to-end trust-region fit on undamped tiles.

delta = f || D x0 || with x0 the Gauss-Newton step: f = 2 leaves it inside the region (par = 0, no pass of the loop), the smaller f
need a damping.  The pass count is the reference loop's and at most 5; every traced (par, || D x ||^2, sums[1]) agrees with the
judge evaluated AT THE TRACED par to 1e-9; the returned x is the judge's x at the returned par within the x tolerance of
test_lm_solve_gpu.py (1e-11 per tile on (0.5, 5.0) data, 1e-9 on (-1, 1) data).
"""
import functools

import numpy as np
import pytest

import lm_reference as judge
from helpers import seeded_tiles

pytestmark = pytest.mark.gpu

CASES = [(300, 7, 2, 0.5, 5.0, 1e-11), (50, 5, 1, 0.5, 5.0, 1e-11), (300, 8, 6, -1.0, 1.0, 1e-9)]
FACTORS = [2.0, 0.5, 0.1, 0.01]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


class Problem:
    def __init__(self, qa, ctx, B, r, c, lo, hi):
        rows, self.cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, self.cols, seeded_tiles(1 + r + c, lo, hi, B * r * c))
        self.qr = qa.BlockDiagonalSparseQR(context=ctx)
        f = np.random.default_rng(10 * r + c).uniform(-1.0, 1.0, B * r)
        self.x0, self.qtb = self.qr.computeAndSolve(mat, f, returnQtB=True)       # the Q-less route: no Q anywhere below
        self.t = judge.Tiles(self.cols, self.qr.rValues().cpu().numpy(), self.qr.colsPermutation(), self.qtb)
        norms = self.qr.colNorms()
        self.diag = np.where(norms == 0.0, 1.0, norms)
        self.dx0 = float(np.linalg.norm(self.diag * judge.solve(self.t, self.diag, 0.0)[0]))


@functools.lru_cache(maxsize=None)
def problem(qa, ctx, B, r, c, lo, hi):
    return Problem(qa, ctx, B, r, c, lo, hi)


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@pytest.mark.parametrize("B,r,c,lo,hi,xtol", CASES)
@pytest.mark.parametrize("f", FACTORS)
def test_lmpar_matches_the_reference_loop(qa, ctx, B, r, c, lo, hi, xtol, f):
    p = problem(qa, ctx, B, r, c, lo, hi)
    delta = f * p.dx0
    par, x, iters, trace = p.qr.lmpar(p.qtb, p.diag, delta, returnTrace=True)
    want_par, _, want_iters, want_trace = judge.lmpar(p.t, p.diag, delta)
    print(f"f = {f}: par {par:.6e} (reference {want_par:.6e}), passes {iters} (reference {want_iters})")
    assert iters == want_iters and iters <= 5
    assert trace.shape == (iters + 1, 3) and trace[0, 0] == 0.0
    if f == 2.0:
        assert par == 0.0 and iters == 0
    else:
        assert par > 0.0 and par == trace[-1, 0]
        assert abs(np.linalg.norm(p.diag * x) - delta) <= 0.1 * delta
        assert rel(par, want_par) <= 1e-9
    for pv, s0, s1 in trace:                                  # every evaluation, at the par the device used
        _, s, _ = judge.solve(p.t, p.diag, pv)
        assert rel(s0, s[0]) <= 1e-9 and rel(s1, s[1]) <= 1e-9, (pv, s0, s1, s)
    want_x, _, _ = judge.solve(p.t, p.diag, par)
    err = judge.per_tile_rel(x, want_x, p.t)
    print(f"x per tile {err:.2e}")
    assert err <= xtol


def test_start_value_is_clamped(qa, ctx):
    """A start value above paru = || D^-1 g || / delta or below parl enters the loop as the bound."""
    p = problem(qa, ctx, 300, 7, 2, 0.5, 5.0)
    delta = 0.1 * p.dx0
    gnorm = np.sqrt(judge.gradient(p.t, p.diag)[1])
    _, _, _, trace = p.qr.lmpar(p.qtb, p.diag, delta, par=1e30, returnTrace=True)
    assert rel(trace[1, 0], gnorm / delta) <= 1e-12
    s = judge.solve(p.t, p.diag, 0.0)[1]
    parl = (p.dx0 - delta) / (delta * s[1] / s[0])
    assert parl > 0.0
    par, x, iters, trace = p.qr.lmpar(p.qtb, p.diag, delta, par=1e-300, returnTrace=True)
    assert rel(trace[1, 0], parl) <= 1e-9
    want = judge.lmpar(p.t, p.diag, delta, par=1e-300)
    assert iters == want[2] and rel(par, want[0]) <= 1e-9
    assert abs(np.linalg.norm(p.diag * x) - delta) <= 0.1 * delta
    # diag = None is D = I
    par1, x1, _ = p.qr.lmpar(p.qtb, None, 0.5 * np.linalg.norm(p.x0))
    par2, x2, _ = p.qr.lmpar(p.qtb, np.ones(p.t.n), 0.5 * np.linalg.norm(p.x0))
    assert par1 == par2 and par1 > 0.0
    np.testing.assert_array_equal(x1, x2)


def test_trust_region_fit_on_undamped_tiles(qa):
    """test_qless_gpu.test_lm_loop_with_factorize_and_solve's curve fits y = exp(a t) + b, but on the UNDAMPED 7 x 2 tiles: one
    factorizeAndSolve(returnQtB=True) per Jacobian, lmpar for the step (no second factorisation for a trial damping), and MINPACK's
    plain update of the trust region.  The plan is analysed once."""
    B = 500
    rng = np.random.default_rng(5)
    t = np.linspace(0.0, 1.0, 7)
    a_true, b_true = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    y = np.exp(a_true[:, None] * t) + b_true[:, None]
    qr = qa.BlockDiagonalSparseQR(context=qa.Context(0))
    rows, cols = np.full(B, 7, np.int32), np.full(B, 2, np.int32)
    a, b = np.zeros(B), np.zeros(B)

    def residual(a, b):
        return np.exp(a[:, None] * t) + b[:, None] - y          # (B, 7)

    cost = 0.5 * np.sum(residual(a, b) ** 2)
    plan_before, delta, par, diag = None, None, 0.0, None
    factorizations = damped_steps = 0
    for it in range(40):
        r = residual(a, b)
        J = np.zeros((B, 2, 7))                                   # column-major 7x2 tiles
        J[:, 0, :] = t * np.exp(a[:, None] * t)                   # d/da
        J[:, 1, :] = 1.0                                          # d/db
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, J.ravel())
        if plan_before is None:
            qr.analyzePattern(mat)
            plan_before = qr._plan.value
            assert "bdqr_thin_rhs_kernel" in qr.rhsKernelName(1) and "bd_lm_thin_kernel" in qr.lmKernelName()
        qtb = qr.factorizeAndSolve(mat, (-r).ravel(), returnQtB=True, solve=False)
        factorizations += 1
        assert qr._plan.value == plan_before                      # the pattern analysis is reused
        norms = qr.colNorms()
        diag = np.where(norms == 0.0, 1.0, norms) if diag is None else np.maximum(diag, norms)
        if delta is None:
            delta = 1.0                                           # a small region: the first steps are damped ones
        for inner in range(20):                                   # trial steps on the SAME factors
            par, dx, _ = qr.lmpar(qtb, diag, delta, par)
            dx = dx.reshape(B, 2)
            damped_steps += par > 0.0
            pnorm = np.linalg.norm(diag * dx.ravel())
            new_cost = 0.5 * np.sum(residual(a + dx[:, 0], b + dx[:, 1]) ** 2)
            lin = r + np.einsum("bcr,bc->br", J, dx)
            predicted = cost - 0.5 * np.sum(lin ** 2)
            ratio = (cost - new_cost) / predicted if predicted > 0 else 0.0
            if ratio <= 0.25:
                delta = 0.5 * min(delta, pnorm)
            elif par == 0.0 or ratio >= 0.75:
                delta = 2.0 * pnorm
            if ratio >= 1e-4:
                a, b, cost = a + dx[:, 0], b + dx[:, 1], new_cost
                break
        if cost < 1e-24:
            break
    print(f"{factorizations} factorisations, {damped_steps} damped steps, cost {cost:.2e}")
    assert damped_steps >= 3                                      # (the numpy loop takes five before the region stops binding)
    assert np.max(np.abs(a - a_true)) < 1e-8 and np.max(np.abs(b - b_true)) < 1e-8
