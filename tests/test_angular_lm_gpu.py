"""GPU: BlockAngularSparseQR.lmSolve -- the damped solve at a trial par on the factors factorizeAndSolve() keeps.

The judge is numpy.linalg.lstsq on [J; sqrt(par) D] built from the ORIGINAL J1, J2 and b: independent of every factor.  x is judged
by rel_fro <= 1e-9 (the project's bound for x in tests/test_angular.py), 2e-9 against the parent's route (computeAndSolve on the
damped matrix: two device results).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lm_panel_reference as judge
from helpers import rel_fro
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

PARS = [0.0, 1e-3, 1.0, 1e3]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


def assert_clear_pivots(res, rel=1e-9):
    """Every pivot step of the right block has a clear winner (the oracle's R2: the chosen column's remaining norm exceeds the
    runner-up's by more than `rel`), so the device and the oracle cannot disagree on the order: no case depends on a lucky seed."""
    m2 = res.m2
    R2 = np.triu(res.qr2[:m2, :])
    rem = np.sqrt(np.cumsum((R2 ** 2)[::-1], axis=0)[::-1])
    for k in range(m2 - 1):
        win, runner = rem[k, k], rem[k, k + 1:].max()
        assert win > runner * (1.0 + rel), f"pivot step {k}: winner {win!r} against runner-up {runner!r}: choose another seed"


class Problem:
    """[J1 | J2] x = b with J1 = num_vars blocks of r x c (column-major tiles) and n2 rows below them"""

    def __init__(self, num_vars, r, c, m2, n2, tiles, J2, b):
        self.num_vars, self.r, self.c, self.m2, self.n2 = num_vars, r, c, m2, n2
        self.tiles, self.J2, self.b = tiles, J2, b
        self.blocks = [tiles[i * r * c:(i + 1) * r * c].reshape(c, r).T for i in range(num_vars)]
        J1 = sp.block_diag(self.blocks, format="csc").toarray()
        if n2:
            J1 = np.vstack([J1, np.zeros((n2, c * num_vars))])
        self.J = np.hstack([J1, J2])
        self.m1 = c * num_vars
        self.norms = np.linalg.norm(self.J, axis=0)

    def mat(self, qa, form="dense"):
        left = qa.SparseBlockDiagonal.fromTiles(np.full(self.num_vars, self.r, np.int32), np.full(self.num_vars, self.c, np.int32),
                                                self.tiles, rows=self.r * self.num_vars)
        right = self.J2 if form == "dense" else sp.csr_matrix(self.J2)
        return qa.BlockMatrix1x2(left, right)

    def damped(self, qa, diag, par):
        """The parent commit's route for one trial damping: the damped matrix in block-angular form -- sqrt(par) D_t below every
        left tile (zero rows in J2 and b next to them), sqrt(par) D2 below J2 -- for computeAndSolve()."""
        D = np.ones(self.m1 + self.m2) if diag is None else diag
        r, c, nv, m2 = self.r, self.c, self.num_vars, self.m2
        sq = np.sqrt(par)
        tiles = np.concatenate([np.vstack([self.blocks[i], sq * np.diag(D[i * c:(i + 1) * c])]).T.ravel() for i in range(nv)])
        J2 = np.zeros((nv, r + c, m2)); J2[:, :r, :] = self.J2[:nv * r].reshape(nv, r, m2)
        J2 = np.vstack([J2.reshape(nv * (r + c), m2), self.J2[nv * r:], sq * np.diag(D[self.m1:])])
        b = np.zeros((nv, r + c)); b[:, :r] = self.b[:nv * r].reshape(nv, r)
        b = np.concatenate([b.ravel(), self.b[nv * r:], np.zeros(m2)])
        left = qa.SparseBlockDiagonal.fromTiles(np.full(nv, r + c, np.int32), np.full(nv, c, np.int32), tiles, rows=(r + c) * nv)
        return qa.BlockMatrix1x2(left, J2), b


@functools.lru_cache(maxsize=None)
def gaussian_problem(num_vars, r, c, m2, n2, seed):
    rng = np.random.default_rng(seed)
    tiles = rng.standard_normal(num_vars * r * c)
    J2 = rng.standard_normal((num_vars * r + n2, m2))
    p = Problem(num_vars, r, c, m2, n2, tiles, J2, rng.standard_normal(num_vars * r + n2))
    assert_clear_pivots(orc.ba_factorize(orc.BDProblem.uniform(num_vars, r, c, tiles), J2))
    return p


# ---- the ellipse of examples/ellipse_fitting.cpp, restated ------------------------------------------------------------------------

NPTS = 300


def ellipse_model(uv):
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    return np.stack([a * np.cos(t) * np.cos(r) - b * np.sin(t) * np.sin(r) + x0,
                     a * np.cos(t) * np.sin(r) + b * np.sin(t) * np.cos(r) + y0])


def ellipse_jacobian(uv, pts):
    """The UNDAMPED Jacobian of EllipseFitting (examples/ellipse_fitting.cpp:46-96) in block-angular form: one 2 x 1 block per point
    (d f_i / d t_i) next to the 5 ellipse parameters; returns (tiles, J2, -f)."""
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    f = (pts - ellipse_model(uv)).T
    ct, st, cr, sr = np.cos(t), np.sin(t), np.cos(r), np.sin(r)
    tiles = np.zeros((NPTS, 1, 2))
    tiles[:, 0, 0] = a * cr * st + b * sr * ct
    tiles[:, 0, 1] = a * sr * st - b * cr * ct
    J2 = np.zeros((NPTS, 2, 5))
    J2[:, 0, :] = np.stack([-ct * cr, st * sr, -np.ones(NPTS), np.zeros(NPTS), a * ct * sr + b * st * cr], axis=1)
    J2[:, 1, :] = np.stack([-ct * sr, -st * cr, np.zeros(NPTS), -np.ones(NPTS), -a * ct * cr + b * st * sr], axis=1)
    return tiles.ravel(), J2.reshape(2 * NPTS, 5), -f.ravel()


def ellipse_data():
    rng = np.random.default_rng(11)
    truth = np.concatenate([np.sort(rng.uniform(0.0, 2.0 * np.pi, NPTS)), [3.0, 2.0, 0.5, -0.3, 0.4]])
    pts = ellipse_model(truth)                                     # noise-free
    start = truth + np.concatenate([0.05 * rng.standard_normal(NPTS), [0.3, -0.2, 0.1, 0.1, -0.1]])
    return truth, pts, start


@functools.lru_cache(maxsize=None)
def ellipse_problem():
    _, pts, start = ellipse_data()
    tiles, J2, rhs = ellipse_jacobian(start, pts)
    return Problem(NPTS, 2, 1, 5, 0, tiles, J2, rhs)


def problems():
    return {"8x(2x1)": lambda: gaussian_problem(8, 2, 1, 5, 0, 1), "64x(7x2)": lambda: gaussian_problem(64, 7, 2, 24, 3, 2),
            "20x(8x6)": lambda: gaussian_problem(20, 8, 6, 9, 2, 3), "ellipse": ellipse_problem}


# ---- lmSolve against lstsq ---------------------------------------------------------------------------------------------------------------

def check_problem(qa, p, form="dense", parent=True):
    ba = qa.BlockAngularSparseQR()
    with pytest.raises(RuntimeError, match="lmSolve"):
        ba.lmSolve(None, 1.0)
    x0 = ba.computeAndSolve(p.mat(qa, form), p.b)
    assert ba.info() == 0 and ba._lm_ready
    name = qa._capi.lib().qrk_bd_lm_panel_kernel_name(ba.m_leftSolver._plan, p.m2 + 1).decode()
    assert ("thin" in name) == (p.c <= 2) and "unsupported" not in name
    R_before = ba.matrixR().toarray()
    worst = np.zeros(4)
    other = qa.BlockAngularSparseQR()
    for mode in ("none", "norms"):
        diag = None if mode == "none" else p.norms
        for par in PARS:
            x, dx2 = ba.lmSolve(diag, par, returnDxNorm2=True)
            assert isinstance(x, np.ndarray) and x.shape == (p.m1 + p.m2,)
            want = judge.damped_lstsq(p.J, p.b, diag, par)
            D = np.ones_like(want) if diag is None else diag
            e = [rel_fro(x, want), abs(dx2 - np.sum((D * want) ** 2)) / np.sum((D * want) ** 2), 0.0, 0.0]
            if par == 0.0:
                e[2] = rel_fro(x, x0)
            if parent:
                dm, db = p.damped(qa, diag, par)
                e[3] = rel_fro(x, other.computeAndSolve(dm, db))
            print(f"{form} diag {mode} par {par:g}: x vs lstsq {e[0]:.2e}  |Dx|^2 {e[1]:.2e}  vs factorizeAndSolve {e[2]:.2e}  vs damped computeAndSolve {e[3]:.2e}")
            worst = np.maximum(worst, e)
            np.testing.assert_array_equal(ba.lmSolve(diag, par), x)               # repeatable, without the norm: the same bits
    print(f"worst: x {worst[0]:.2e}  |Dx|^2 {worst[1]:.2e}  par = 0 {worst[2]:.2e}  parent's route {worst[3]:.2e}")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9 and worst[2] <= 1e-9 and worst[3] <= 2e-9
    # W is intact: the factors read the same after any number of damped solves
    np.testing.assert_array_equal(ba.matrixR().toarray(), R_before)
    np.testing.assert_array_equal(ba.computeAndSolve(p.mat(qa, form), p.b), x0)


@pytest.mark.parametrize("name", ["8x(2x1)", "64x(7x2)", "20x(8x6)", "ellipse"])
def test_lm_solve_matches_lstsq(qa, name):
    check_problem(qa, problems()[name]())


def test_sparse_right_block(qa):
    check_problem(qa, gaussian_problem(64, 7, 2, 24, 3, 2), form="csr", parent=False)


def test_device_right_hand_side_and_state(qa):
    import torch
    p = gaussian_problem(64, 7, 2, 24, 3, 2)
    ba = qa.BlockAngularSparseQR()
    ba.computeAndSolve(p.mat(qa), torch.from_numpy(p.b).to("cuda"))
    x = ba.lmSolve(torch.from_numpy(p.norms).to("cuda"), 0.5)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    assert rel_fro(x.cpu().numpy(), judge.damped_lstsq(p.J, p.b, p.norms, 0.5)) <= 1e-9
    # another shape re-sizes the kept arrays; compute() (explicit Q) leaves nothing to damp
    q = gaussian_problem(20, 8, 6, 9, 2, 3)
    ba.computeAndSolve(q.mat(qa), q.b)
    assert rel_fro(ba.lmSolve(None, 2.0), judge.damped_lstsq(q.J, q.b, None, 2.0)) <= 1e-9
    ba.compute(q.mat(qa))
    with pytest.raises(RuntimeError, match="lmSolve"):
        ba.lmSolve(None, 1.0)
    ba.computeAndSolve(q.mat(qa), q.b)
    with pytest.raises(ValueError):
        ba.lmSolve(None, -1.0)


# ---- the LM loop ------------------------------------------------------------------------------------------------------------------------------

def kept_factor_lm(qa, start, pts):
    """ellipse_lm of tests/test_angular_qless_gpu.py (accept a step that lowers the cost: lambda / 10, else lambda x 10; at most 60
    trial steps; stop below 1e-24) with one computeAndSolve of the UNDAMPED Jacobian per accepted iterate; every trial lambda goes
    through lmSolve(None, lambda).  Returns (uv, cost, factorisations, trials)."""
    rows, cols = np.full(NPTS, 2, np.int32), np.full(NPTS, 1, np.int32)
    ba = qa.BlockAngularSparseQR()
    uv, lam = start.copy(), 1e-2
    cost = 0.5 * np.sum((pts - ellipse_model(uv)) ** 2)
    factorisations = trials = 0
    fresh = False
    for it in range(60):
        if not fresh:
            tiles, J2, rhs = ellipse_jacobian(uv, pts)
            ba.computeAndSolve(qa.BlockMatrix1x2(qa.SparseBlockDiagonal.fromTiles(rows, cols, tiles), J2), rhs)
            factorisations, fresh = factorisations + 1, True
        dx = ba.lmSolve(None, lam)
        trials += 1
        trial = uv + dx
        new_cost = 0.5 * np.sum((pts - ellipse_model(trial)) ** 2)
        if new_cost < cost:
            uv, cost, lam, fresh = trial, new_cost, lam * 0.1, False
        else:
            lam *= 10.0
        if cost < 1e-24:
            break
    return uv, cost, factorisations, trials


@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_lm_loop_ellipse_fitting_on_kept_factors(qa, scale):
    """The loop from ellipse_data()'s start (scale 1) and from a start eight times as far from the generating parameters.

    From ellipse_data()'s own start no trial is ever rejected (numpy.linalg.lstsq in place of the solver: 5 trial steps, 5
    accepted), so that run has no rejected lambda to save a factorisation on and can only show factorisations <= trials.  A kept
    factorisation pays when a trial is REJECTED; the same loop with lstsq from the start scaled by 8 rejects 3 of 13 trials
    (10 factorisations) and still converges, so that start carries the assertion `factorisations < trials`.  Both starts reach
    cost < 1e-20 and the generating parameters within 1e-8, as test_lm_loop_ellipse_fitting does."""
    truth, pts, start = ellipse_data()
    uv, cost, factorisations, trials = kept_factor_lm(qa, truth + scale * (start - truth), pts)
    print(f"kept-factor loop, start x {scale:g}: cost {cost:.2e}, {factorisations} factorisations for {trials} trial steps")
    assert cost < 1e-20
    assert np.max(np.abs(uv[NPTS:] - truth[NPTS:])) < 1e-8
    assert factorisations <= trials
    if scale > 1.0:
        assert factorisations < trials
