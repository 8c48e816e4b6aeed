"""GPU: one Levenberg-Marquardt step of the block-angular composition without Q1 (BlockAngularSparseQR.computeAndSolve over
qrk_bd_factorize_apply_qt) against the CPU oracle and against the explicit route, compute() + solve().

Tolerances are those of tests/test_angular.py for the same quantities: column permutation bit-exact, matrixR() and Q^T b within 1e-12
rel_fro, x within 1e-9.  The two routes answer to the oracle within those, so to each other within twice that.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import rel_fro
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


# ---- problems --------------------------------------------------------------------------------------------------------------------

def angular_problem(num_vars, m2, seed=1, n2=0, r=7, c=2):
    """generate_block_angular_matrix shape (test/test-qrkit.cpp:135-165) with non-overlapping r x c blocks: J1 = num_vars blocks,
    J2 = dense (r num_vars + n2) x m2, all U(0.5, 5) from the reference's generator (tests/test_angular.py)."""
    vals = orc.gen_uniform(seed, 0.5, 5.0, num_vars * r * c + (r * num_vars + n2) * m2)
    tiles = vals[:num_vars * r * c]
    J2 = vals[num_vars * r * c:].reshape(r * num_vars + n2, m2)
    prob = orc.BDProblem.uniform(num_vars, r, c, tiles)
    J1 = sp.block_diag([tiles[i * r * c:(i + 1) * r * c].reshape(c, r).T for i in range(num_vars)], format="csc")
    if n2:
        J1 = sp.vstack([J1, sp.csc_matrix((n2, c * num_vars))], format="csc")
    return prob, tiles, J1, J2


def assert_clear_pivots(res, rel=1e-9):
    """Every pivot step of the right block has a clear winner: the largest remaining column norm (the chosen column's, |R2(k, k)|)
    exceeds the runner-up's by more than `rel`.  The device decides the order on values that differ from the oracle's in the last
    bits, so the bit-exact comparison of the permutation only means something where this holds.  On the oracle's result alone."""
    m2 = res.m2
    R2 = np.triu(res.qr2[:m2, :])
    rem = np.sqrt(np.cumsum((R2 ** 2)[::-1], axis=0)[::-1])      # rem[k, j] = |R2(k:, j)|: column j's remaining norm at step k
    for k in range(m2 - 1):
        win, runner = rem[k, k], rem[k, k + 1:].max()
        assert win > runner * (1.0 + rel), f"pivot step {k}: winner {win!r} against runner-up {runner!r}: choose another seed"


# (num_vars, m2, n2, block rows, block cols): the shapes of tests/test_angular.py and the ellipse shape (2 x 1 blocks, m2 = 5)
CASES = [(64, 24, 0, 7, 2), (100, 30, 17, 7, 2), (1024, 384, 0, 7, 2), (300, 5, 0, 2, 1)]


@functools.lru_cache(maxsize=None)
def case(num_vars, m2, n2, r, c):
    prob, tiles, J1, J2 = angular_problem(num_vars, m2, n2=n2, r=r, c=c)
    ref = orc.ba_factorize(prob, J2)
    J = sp.hstack([J1, sp.csc_matrix(J2)], format="csc")
    x = np.random.default_rng(0).uniform(-1, 1, J.shape[1])
    b = J @ x
    return prob, tiles, J2, ref, x, b, orc.ba_apply_qt(ref, b)


def right_block(J2, form):
    return J2 if form == "dense" else (sp.csr_matrix(J2) if form == "csr" else sp.csc_matrix(J2))


# ---- oracle parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "csr", "csc"])
@pytest.mark.parametrize("num_vars,m2,n2,r,c", CASES)
def test_compute_and_solve_matches_oracle(qa, num_vars, m2, n2, r, c, form):
    prob, tiles, J2, ref, x, b, qtb_ref = case(num_vars, m2, n2, r, c)
    assert_clear_pivots(ref)
    left = qa.SparseBlockDiagonal.fromTiles(prob.rows, prob.cols, tiles)
    ba = qa.BlockAngularSparseQR()
    got_x, got_qtb = ba.computeAndSolve(qa.BlockMatrix1x2(left, right_block(J2, form)), b, returnQtB=True)
    assert "bdqr_thin_panel_kernel" in ba.m_leftSolver.panelKernelName(m2 + 1)
    assert ba.info() == 0 and ba.rank() == ref.rank
    np.testing.assert_array_equal(ba.colsPermutation(), ref.perm)                   # bit-exact
    np.testing.assert_array_equal(ba.rowsPermutation(), np.arange(J2.shape[0]))
    e_r, e_q = rel_fro(ba.matrixR().toarray(), ref.R.toarray()), rel_fro(got_qtb, qtb_ref)
    x_ref = orc_solve(ref, qtb_ref)
    e_x, e_gen = rel_fro(got_x, x_ref), rel_fro(got_x, x)
    print(f"R {e_r:.2e}  Q^T b {e_q:.2e}  x vs oracle {e_x:.2e}  x vs generating vector {e_gen:.2e}")
    assert e_r <= 1e-12 and e_q <= 1e-12
    assert e_x <= 1e-9 and e_gen <= 1e-9


def orc_solve(ref, qtb):
    """_solve_impl (BlockAngularSparseQR.h:202-227) on the oracle's factors: x = P R(0:n, 0:n)^-1 (Q^T b)(0:n)"""
    import scipy.sparse.linalg as spl
    n = ref.m1 + ref.m2
    z = spl.spsolve_triangular(ref.R[:n, :n].tocsr(), qtb[:n], lower=False)
    x = np.zeros(n); x[ref.perm] = z
    return x


# ---- agreement with the explicit route --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_vars,m2,n2,r,c", CASES)
def test_agrees_with_compute_and_solve(qa, num_vars, m2, n2, r, c):
    prob, tiles, J2, ref, x, b, _ = case(num_vars, m2, n2, r, c)
    left = qa.SparseBlockDiagonal.fromTiles(prob.rows, prob.cols, tiles)
    mat = qa.BlockMatrix1x2(left, J2)
    fused, explicit = qa.BlockAngularSparseQR(), qa.BlockAngularSparseQR()
    xf = fused.computeAndSolve(mat, b)
    explicit.compute(mat)
    xe = explicit.solve(b)
    np.testing.assert_array_equal(fused.colsPermutation(), explicit.colsPermutation())
    e_r, e_x = rel_fro(fused.matrixR().toarray(), explicit.matrixR().toarray()), rel_fro(xf, xe)
    print(f"R fused vs explicit {e_r:.2e}  x {e_x:.2e}")
    assert e_r <= 2e-12 and e_x <= 2e-9
    assert fused.rank() == explicit.rank()


# ---- state ------------------------------------------------------------------------------------------------------------------------

def test_state_after_compute_and_solve(qa):
    import torch
    prob, tiles, J2, ref, x, b, qtb_ref = case(100, 30, 17, 7, 2)
    left = qa.SparseBlockDiagonal.fromTiles(prob.rows, prob.cols, tiles)
    mat = qa.BlockMatrix1x2(left, J2)
    ba = qa.BlockAngularSparseQR()
    x1 = ba.computeAndSolve(mat, b)
    for call in (ba.matrixQ, lambda: ba.applyQ(b), lambda: ba.applyQt(b), lambda: ba.solve(b)):
        with pytest.raises(RuntimeError, match="factorised without Q"):
            call()
    assert ba.rank() == ref.rank and ba.info() == 0 and ba.rows() == J2.shape[0] and ba.cols() == ref.m1 + ref.m2
    # a device right-hand side gives a device x; two identical calls give the same bits
    x2 = ba.factorizeAndSolve(mat, torch.from_numpy(b).to("cuda"))
    assert isinstance(x2, torch.Tensor) and x2.is_cuda
    np.testing.assert_array_equal(x2.cpu().numpy(), x1)
    # a second computeAndSolve with another shape re-sizes W
    prob2, tiles2, J22, ref2, xx2, b2, _ = case(64, 24, 0, 7, 2)
    left2 = qa.SparseBlockDiagonal.fromTiles(prob2.rows, prob2.cols, tiles2)
    x3 = ba.computeAndSolve(qa.BlockMatrix1x2(left2, J22), b2)
    assert tuple(ba._W.shape) == (J22.shape[0], 25)
    np.testing.assert_array_equal(ba.colsPermutation(), ref2.perm)
    assert rel_fro(x3, xx2) <= 1e-9 and rel_fro(ba.matrixR().toarray(), ref2.R.toarray()) <= 1e-12
    # compute() restores the explicit-Q behaviour
    ba.compute(mat)
    assert rel_fro(ba.applyQt(b), qtb_ref) <= 1e-12 and rel_fro(ba.solve(b), x) <= 1e-9
    assert rel_fro(ba.matrixQ().transpose() @ b, qtb_ref) <= 1e-12


def test_smallest_problem(qa):
    """Three 2 x 1 blocks next to two dense columns: one partial workgroup, a panel of three columns, 3 bottom rows for 2 columns."""
    prob, tiles, J1, J2 = angular_problem(3, 2, seed=3, r=2, c=1)
    ref = orc.ba_factorize(prob, J2)
    assert_clear_pivots(ref)
    left = qa.SparseBlockDiagonal.fromTiles(prob.rows, prob.cols, tiles)
    b = np.random.default_rng(2).uniform(-1, 1, 6)
    ba = qa.BlockAngularSparseQR()
    x, qtb = ba.computeAndSolve(qa.BlockMatrix1x2(left, J2), b, returnQtB=True)
    np.testing.assert_array_equal(ba.colsPermutation(), ref.perm)
    qtb_ref = orc.ba_apply_qt(ref, b)
    assert rel_fro(ba.matrixR().toarray(), ref.R.toarray()) <= 1e-12 and rel_fro(qtb, qtb_ref) <= 1e-12
    assert rel_fro(x, orc_solve(ref, qtb_ref)) <= 1e-9


# ---- the LM loop of examples/ellipse_fitting.cpp -------------------------------------------------------------------------------

NPTS = 300


def ellipse_model(uv):
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    return np.stack([a * np.cos(t) * np.cos(r) - b * np.sin(t) * np.sin(r) + x0,
                     a * np.cos(t) * np.sin(r) + b * np.sin(t) * np.cos(r) + y0])


def ellipse_system(uv, pts, lam):
    """The damped step [J; sqrt(lambda) I] dx = [-f; 0] of EllipseFitting (examples/ellipse_fitting.cpp:46-96) in block-angular form.
    The Jacobian's left block is one 2 x 1 block per point (d f_i / d t_i) and its right block has the 5 ellipse parameters.  Damped as
    tests/test_lm_gpu.py damps its blocks (rowpermADiagLambda, test/test-utils.cpp:145-180): the sqrt(lambda) row of a point's own
    unknown goes right below the point's two rows, so the left blocks handed to the solver are 3 x 1 and stay block diagonal; the five
    damping rows of the shared parameters go below J1.  Returns (tiles, J2, rhs)."""
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    f = (pts - ellipse_model(uv)).T                                # (NPTS, 2): fvec(2 i), fvec(2 i + 1)
    ct, st, cr, sr = np.cos(t), np.sin(t), np.cos(r), np.sin(r)
    sl = np.sqrt(lam)
    tiles = np.zeros((NPTS, 1, 3))
    tiles[:, 0, 0] = a * cr * st + b * sr * ct
    tiles[:, 0, 1] = a * sr * st - b * cr * ct
    tiles[:, 0, 2] = sl
    J2 = np.zeros((NPTS, 3, 5))
    J2[:, 0, :] = np.stack([-ct * cr, st * sr, -np.ones(NPTS), np.zeros(NPTS), a * ct * sr + b * st * cr], axis=1)
    J2[:, 1, :] = np.stack([-ct * sr, -st * cr, np.zeros(NPTS), -np.ones(NPTS), -a * ct * cr + b * st * sr], axis=1)
    J2 = np.vstack([J2.reshape(3 * NPTS, 5), sl * np.eye(5)])
    rhs = np.zeros((NPTS, 3)); rhs[:, :2] = -f
    return tiles.ravel(), J2, np.concatenate([rhs.ravel(), np.zeros(5)])


def ellipse_lm(step, uv0, pts, on_step=None):
    """Levenberg-Marquardt as tests/test_lm_gpu.py runs it: accept a step that lowers the cost (lambda / 10), else lambda x 10."""
    uv, lam = uv0.copy(), 1e-2
    cost = 0.5 * np.sum((pts - ellipse_model(uv)) ** 2)
    for it in range(60):
        tiles, J2, rhs = ellipse_system(uv, pts, lam)
        dx = step(tiles, J2, rhs)
        if on_step is not None:
            on_step(tiles, J2, rhs, dx)
        trial = uv + np.concatenate([dx[:NPTS], dx[NPTS:]])
        new_cost = 0.5 * np.sum((pts - ellipse_model(trial)) ** 2)
        if new_cost < cost:
            uv, cost, lam = trial, new_cost, lam * 0.1
        else:
            lam *= 10.0
        if cost < 1e-24:
            break
    return uv, cost


def ellipse_data():
    rng = np.random.default_rng(11)
    truth = np.concatenate([np.sort(rng.uniform(0.0, 2.0 * np.pi, NPTS)), [3.0, 2.0, 0.5, -0.3, 0.4]])
    pts = ellipse_model(truth)                                     # noise-free
    start = truth + np.concatenate([0.05 * rng.standard_normal(NPTS), [0.3, -0.2, 0.1, 0.1, -0.1]])
    return truth, pts, start


def test_lm_loop_ellipse_fitting(qa):
    truth, pts, start = ellipse_data()
    rows, cols = np.full(NPTS, 3, np.int32), np.full(NPTS, 1, np.int32)
    fused, explicit = qa.BlockAngularSparseQR(), qa.BlockAngularSparseQR()
    worst = [0.0]

    def fused_step(tiles, J2, rhs):
        return fused.computeAndSolve(qa.BlockMatrix1x2(qa.SparseBlockDiagonal.fromTiles(rows, cols, tiles), J2), rhs)

    def explicit_step(tiles, J2, rhs):
        explicit.compute(qa.BlockMatrix1x2(qa.SparseBlockDiagonal.fromTiles(rows, cols, tiles), J2))
        return explicit.solve(rhs)

    def compare(tiles, J2, rhs, dx):
        worst[0] = max(worst[0], rel_fro(dx, explicit_step(tiles, J2, rhs)))       # the same Jacobian through the other route

    uv_f, cost_f = ellipse_lm(fused_step, start, pts, on_step=compare)
    assert "bdqr_thin_panel_kernel" in fused.m_leftSolver.panelKernelName(6)
    print(f"fused loop: cost {cost_f:.2e}, worst step difference {worst[0]:.2e}")
    assert worst[0] <= 1e-9
    uv_e, cost_e = ellipse_lm(explicit_step, start, pts)
    assert cost_f < 1e-20 and cost_e < 1e-20
    # both loops end at the same parameters, the generating ones (the model is 2 pi periodic in t and the data noise-free)
    assert np.max(np.abs(uv_f[NPTS:] - uv_e[NPTS:])) < 1e-8 and np.max(np.abs(uv_f[NPTS:] - truth[NPTS:])) < 1e-8
    assert np.max(np.abs(uv_f[:NPTS] - uv_e[:NPTS])) < 1e-8
