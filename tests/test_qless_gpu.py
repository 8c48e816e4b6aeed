"""GPU: factorise-and-solve without Q (qrk_bd_factorize_rhs; BlockDiagonalSparseQR.factorizeAndSolve) against the CPU oracle.

The oracle is the judge: permutation bit-exact; R, tau and Q^T b within RTOL = 1e-12 PER TILE (Q^T b expected from the oracle's Q
values arranged by the oracle's pattern); x against the oracle's solve at the tolerances of the explicit route (thin shapes on
seeded_tiles(., 0.5, 5.0): 1e-11 as test_lm_gpu.py; 32 x 32 on seeded_tiles(3, -1, 1): 1e-9 as test_bd_gpu.py).  Plans without a
Q-less kernel run the explicit kernels through a scratch: their results are bitwise those of compute() + applyQt() / solve().
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import RTOL, oracle_factorize, per_tile_rel, rel_fro, seeded_tiles, tile_sizes

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


# ---- the expected values -------------------------------------------------------------------------------------------------------

class Ref:
    """Oracle factorisation of one batch, its Q as a sparse matrix, and where every tile's entries of Q^T b sit."""

    def __init__(self, rows, cols, tiles, mat_rows, q_format, solver):
        self.rows, self.cols, self.tiles = np.asarray(rows, np.int32), np.asarray(cols, np.int32), tiles
        self.mat_rows, self.mat_cols, self.sum_rows = int(mat_rows), int(self.cols.sum()), int(self.rows.sum())
        self.q_format, self.solver = q_format, solver
        self.prob, self.ref = oracle_factorize(self.rows, self.cols, tiles, mat_rows=mat_rows, q_format=q_format, block_solver=solver)
        qp, qi, _, _ = self.prob.pattern()
        self.Q = sp.csr_matrix((self.ref.Q_vals, qi, qp), shape=(self.mat_rows, self.mat_rows))
        # positions of Q^T b, tile by tile (bd_aux.hip / BlockDiagonalSparseQR.h:455-492): FullQ [U.. | N..], BlockDiagonalQ by rows
        idx = []
        br = bc = 0
        for r, c in zip(self.rows.tolist(), self.cols.tolist()):
            k = np.arange(r)
            idx.append(np.where(k < c, bc + k, self.mat_cols + (br - bc) + (k - c)) if q_format == FULL_Q else br + k)
            br += r; bc += c
        self.qtb_idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)

    def qtb(self, b):
        return self.Q.T @ b.reshape(self.mat_rows, -1)

    def x(self, b):
        return self.prob.solve(self.ref, b.reshape(self.mat_rows, -1))


@functools.lru_cache(maxsize=None)
def uniform_ref(B, r, c, lo, hi, seed, extra, q_format, solver):
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    return Ref(rows, cols, seeded_tiles(seed, lo, hi, B * r * c), B * r + extra, q_format, solver)


def rhs_for(ref, nrhs, seed=0):
    return np.random.default_rng(100 + seed + ref.mat_rows).uniform(-1.0, 1.0, (ref.mat_rows, nrhs))


def solver_for(qa, ctx, ref, hc=True):
    mat = qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, ref.tiles, rows=ref.mat_rows)
    return mat, qa.BlockDiagonalSparseQR(blockSolver=ref.solver, qFormat=ref.q_format, context=ctx, hCoeffs=hc)


def check_factors(qr, ref, hc=True, tol=RTOL):
    """perm bit-exact; R and tau within tol per tile"""
    assert qr.info() == ref.ref.info and qr.rank() == ref.ref.rank
    np.testing.assert_array_equal(qr.colsPermutation(), ref.ref.perm)
    _, sr, sc = tile_sizes(ref.rows, ref.cols)
    e_r = per_tile_rel(qr.rValues().cpu().numpy(), ref.ref.R_vals, sr)
    e_t = per_tile_rel(qr.hCoeffs().cpu().numpy(), ref.ref.hcoeffs, sc) if hc else 0.0
    print(f"R per tile {e_r:.2e}, tau per tile {e_t:.2e}")
    assert e_r <= tol and e_t <= tol


def check_qtb(got, ref, b, tol=RTOL):
    got, want, b = (np.asarray(a).reshape(ref.mat_rows, -1) for a in (got, ref.qtb(b), b))
    worst = max(per_tile_rel(got[ref.qtb_idx, j], want[ref.qtb_idx, j], ref.rows) for j in range(got.shape[1]))
    print(f"Q^T b per tile {worst:.2e}")
    assert worst <= tol
    np.testing.assert_array_equal(got[ref.sum_rows:], b[ref.sum_rows:])      # trailing identity rows of Q copy b


def check_x(got, ref, b, tol):
    err = rel_fro(np.asarray(got).reshape(ref.mat_cols, -1), ref.x(b))
    print(f"x {err:.2e}")
    assert err <= tol


def run_all_outputs(qa, ctx, ref, nrhs, xtol, kernel):
    """Every combination a caller can ask for on one batch: x and Q^T b / x only / Q^T b only with tau, both without tau."""
    b = rhs_for(ref, nrhs)
    bb = b if nrhs > 1 else b[:, 0]
    if ref.q_format == FULL_Q:
        modes = ((True, True, True), (True, True, False), (True, False, True), (False, True, True))
    else:       # R is upper triangular only in the FullQ format: a BlockDiagonalQ solver gives Q^T b alone, as with solve()
        modes = ((True, False, True), (False, False, True))
    for hc, want_x, want_qtb in modes:
        mat, qr = solver_for(qa, ctx, ref, hc)
        out = qr.computeAndSolve(mat, bb, returnQtB=want_qtb, solve=want_x)
        assert kernel in qr.rhsKernelName(nrhs), qr.rhsKernelName(nrhs)
        x, y = out if (want_x and want_qtb) else ((out, None) if want_x else (None, out))
        check_factors(qr, ref, hc)
        if want_qtb:
            assert y.shape == bb.shape
            check_qtb(y, ref, b)
        if want_x:
            assert x.shape == ((ref.mat_cols, nrhs) if nrhs > 1 else (ref.mat_cols,))
            check_x(x, ref, b, xtol)


# ---- thin tiles: bdqr_thin_rhs.hip ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c", [(7, 2), (9, 2), (2, 1), (5, 1), (2, 2), (16, 2)])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])       # the 256-tile workgroup edge and a second sweep
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("solver", [0, 1])
def test_thin_tiles_match_oracle(qa, ctx, r, c, B, nrhs, solver):
    """mat_rows = sum of rows + 5: five trailing identity rows pass b through; both Q formats (the layout of Q^T b)."""
    for qf in (FULL_Q, BLOCK_DIAGONAL_Q):
        run_all_outputs(qa, ctx, uniform_ref(B, r, c, 0.5, 5.0, 1 + r + c, 5, qf, solver), nrhs, 1e-11, "bdqr_thin_rhs_kernel")


def test_thin_tiles_without_trailing_rows(qa, ctx):
    for (r, c) in ((7, 2), (5, 1)):
        run_all_outputs(qa, ctx, uniform_ref(300, r, c, 0.5, 5.0, 4, 0, FULL_Q, 0), 2, 1e-11, "bdqr_thin_rhs_kernel")


# ---- 32 x 32: the right-hand-side form of bdqr_pair4.hip --------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2, 3, 301])                # odd count = missing partner
@pytest.mark.parametrize("nrhs", [1, 2, 32])
@pytest.mark.parametrize("solver", [0, 1])
def test_32x32_tiles_match_oracle(qa, ctx, B, nrhs, solver):
    run_all_outputs(qa, ctx, uniform_ref(B, 32, 32, -1.0, 1.0, 3, 0, FULL_Q, solver), nrhs, 1e-9, "bdqr_pair4_rhs_kernel")


@pytest.mark.parametrize("qf", [FULL_Q, BLOCK_DIAGONAL_Q])
def test_32x32_trailing_rows_and_q_formats(qa, ctx, qf):
    """An odd mat_rows: the right-hand sides past the first are only 8-byte aligned, and five identity rows copy b."""
    run_all_outputs(qa, ctx, uniform_ref(5, 32, 32, -1.0, 1.0, 3, 5, qf, 0), 3, 1e-9, "bdqr_pair4_rhs_kernel")


# ---- plans without a Q-less kernel: the explicit kernels through the plan's scratch ---------------------------------------------

def check_fallback(qa, ctx, ref, nrhs, mat=None):
    b = rhs_for(ref, nrhs)
    mat0, qr = solver_for(qa, ctx, ref)
    mat = mat or mat0
    qr.analyzePattern(mat)
    assert "fallback" in qr.rhsKernelName(nrhs) or mat is not mat0
    x, y = qr.factorizeAndSolve(mat, b, returnQtB=True)
    check_factors(qr, ref)
    check_qtb(y, ref, b)
    r1, p1, t1 = qr.rValues().clone(), qr.colsPermutation().copy(), qr.hCoeffs().clone()
    qr.compute(mat)
    import torch
    assert torch.equal(qr.rValues(), r1) and torch.equal(qr.hCoeffs(), t1)
    np.testing.assert_array_equal(qr.colsPermutation(), p1)
    np.testing.assert_array_equal(y, qr.applyQt(b))          # the same kernels on the same Q: the same bits
    np.testing.assert_array_equal(x, qr.solve(b))


@pytest.mark.parametrize("B,r,c", [(300, 8, 6), (65, 32, 20), (8, 64, 64)])
def test_fallback_shapes_match_oracle_and_the_explicit_route(qa, ctx, B, r, c):
    check_fallback(qa, ctx, uniform_ref(B, r, c, -1.0, 1.0, 7, 0, FULL_Q, 0), 2)


def test_fallback_mixed_batch(qa, ctx):
    rng = np.random.default_rng(7)                           # the 400-tile mixed batch of test_bd_gpu.py
    B = 400
    cols = rng.integers(1, 33, B).astype(np.int32)
    rows = (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32)
    tiles = seeded_tiles(11, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    check_fallback(qa, ctx, Ref(rows, cols, tiles, int(rows.sum()) + 5, FULL_Q, 0), 2)


def test_fallback_beyond_the_fast_paths(qa, ctx):
    """33 right-hand sides on 32 x 32, 5 on 7 x 2 (more than the kernels carry), and a tiles array that is only 8-byte aligned."""
    import torch
    ref = uniform_ref(3, 32, 32, -1.0, 1.0, 3, 0, FULL_Q, 0)
    check_fallback(qa, ctx, ref, 33)
    check_fallback(qa, ctx, uniform_ref(300, 7, 2, 0.5, 5.0, 10, 5, FULL_Q, 0), 5)
    buf = torch.empty(ref.tiles.size + 1, dtype=torch.float64, device=ctx.device)
    buf[1:] = torch.from_numpy(ref.tiles).to(ctx.device)
    view = buf[1:]
    assert view.data_ptr() % 16 == 8
    mat = qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, view)
    assert mat.tiles_dev.data_ptr() == view.data_ptr()
    check_fallback(qa, ctx, ref, 1, mat=mat)
    x = qa.BlockDiagonalSparseQR(context=ctx).computeAndSolve(mat, rhs_for(ref, 1)[:, 0])
    check_x(x, ref, rhs_for(ref, 1), 1e-9)


# ---- ties: every tile flagged and redone in Eigen's operation order ---------------------------------------------------------------

def tie_tiles(kind, B, r, c, seed):
    rng = np.random.default_rng(seed)
    if kind == "pm1":                # every column has the same norm: the first pivot is a tie
        t = rng.choice([-1.0, 1.0], (B, c, r))
    else:                            # a duplicated column: the two tie whenever either is the largest
        t = rng.uniform(-1.0, 1.0, (B, c, r))
        t[:, c - 1, :] = t[:, c // 3, :]
    return t.reshape(-1)             # (tile, column, row) = column-major tiles back to back


@pytest.mark.parametrize("kind", ["pm1", "dup"])
@pytest.mark.parametrize("r,c,kernel", [(7, 2, "bdqr_thin_rhs_kernel"), (32, 32, "bdqr_pair4_rhs_kernel")])
def test_tie_tiles_are_redone_exactly(qa, ctx, kind, r, c, kernel):
    """R may be singular here: the permutation, R, tau and Q^T b are compared (x is whatever the division gives)."""
    B = 300
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    ref = Ref(rows, cols, tie_tiles(kind, B, r, c, 5), B * r, FULL_Q, 0)
    b = rhs_for(ref, 2)
    mat, qr = solver_for(qa, ctx, ref)
    _, y = qr.computeAndSolve(mat, b, returnQtB=True)
    assert kernel in qr.rhsKernelName(2)
    check_factors(qr, ref)
    check_qtb(y, ref, b)
    # ... and a clean batch right behind it on the same plan: the redo list was consumed and reset
    ref2 = uniform_ref(B, r, c, 0.5, 5.0, 9, 0, FULL_Q, 0)
    b2 = rhs_for(ref2, 2, seed=1)
    x2, y2 = qr.factorizeAndSolve(qa.SparseBlockDiagonal.fromTiles(rows, cols, ref2.tiles), b2, returnQtB=True)
    check_factors(qr, ref2)
    check_qtb(y2, ref2, b2)


# ---- dispatch, state, the LM loop -----------------------------------------------------------------------------------------------

def test_dispatch_names_the_kernels(qa, ctx):
    """Without this a build that always takes the fallback would pass everything else."""
    def name(B, r, c, nrhs):
        rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
        qr = qa.BlockDiagonalSparseQR(context=ctx)
        qr.analyzePattern(qa.SparseBlockDiagonal.fromTiles(rows, cols, np.zeros(B * r * c)))
        return qr.rhsKernelName(nrhs)
    assert "bdqr_thin_rhs_kernel" in name(10, 7, 2, 1)
    assert "bdqr_thin_rhs_kernel" in name(10, 9, 2, 1)
    assert "bdqr_pair4_rhs_kernel" in name(10, 32, 32, 1)
    assert "bdqr_pair4_rhs_kernel" in name(10, 32, 32, 32)
    assert "fallback" in name(10, 8, 6, 1)
    assert "fallback" in name(10, 32, 32, 33)
    assert "fallback" in name(10, 7, 2, 64)
    assert "fallback" in name(10, 64, 64, 1)


def test_state_after_factorize_and_solve(qa, ctx):
    import torch
    ref = uniform_ref(300, 7, 2, 0.5, 5.0, 10, 0, FULL_Q, 0)
    b = rhs_for(ref, 1)[:, 0]
    mat, qr = solver_for(qa, ctx, ref)
    x1, y1 = qr.computeAndSolve(mat, b, returnQtB=True)
    for call in (qr.qValues, qr.matrixQ, lambda: qr.solve(b), lambda: qr.applyQt(b), lambda: qr.applyQ(b)):
        with pytest.raises(RuntimeError, match="factorised without Q"):
            call()
    # what needs no Q works
    assert qr.rank() == ref.ref.rank and qr.info() == 0
    assert rel_fro(qr.matrixR().data, ref.ref.R_vals) <= RTOL
    z = qr.solveR(y1[:ref.mat_cols])
    back = np.zeros_like(z); back[qr.colsPermutation()] = z
    assert rel_fro(back, x1) <= 1e-13
    r1, p1 = qr.rValues().clone(), qr.colsPermutation().copy()
    # two identical calls: bitwise identical outputs
    x2, y2 = qr.factorizeAndSolve(mat, b, returnQtB=True)
    np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(y1, y2)
    assert torch.equal(qr.rValues(), r1)
    np.testing.assert_array_equal(qr.colsPermutation(), p1)
    # compute() restores the explicit-Q behaviour
    qr.compute(mat)
    assert rel_fro(qr.qValues().cpu().numpy(), ref.ref.Q_vals) <= RTOL
    # (both routes answer to the oracle within 1e-11 for x and 1e-12 for Q^T b: to each other within twice that)
    assert rel_fro(qr.solve(b), x1) <= 2e-11 and rel_fro(qr.applyQt(b), y1) <= 2e-12
    # ... and on 32 x 32
    ref = uniform_ref(33, 32, 32, -1.0, 1.0, 3, 0, FULL_Q, 0)
    b = rhs_for(ref, 2)
    mat, qr = solver_for(qa, ctx, ref)
    o1 = qr.computeAndSolve(mat, b, returnQtB=True)
    o2 = qr.factorizeAndSolve(mat, b, returnQtB=True)
    np.testing.assert_array_equal(o1[0], o2[0])
    np.testing.assert_array_equal(o1[1], o2[1])
    with pytest.raises(RuntimeError, match="factorised without Q"):
        qr.solve(b)


def test_argument_checks_and_landscape(qa, ctx):
    import ctypes as C
    import torch
    from qrkit_amd import _capi as capi
    ref = uniform_ref(10, 7, 2, 0.5, 5.0, 10, 0, BLOCK_DIAGONAL_Q, 0)
    mat, qr = solver_for(qa, ctx, ref)
    qr.analyzePattern(mat)
    lib, dev = capi.lib(), ctx.device
    t = mat.device_tiles(dev)
    b = torch.zeros(ref.mat_rows + 1, dtype=torch.float64, device=dev)                    # one more: the shifted qtb below stays inside b
    y, x = torch.zeros_like(b), torch.zeros(ref.mat_cols, dtype=torch.float64, device=dev)
    r = torch.zeros(30, dtype=torch.float64, device=dev)
    p = torch.zeros(ref.mat_cols, dtype=torch.int32, device=dev)
    call = lambda bb, yy, xx: lib.qrk_bd_factorize_rhs(qr._plan, t.data_ptr(), bb, 1, r.data_ptr(), p.data_ptr(), None, yy, xx, capi.MEM_DEVICE)
    assert call(b.data_ptr(), None, None) == capi.STATUS_INVALID_ARGUMENT                 # nothing asked for
    assert call(b.data_ptr(), b.data_ptr(), None) == capi.STATUS_INVALID_ARGUMENT         # b overlaps qtb
    assert call(b.data_ptr(), b.data_ptr() + 8, None) == capi.STATUS_INVALID_ARGUMENT
    assert call(b.data_ptr(), y.data_ptr(), x.data_ptr()) == capi.STATUS_UNSUPPORTED      # x on a BlockDiagonalQ plan: as qrk_bd_solve
    assert call(b.data_ptr(), y.data_ptr(), None) == capi.STATUS_OK
    with pytest.raises(capi.QrkError):
        qr.factorizeAndSolve(mat, np.zeros(ref.mat_rows))
    # a landscape tile: InvalidInput, as after factorize()
    rows, cols = np.array([4, 3], np.int32), np.array([2, 5], np.int32)
    lm = qa.SparseBlockDiagonal.fromTiles(rows, cols, seeded_tiles(1, -1, 1, 4 * 2 + 3 * 5))
    q2 = qa.BlockDiagonalSparseQR(context=ctx)
    assert q2.computeAndSolve(lm, np.zeros(7)) is None
    assert q2.info() == qa.INFO_INVALID_INPUT and not q2.m_isInitialized


def test_host_memory_space(qa, ctx):
    """QRK_MEM_HOST stages like qrk_bd_factorize: host arrays in, host arrays out."""
    import ctypes as C
    from qrkit_amd import _capi as capi
    ref = uniform_ref(300, 9, 2, 0.5, 5.0, 12, 5, FULL_Q, 0)
    mat, qr = solver_for(qa, ctx, ref)
    qr.analyzePattern(mat)
    b = np.asfortranarray(rhs_for(ref, 2))
    r = np.zeros(ref.ref.R_vals.size); p = np.zeros(ref.mat_cols, np.int32); hc = np.zeros(ref.mat_cols)
    y = np.zeros_like(b, order="F"); x = np.zeros((ref.mat_cols, 2), order="F")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(capi.lib().qrk_bd_factorize_rhs(qr._plan, ptr(ref.tiles), ptr(b), 2, ptr(r), ptr(p), ptr(hc), ptr(y), ptr(x), capi.MEM_HOST),
               ctx.handle)
    np.testing.assert_array_equal(p, ref.ref.perm)
    _, sr, sc = tile_sizes(ref.rows, ref.cols)
    assert per_tile_rel(r, ref.ref.R_vals, sr) <= RTOL and per_tile_rel(hc, ref.ref.hcoeffs, sc) <= RTOL
    check_qtb(y, ref, b)
    check_x(x, ref, b, 1e-11)


def test_lm_loop_with_factorize_and_solve(qa):
    """test_lm_gpu.py's curve fits y = exp(a t) + b (7 samples, 2 parameters each, damped to 9x2 blocks) with the Q-less step:
    analyzePattern() once, factorizeAndSolve() per iteration, the plan unchanged."""
    B = 500
    rng = np.random.default_rng(5)
    t = np.linspace(0.0, 1.0, 7)
    a_true, b_true = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    y = np.exp(a_true[:, None] * t) + b_true[:, None]
    qr = qa.BlockDiagonalSparseQR(context=qa.Context(0))
    rows, cols = np.full(B, 9, np.int32), np.full(B, 2, np.int32)
    a, b = np.zeros(B), np.zeros(B)
    lam = 1e-2

    def residual(a, b):
        return np.exp(a[:, None] * t) + b[:, None] - y          # (B, 7)

    cost = 0.5 * np.sum(residual(a, b) ** 2)
    plan_before = None
    for it in range(30):
        r = residual(a, b)
        tiles = np.zeros((B, 2, 9))                               # column-major 9x2 tiles
        tiles[:, 0, :7] = t * np.exp(a[:, None] * t)              # d/da
        tiles[:, 1, :7] = 1.0                                     # d/db
        tiles[:, 0, 7] = np.sqrt(lam)                             # [J_i; sqrt(lambda) I_2]
        tiles[:, 1, 8] = np.sqrt(lam)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, tiles.ravel())
        if plan_before is None:
            qr.analyzePattern(mat)
            plan_before = qr._plan.value
            assert "bdqr_thin_rhs_kernel" in qr.rhsKernelName(1)
        rhs = np.zeros((B, 9)); rhs[:, :7] = -r
        dx = qr.factorizeAndSolve(mat, rhs.ravel()).reshape(B, 2)
        assert qr._plan.value == plan_before                      # the pattern analysis is reused
        new_cost = 0.5 * np.sum(residual(a + dx[:, 0], b + dx[:, 1]) ** 2)
        if new_cost < cost:
            a, b, cost, lam = a + dx[:, 0], b + dx[:, 1], new_cost, lam * 0.1
        else:
            lam *= 10.0
        if cost < 1e-24:
            break
    assert np.max(np.abs(a - a_true)) < 1e-8 and np.max(np.abs(b - b_true)) < 1e-8
