"""GPU: factorize + Q^T of a wide strided panel without Q (qrk_bd_factorize_apply_qt; bdqr_thin_panel.hip) against the CPU oracle,
at the C ABI.

The oracle is the judge, with the tolerances of tests/test_qless_gpu.py: permutation bit-exact; R, tau and Q^T-of-panel within
RTOL = 1e-12 PER TILE (the expected panel is the oracle's Q, arranged by the oracle's pattern, transposed, times the panel).  Plans
without the thin kernel run the explicit kernels through the plan's scratch: their results are bitwise those of compute() + applyQt().
Every thin case runs with five trailing identity rows and odd, different leading dimensions, and the padding rows of the output
must keep a sentinel.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import RTOL, oracle_factorize, per_tile_rel, seeded_tiles, tile_sizes

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1
SENTINEL = 7777.25
KERNEL = "bdqr_thin_panel_kernel"


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


class Ref:
    """Oracle factorisation of one batch, its Q as a sparse matrix, and where every tile's entries of Q^T c sit."""

    def __init__(self, rows, cols, tiles, mat_rows, q_format, solver):
        self.rows, self.cols, self.tiles = np.asarray(rows, np.int32), np.asarray(cols, np.int32), tiles
        self.mat_rows, self.mat_cols, self.sum_rows = int(mat_rows), int(self.cols.sum()), int(self.rows.sum())
        self.q_format, self.solver = q_format, solver
        self.prob, self.ref = oracle_factorize(self.rows, self.cols, tiles, mat_rows=mat_rows, q_format=q_format, block_solver=solver)
        qp, qi, _, _ = self.prob.pattern()
        self.Q = sp.csr_matrix((self.ref.Q_vals, qi, qp), shape=(self.mat_rows, self.mat_rows))
        # positions of Q^T c, tile by tile (BlockDiagonalSparseQR.h:455-492): FullQ [U.. | N..], BlockDiagonalQ by rows
        idx = []
        br = bc = 0
        for r, c in zip(self.rows.tolist(), self.cols.tolist()):
            k = np.arange(r)
            idx.append(np.where(k < c, bc + k, self.mat_cols + (br - bc) + (k - c)) if q_format == FULL_Q else br + k)
            br += r; bc += c
        self.qt_idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def uniform_ref(B, r, c, lo, hi, seed, extra, q_format, solver):
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    return Ref(rows, cols, seeded_tiles(seed, lo, hi, B * r * c), B * r + extra, q_format, solver)


def panel_for(ref, ncols, seed=0):
    return np.random.default_rng(100 + seed + ref.mat_rows + ncols).uniform(-1.0, 1.0, (ref.mat_rows, ncols))


def odd_lds(mat_rows):
    """ldc = mat_rows + 3 and ldq = mat_rows + 5, bumped to the next odd number: columns past the first are 8-byte aligned only"""
    return (mat_rows + 3) | 1, (mat_rows + 5) | 1


class Run:
    """One qrk_bd_factorize_apply_qt call on device buffers with the given leading dimensions."""

    def __init__(self, qa, ctx, ref, panel, ldc, ldq, hc=True, mat=None, qr=None):
        import torch
        from qrkit_amd import _capi as capi
        self.ref, dev = ref, ctx.device
        self.mat = mat or qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, ref.tiles, rows=ref.mat_rows)
        self.qr = qr or qa.BlockDiagonalSparseQR(blockSolver=ref.solver, qFormat=ref.q_format, context=ctx, hCoeffs=hc)
        if qr is None:
            self.qr.analyzePattern(self.mat)
        ncols = panel.shape[1]
        cbuf = np.full((max(ncols, 1), ldc), np.nan)
        cbuf[:ncols, :ref.mat_rows] = panel.T
        self.c = torch.from_numpy(cbuf).to(dev)
        self.out = torch.full((max(ncols, 1), ldq), SENTINEL, dtype=torch.float64, device=dev)
        self.r = torch.zeros(max(ref.ref.R_vals.size, 1), dtype=torch.float64, device=dev)
        self.p = torch.full((max(ref.mat_cols, 1),), -1, dtype=torch.int32, device=dev)
        self.hc = torch.zeros(max(ref.mat_cols, 1), dtype=torch.float64, device=dev) if hc else None
        ctx.use_current_stream()
        t = self.mat.device_tiles(dev)
        self.status = capi.lib().qrk_bd_factorize_apply_qt(self.qr._plan, t.data_ptr(), self.c.data_ptr(), ldc, ncols, self.r.data_ptr(),
                                                           self.p.data_ptr(), self.hc.data_ptr() if hc else None, self.out.data_ptr(), ldq,
                                                           capi.MEM_DEVICE)
        capi.check(self.status, ctx.handle)
        info, rank = C.c_int(), C.c_int64()
        capi.check(capi.lib().qrk_bd_info(self.qr._plan, C.byref(info), C.byref(rank)), ctx.handle)
        self.info, self.rank = info.value, rank.value
        self.got = self.out.cpu().numpy()[:ncols]          # (ncols, ldq)


def check_factors(run, tol=RTOL):
    ref = run.ref
    assert run.info == ref.ref.info and run.rank == ref.ref.rank
    np.testing.assert_array_equal(run.p.cpu().numpy()[:ref.mat_cols], ref.ref.perm)
    _, sr, sc = tile_sizes(ref.rows, ref.cols)
    e_r = per_tile_rel(run.r.cpu().numpy()[:ref.ref.R_vals.size], ref.ref.R_vals, sr)
    e_t = per_tile_rel(run.hc.cpu().numpy()[:ref.mat_cols], ref.ref.hcoeffs, sc) if run.hc is not None else 0.0
    print(f"R per tile {e_r:.2e}, tau per tile {e_t:.2e}")
    assert e_r <= tol and e_t <= tol


def check_panel(run, panel, tol=RTOL):
    """every column within tol per tile, the trailing identity rows copied, the padding rows untouched"""
    ref = run.ref
    ncols = panel.shape[1]
    got = run.got[:, :ref.mat_rows].T
    want = ref.Q.T @ panel
    worst = max((per_tile_rel(got[ref.qt_idx, j], want[ref.qt_idx, j], ref.rows) for j in range(ncols)), default=0.0)
    print(f"Q^T c per tile {worst:.2e} over {ncols} columns")
    assert worst <= tol
    np.testing.assert_array_equal(got[ref.sum_rows:], panel[ref.sum_rows:])
    assert np.all(run.got[:, ref.mat_rows:] == SENTINEL), "the padding rows of qtc between mat_rows and ldq were written"


# ---- thin tiles: bdqr_thin_panel.hip ---------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (2, 1), (2, 2), (3, 1), (7, 2), (9, 2), (16, 2)]
TILES = [5, 256, 300, 1024]         # one partial workgroup, one exact, one full plus partial, several chunks
WIDTHS = [1, 2, 6, 33, 385]         # remainders of every group size (4, 2, 1 columns); the column-slice split with and without a ragged slice


def thin_cases():
    """The product thinned: every value of every axis with every shape's neighbours rotating, plus the corners."""
    cases = []
    for i, (r, c) in enumerate(SHAPES):
        for k in range(4):
            cases.append((r, c, TILES[(i + k) % 4], WIDTHS[(i + 2 * k) % 5], (i + k) % 2, (i + k // 2) % 2))
    for (r, c) in ((7, 2), (2, 1), (16, 2)):
        cases += [(r, c, 5, 385, 0, FULL_Q), (r, c, 1024, 385, 0, FULL_Q), (r, c, 300, 33, 1, BLOCK_DIAGONAL_Q)]
    cases += [(7, 2, 1024, 385, 1, BLOCK_DIAGONAL_Q), (9, 2, 300, 33, 0, FULL_Q), (3, 1, 1024, 6, 0, BLOCK_DIAGONAL_Q)]
    return sorted(set(cases))


def test_thin_cases_cover_every_axis():
    cases = thin_cases()
    for axis, values in ((0, {r for r, _ in SHAPES}), (2, set(TILES)), (3, set(WIDTHS)), (4, {0, 1}), (5, {0, 1})):
        assert {case[axis] for case in cases} == values
    assert {(r, c) for r, c, *_ in cases} == set(SHAPES)


@pytest.mark.parametrize("r,c,B,ncols,solver,qf", thin_cases())
def test_thin_panel_matches_oracle(qa, ctx, r, c, B, ncols, solver, qf):
    """mat_rows = the tiles' rows + 5 (trailing identity rows), ldc = mat_rows + 3 and ldq = mat_rows + 5 made odd, ldc != ldq."""
    ref = uniform_ref(B, r, c, 0.5, 5.0, 1 + r + c, 5, qf, solver)
    panel = panel_for(ref, ncols)
    ldc, ldq = odd_lds(ref.mat_rows)
    assert ldc % 2 == 1 and ldq % 2 == 1 and ldc != ldq
    run = Run(qa, ctx, ref, panel, ldc, ldq, hc=(B + ncols) % 2 == 0)
    assert KERNEL in run.qr.panelKernelName(ncols)
    check_factors(run)
    check_panel(run, panel)


def test_thin_panel_tight_leading_dimensions_and_no_trailing_rows(qa, ctx):
    """ldc = ldq = mat_rows = the tiles' rows: the contiguous panel qrk_bd_apply_qt takes"""
    for (r, c, B, ncols) in ((7, 2, 300, 33), (2, 1, 600, 6)):
        ref = uniform_ref(B, r, c, 0.5, 5.0, 4, 0, FULL_Q, 0)
        panel = panel_for(ref, ncols)
        run = Run(qa, ctx, ref, panel, ref.mat_rows, ref.mat_rows)
        check_factors(run)
        check_panel(run, panel)


def test_two_identical_calls_give_the_same_bits(qa, ctx):
    ref = uniform_ref(1024, 7, 2, 0.5, 5.0, 10, 5, FULL_Q, 0)
    panel = panel_for(ref, 385)
    ldc, ldq = odd_lds(ref.mat_rows)
    a = Run(qa, ctx, ref, panel, ldc, ldq)
    b = Run(qa, ctx, ref, panel, ldc, ldq, mat=a.mat, qr=a.qr)
    np.testing.assert_array_equal(a.got, b.got)
    np.testing.assert_array_equal(a.r.cpu().numpy(), b.r.cpu().numpy())


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
def test_tie_tiles_are_redone_exactly(qa, ctx, kind):
    B, r, c, ncols = 300, 7, 2, 33
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    ref = Ref(rows, cols, tie_tiles(kind, B, r, c, 5), B * r + 5, FULL_Q, 0)
    panel = panel_for(ref, ncols)
    ldc, ldq = odd_lds(ref.mat_rows)
    run = Run(qa, ctx, ref, panel, ldc, ldq)
    assert KERNEL in run.qr.panelKernelName(ncols)
    check_factors(run)
    check_panel(run, panel)
    # ... and a clean batch right behind it on the same plan: the redo list was consumed and reset
    ref2 = uniform_ref(B, r, c, 0.5, 5.0, 9, 5, FULL_Q, 0)
    panel2 = panel_for(ref2, ncols, seed=1)
    mat2 = qa.SparseBlockDiagonal.fromTiles(rows, cols, ref2.tiles, rows=ref2.mat_rows)
    run2 = Run(qa, ctx, ref2, panel2, ldc, ldq, mat=mat2, qr=run.qr)
    check_factors(run2)
    check_panel(run2, panel2)


# ---- dispatch ------------------------------------------------------------------------------------------------------------------

def analysed(qa, ctx, rows, cols):
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    qr.analyzePattern(qa.SparseBlockDiagonal.fromTiles(rows, cols, np.zeros(int((rows.astype(np.int64) * cols).sum()))))
    return qr


def test_dispatch_names_the_kernels(qa, ctx):
    """Without this a build that always takes the fallback would pass everything else."""
    def uni(B, r, c):
        return analysed(qa, ctx, np.full(B, r, np.int32), np.full(B, c, np.int32))
    thin = uni(10, 7, 2)
    for w in (1, 5, 64, 385):
        assert KERNEL in thin.panelKernelName(w)
    assert KERNEL in uni(10, 16, 2).panelKernelName(385) and KERNEL in uni(10, 1, 1).panelKernelName(1)
    assert "fallback" in uni(10, 8, 6).panelKernelName(5)
    assert "fallback" in uni(10, 32, 32).panelKernelName(5)
    assert "fallback" in analysed(qa, ctx, np.array([7, 9, 7], np.int32), np.array([2, 2, 1], np.int32)).panelKernelName(5)
    # qrk_bd_rhs_kernel_name answers as before (tests/test_qless_gpu.py, test_dispatch_names_the_kernels)
    assert "bdqr_thin_rhs_kernel" in thin.rhsKernelName(1)
    assert "bdqr_thin_rhs_kernel" in uni(10, 9, 2).rhsKernelName(1)
    assert "bdqr_pair4_rhs_kernel" in uni(10, 32, 32).rhsKernelName(1)
    assert "bdqr_pair4_rhs_kernel" in uni(10, 32, 32).rhsKernelName(32)
    assert "fallback" in uni(10, 8, 6).rhsKernelName(1)
    assert "fallback" in uni(10, 32, 32).rhsKernelName(33)
    assert "fallback" in thin.rhsKernelName(64) and "fallback" in thin.rhsKernelName(5)
    assert "fallback" in uni(10, 64, 64).rhsKernelName(1)


# ---- plans without the thin kernel: the explicit kernels through the plan's scratch -----------------------------------------------

def check_fallback(qa, ctx, ref, ncols):
    import torch
    panel = panel_for(ref, ncols)
    ldc, ldq = odd_lds(ref.mat_rows)
    run = Run(qa, ctx, ref, panel, ldc, ldq)
    assert "fallback" in run.qr.panelKernelName(ncols)
    check_factors(run)
    check_panel(run, panel)
    qr = run.qr
    qr.compute(run.mat)
    assert torch.equal(qr.rValues(), run.r[:ref.ref.R_vals.size]) and torch.equal(qr.hCoeffs(), run.hc[:ref.mat_cols])
    np.testing.assert_array_equal(qr.colsPermutation(), run.p.cpu().numpy()[:ref.mat_cols])
    got = run.got[:, :ref.mat_rows].T
    np.testing.assert_array_equal(got, qr.applyQt(panel))        # the same kernels on the same Q: the same bits
    for j in range(ncols):                                         # ... and column by column
        np.testing.assert_array_equal(got[:, j], qr.applyQt(np.ascontiguousarray(panel[:, j])))


def test_fallback_8x6_matches_oracle_and_the_explicit_route(qa, ctx):
    check_fallback(qa, ctx, uniform_ref(300, 8, 6, -1.0, 1.0, 7, 5, FULL_Q, 0), 6)


def test_fallback_mixed_batch(qa, ctx):
    rng = np.random.default_rng(7)                           # the 400-tile mixed batch of test_bd_gpu.py
    B = 400
    cols = rng.integers(1, 33, B).astype(np.int32)
    rows = (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32)
    tiles = seeded_tiles(11, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    check_fallback(qa, ctx, Ref(rows, cols, tiles, int(rows.sum()) + 5, FULL_Q, 0), 6)


def test_fallback_many_columns_with_padded_leading_dimensions(qa, ctx):
    """33 columns take the many-right-hand-sides kernel of qrk_bd_apply_qt: the strides reach it too (against the oracle and the
    whole-panel applyQt)"""
    ref = uniform_ref(300, 8, 6, -1.0, 1.0, 7, 5, FULL_Q, 0)
    panel = panel_for(ref, 33)
    ldc, ldq = odd_lds(ref.mat_rows)
    run = Run(qa, ctx, ref, panel, ldc, ldq)
    check_factors(run)
    check_panel(run, panel)
    run.qr.compute(run.mat)
    np.testing.assert_array_equal(run.got[:, :ref.mat_rows].T, run.qr.applyQt(panel))


# ---- arguments, landscape, host memory, no columns -----------------------------------------------------------------------------

def test_argument_checks_and_landscape(qa, ctx):
    import torch
    from qrkit_amd import _capi as capi
    ref = uniform_ref(10, 7, 2, 0.5, 5.0, 10, 0, FULL_Q, 0)
    mat = qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, ref.tiles, rows=ref.mat_rows)
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    qr.analyzePattern(mat)
    lib, dev, n = capi.lib(), ctx.device, ref.mat_rows
    t = mat.device_tiles(dev)
    c = torch.zeros(3 * (n + 2), dtype=torch.float64, device=dev)
    y = torch.zeros(3 * (n + 2), dtype=torch.float64, device=dev)
    r = torch.zeros(30, dtype=torch.float64, device=dev)
    p = torch.zeros(ref.mat_cols, dtype=torch.int32, device=dev)

    def call(tiles=t.data_ptr(), cc=c.data_ptr(), ldc=n + 2, ncols=3, rr=r.data_ptr(), pp=p.data_ptr(), yy=y.data_ptr(), ldq=n + 2):
        return lib.qrk_bd_factorize_apply_qt(qr._plan, tiles, cc, ldc, ncols, rr, pp, None, yy, ldq, capi.MEM_DEVICE)

    def refused(**kw):
        st = call(**kw)
        return st == capi.STATUS_INVALID_ARGUMENT and len(lib.qrk_last_error(ctx.handle)) > 0

    assert call() == capi.STATUS_OK
    assert refused(ldc=n - 1) and refused(ldq=n - 1)
    assert refused(ncols=-1)
    assert refused(tiles=None) and refused(rr=None) and refused(pp=None) and refused(cc=None) and refused(yy=None)
    # Every span below lies inside the 3 * (n + 2) = 216 doubles of the tensor it points into (n = 70, ld = 72: a panel of k columns
    # spans (k - 1) * 72 + 70 elements), the refused ones too, although they never reach a kernel.
    assert refused(yy=c.data_ptr())                                          # the same span: c and qtc both c[0, 214)
    assert refused(yy=c.data_ptr() + 8 * (n - 1), ncols=1)                   # the first entry of qtc is the last of c: c[0, 70), qtc c[69, 139)
    assert refused(cc=y.data_ptr() + 8 * (n + 2), ncols=2)                   # c inside the span of qtc: c y[72, 214), qtc y[0, 142)
    assert call(cc=y.data_ptr() + 8 * n, ncols=1, yy=y.data_ptr()) == capi.STATUS_OK      # back to back, no overlap: qtc y[0, 70), c y[70, 140)
    assert call(cc=None, yy=None, ncols=0) == capi.STATUS_OK                 # no columns: no panel needed
    # a landscape tile: InvalidInput, as after qrk_bd_factorize
    rows, cols = np.array([4, 3], np.int32), np.array([2, 5], np.int32)
    lm = qa.SparseBlockDiagonal.fromTiles(rows, cols, seeded_tiles(1, -1, 1, 4 * 2 + 3 * 5))
    q2 = qa.BlockDiagonalSparseQR(context=ctx)
    q2.analyzePattern(lm)
    assert q2.factorizeApplyQtDevice(lm, c.data_ptr(), 7, 1, y.data_ptr(), 7) is None
    assert q2.info() == qa.INFO_INVALID_INPUT and not q2.m_isInitialized


def test_no_columns_gives_the_factors_only(qa, ctx):
    for ref in (uniform_ref(300, 7, 2, 0.5, 5.0, 10, 5, FULL_Q, 0), uniform_ref(300, 8, 6, -1.0, 1.0, 7, 5, FULL_Q, 0)):
        run = Run(qa, ctx, ref, np.zeros((ref.mat_rows, 0)), ref.mat_rows, ref.mat_rows)
        check_factors(run)
        assert np.all(run.out.cpu().numpy() == SENTINEL)


def test_facade_state_after_factorize_apply_qt(qa, ctx):
    """BlockDiagonalSparseQR.factorizeApplyQtDevice leaves the state of factorizeAndSolve(): no Q, but R and solveR."""
    import torch
    ref = uniform_ref(300, 7, 2, 0.5, 5.0, 10, 0, FULL_Q, 0)
    mat = qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, ref.tiles, rows=ref.mat_rows)
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    qr.analyzePattern(mat)
    b = panel_for(ref, 1)[:, 0]
    cin = torch.from_numpy(b).to(ctx.device)
    out = torch.empty_like(cin)
    qr.factorizeApplyQtDevice(mat, cin.data_ptr(), ref.mat_rows, 1, out.data_ptr(), ref.mat_rows)
    for call in (qr.qValues, qr.matrixQ, lambda: qr.solve(b), lambda: qr.applyQt(b), lambda: qr.applyQ(b)):
        with pytest.raises(RuntimeError, match="factorised without Q"):
            call()
    assert qr.rank() == ref.ref.rank and qr.info() == 0
    np.testing.assert_array_equal(qr.colsPermutation(), ref.ref.perm)
    z = qr.solveR(out[:ref.mat_cols].cpu().numpy())
    x = np.zeros_like(z); x[qr.colsPermutation()] = z
    want = ref.prob.solve(ref.ref, b)
    assert np.linalg.norm(x - want) <= 1e-11 * np.linalg.norm(want)
    qr.compute(mat)
    assert qr.qValues().numel() == ref.ref.Q_vals.size


def test_host_memory_space(qa, ctx):
    """QRK_MEM_HOST stages like qrk_bd_factorize_rhs: host arrays in, host arrays out, the padding rows of qtc kept."""
    from qrkit_amd import _capi as capi
    ref = uniform_ref(300, 9, 2, 0.5, 5.0, 12, 5, FULL_Q, 0)
    mat = qa.SparseBlockDiagonal.fromTiles(ref.rows, ref.cols, ref.tiles, rows=ref.mat_rows)
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    qr.analyzePattern(mat)
    ncols = 6
    panel = panel_for(ref, ncols)
    ldc, ldq = odd_lds(ref.mat_rows)
    cbuf = np.zeros((ncols, ldc)); cbuf[:, :ref.mat_rows] = panel.T
    out = np.full((ncols, ldq), SENTINEL)
    r = np.zeros(ref.ref.R_vals.size); p = np.zeros(ref.mat_cols, np.int32); hc = np.zeros(ref.mat_cols)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(capi.lib().qrk_bd_factorize_apply_qt(qr._plan, ptr(ref.tiles), ptr(cbuf), ldc, ncols, ptr(r), ptr(p), ptr(hc), ptr(out), ldq,
                                                    capi.MEM_HOST), ctx.handle)
    np.testing.assert_array_equal(p, ref.ref.perm)
    _, sr, sc = tile_sizes(ref.rows, ref.cols)
    assert per_tile_rel(r, ref.ref.R_vals, sr) <= RTOL and per_tile_rel(hc, ref.ref.hcoeffs, sc) <= RTOL
    got, want = out[:, :ref.mat_rows].T, ref.Q.T @ panel
    assert max(per_tile_rel(got[ref.qt_idx, j], want[ref.qt_idx, j], ref.rows) for j in range(ncols)) <= RTOL
    np.testing.assert_array_equal(got[ref.sum_rows:], panel[ref.sum_rows:])
    assert np.all(out[:, ref.mat_rows:] == SENTINEL)
