"""GPU: the Levenberg-Marquardt primitives on the block-diagonal factors (qrk_bd_lm_solve / qrk_bd_lm_gradient / qrk_bd_r_col_norms;
BlockDiagonalSparseQR.lmSolve / lmGradient / colNorms) against the dense numpy judge of lm_reference.py.

The judge reads the SAME R, permutation and y the device call reads (copied back from the device): the factorisation's own error
does not enter.  Tolerances, per tile: x 1e-11 on seeded_tiles(., 0.5, 5.0) data and 1e-9 on (-1, 1) data (the 32-column shapes and
the mixed batch) -- the project's tolerances of the plain solve; the sums and gnorm2 1e-9 wherever par >= 1e-2 with diag =
colNorms() (the stack's condition number is at most sqrt(c (1 + par) / par) ~ 60 there: cond^2 c eps ~ 2e-11), at par = 0 on the
tall (0.5, 5.0) shapes only; g and colNorms() 1e-13 per tile.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import lm_reference as judge
from helpers import seeded_tiles

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1
SHAPES = [(5, 1), (7, 2), (9, 2), (8, 3), (8, 6), (12, 8), (16, 9), (16, 16), (40, 17), (40, 32), (32, 32)]
SIZES = [1, 5, 63, 65, 300]
PARS = [0.0, 1e-2, 1.0, 1e2]
DIAGS = ["none", "seeded"]          # next to diag = colNorms(), which every case runs
EXTRA = 5                           # trailing identity rows


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


def data_range(c):
    return (-1.0, 1.0) if c == 32 else (0.5, 5.0)


def x_tol(c):
    return 1e-9 if c == 32 else 1e-11


def cases():
    """The product shapes x sizes x solvers x diag thinned as test_panel_gpu.thin_cases() thins its own: every value of every axis
    with every shape's neighbours rotating, plus the corners."""
    out = []
    for i, (r, c) in enumerate(SHAPES):
        for k in range(4):
            out.append((r, c, SIZES[(i + k) % 5], (i + k) % 2, DIAGS[(i + k // 2) % 2]))
    for (r, c) in ((7, 2), (16, 9), (32, 32)):
        out += [(r, c, 1, 0, "none"), (r, c, 300, 1, "seeded"), (r, c, 65, 0, "seeded")]
    return sorted(set(out))


def test_cases_cover_every_axis():
    cs = cases()
    for axis, values in ((2, set(SIZES)), (3, {0, 1}), (4, set(DIAGS))):
        assert {case[axis] for case in cs} == values
    assert {(r, c) for r, c, *_ in cs} == set(SHAPES)


class Batch:
    """One factorised batch: the solver, and R / the permutation / y as the device holds them, cut for the judge."""

    def __init__(self, qa, ctx, rows, cols, tiles, solver, seed, q_format=FULL_Q):
        self.rows, self.cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
        self.mat_rows, self.mat_cols = int(self.rows.sum()) + EXTRA, int(self.cols.sum())
        self.mat = qa.SparseBlockDiagonal.fromTiles(self.rows, self.cols, tiles, rows=self.mat_rows)
        self.qr = qa.BlockDiagonalSparseQR(blockSolver=solver, qFormat=q_format, context=ctx)
        self.qr.compute(self.mat)
        assert self.qr.info() == 0
        rng = np.random.default_rng(1000 + seed)
        self.y = rng.uniform(-1.0, 1.0, self.mat_cols)
        self.seeded_diag = rng.uniform(0.5, 2.0, self.mat_cols)
        self.t = judge.Tiles(self.cols, self.qr.rValues().cpu().numpy(), self.qr.colsPermutation(), self.y)
        norms = self.qr.colNorms()
        self.norms = norms
        self.diag = np.where(norms == 0.0, 1.0, norms)

    def diag_of(self, mode):
        return {"norms": self.diag, "none": None, "seeded": self.seeded_diag}[mode]


@functools.lru_cache(maxsize=None)
def uniform_batch(qa, ctx, B, r, c, solver):
    lo, hi = data_range(c)
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    return Batch(qa, ctx, rows, cols, seeded_tiles(1 + r + c, lo, hi, B * r * c), solver, r * 100 + c)


@functools.lru_cache(maxsize=None)
def mixed_batch(qa, ctx):
    rng = np.random.default_rng(7)                           # the 400-tile mixed batch of test_qless_gpu.test_fallback_mixed_batch
    B = 400
    cols = rng.integers(1, 33, B).astype(np.int32)
    rows = (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32)
    tiles = seeded_tiles(11, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    return Batch(qa, ctx, rows, cols, tiles, 0, 7)


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def check_solve(b, mode, par, xtol, sums_tol):
    """x per tile and, where sums_tol is given, the three sums against the judge"""
    diag = b.diag_of(mode)
    x, sums = b.qr.lmSolve(b.y, diag, par, returnSums=True)
    assert x.shape == (b.mat_cols,) and isinstance(x, np.ndarray)
    want_x, want_s, _ = judge.solve(b.t, diag, par)
    ex = judge.per_tile_rel(x, want_x, b.t)
    e0, e1 = rel(sums[0], want_s[0]), rel(sums[1], want_s[1])
    print(f"diag {mode} par {par:g}: x per tile {ex:.2e}, sums[0] {e0:.2e}, sums[1] {e1:.2e}, sums[2] {sums[2]:g}")
    assert ex <= xtol
    assert sums[2] == want_s[2]
    if sums_tol is not None:
        assert e0 <= sums_tol and e1 <= sums_tol
    np.testing.assert_array_equal(b.qr.lmSolve(b.y, diag, par), x)          # without the sums: the same x


# ---- the damped solve and its sums ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c,B,solver,mode", cases())
def test_solve_matches_judge(qa, ctx, r, c, B, solver, mode):
    b = uniform_batch(qa, ctx, B, r, c, solver)
    tall = r > c and c != 32                                  # the tall (0.5, 5.0) shapes: the sums are compared at par = 0 too
    for par in PARS:
        check_solve(b, "norms", par, x_tol(c), 1e-9 if (par >= 1e-2 or tall) else None)
        check_solve(b, mode, par, x_tol(c), None)


def test_solve_mixed_batch(qa, ctx):
    b = mixed_batch(qa, ctx)
    assert "bd_lm_group_kernel<64>" in b.qr.lmKernelName()
    for par in PARS:
        check_solve(b, "norms", par, 1e-9, 1e-9 if par >= 1e-2 else None)
        check_solve(b, "seeded", par, 1e-9, None)
    check_solve(b, "none", 1.0, 1e-9, None)


@pytest.mark.parametrize("r,c", [(7, 2), (8, 6), (16, 16)])
def test_zero_columns_and_the_nsing_rule(qa, ctx, r, c):
    """Every third tile has a zero column: its R has an exact zero on the diagonal (the pivoted solver puts it last), z is zero from
    there on and the tile adds nothing to sums[1]; sums[2] counts those tiles."""
    B = 65
    tiles = seeded_tiles(3 + r + c, 0.5, 5.0, B * r * c).reshape(B, c, r).copy()
    tiles[::3, c // 2, :] = 0.0
    b = Batch(qa, ctx, np.full(B, r, np.int32), np.full(B, c, np.int32), tiles.reshape(-1), 0, 5)
    singular = sum(1 for R in b.t.R if np.any(np.diag(R) == 0.0))
    assert singular == len(range(0, B, 3))
    assert np.count_nonzero(b.norms == 0.0) == singular       # colNorms(): an exact zero is written as zero
    for par in (0.0, 1.0):
        x, sums = b.qr.lmSolve(b.y, b.diag, par, returnSums=True)
        want_x, want_s, _ = judge.solve(b.t, b.diag, par)
        assert sums[2] == singular == want_s[2]
        assert judge.per_tile_rel(x, want_x, b.t) <= 1e-11
        assert rel(sums[0], want_s[0]) <= 1e-9 and rel(sums[1], want_s[1]) <= 1e-9
        if par == 0.0:
            zero_cols = b.qr.colsPermutation()[np.arange(0, B, 3) * c + c - 1]
            assert np.all(x[zero_cols] == 0.0)


# ---- gradient and column norms ----------------------------------------------------------------------------------------------------

def per_tile_abs_rel(got, want, t):
    return judge.per_tile_rel(got, want, t)


@pytest.mark.parametrize("r,c,B", [(5, 1, 65), (7, 2, 300), (8, 6, 63), (16, 16, 65), (40, 32, 5), (32, 32, 63)])
def test_gradient_and_col_norms(qa, ctx, r, c, B):
    b = uniform_batch(qa, ctx, B, r, c, 0)
    check_gradient_and_norms(b)


def check_gradient_and_norms(b):
    for mode in ("norms", "none", "seeded"):
        diag = b.diag_of(mode)
        g, gnorm = b.qr.lmGradient(b.y, diag)
        want_g, want_n2 = judge.gradient(b.t, diag)
        eg, en = per_tile_abs_rel(g, want_g, b.t), rel(gnorm ** 2, want_n2)
        print(f"diag {mode}: g per tile {eg:.2e}, gnorm2 {en:.2e}")
        assert eg <= 1e-13 and en <= 1e-9
    assert per_tile_abs_rel(b.norms, judge.col_norms(b.t), b.t) <= 1e-13
    # Q^T b with rows() entries: the first cols() are used
    long_y = np.concatenate([b.y, np.full(b.mat_rows - b.mat_cols, 7.0)])
    np.testing.assert_array_equal(b.qr.lmGradient(long_y, None)[0], b.qr.lmGradient(b.y, None)[0])
    np.testing.assert_array_equal(b.qr.lmSolve(long_y, None, 1.0), b.qr.lmSolve(b.y, None, 1.0))


def test_gradient_and_col_norms_mixed_batch(qa, ctx):
    check_gradient_and_norms(mixed_batch(qa, ctx))


def test_torch_in_torch_out(qa, ctx):
    import torch
    b = uniform_batch(qa, ctx, 63, 8, 6, 0)
    y, d = torch.from_numpy(b.y).to(ctx.device), torch.from_numpy(b.diag).to(ctx.device)
    x = b.qr.lmSolve(y, d, 1.0)
    g, _ = b.qr.lmGradient(y, d)
    assert isinstance(x, torch.Tensor) and x.is_cuda and isinstance(g, torch.Tensor) and g.is_cuda
    np.testing.assert_array_equal(x.cpu().numpy(), b.qr.lmSolve(b.y, b.diag, 1.0))
    assert isinstance(b.qr.colNormsDevice(), torch.Tensor)


# ---- repeatability, the host memory space ---------------------------------------------------------------------------------------

def all_batches(qa, ctx):
    return [uniform_batch(qa, ctx, 300, 7, 2, 0), uniform_batch(qa, ctx, 300, 16, 9, 0), uniform_batch(qa, ctx, 63, 32, 32, 1),
            mixed_batch(qa, ctx)]


def test_two_identical_calls_give_identical_bits(qa, ctx):
    for b in all_batches(qa, ctx):
        for par in (0.0, 1.0):
            x1, s1 = b.qr.lmSolve(b.y, b.diag, par, returnSums=True)
            x2, s2 = b.qr.lmSolve(b.y, b.diag, par, returnSums=True)
            np.testing.assert_array_equal(x1, x2)
            np.testing.assert_array_equal(s1, s2)
        g1, n1 = b.qr.lmGradient(b.y, b.diag)
        g2, n2 = b.qr.lmGradient(b.y, b.diag)
        np.testing.assert_array_equal(g1, g2)
        assert n1 == n2


def test_host_memory_space_gives_the_devices_bits(qa, ctx):
    from qrkit_amd import _capi as capi
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for b in all_batches(qa, ctx):
        r = np.ascontiguousarray(b.qr.rValues().cpu().numpy())
        p = np.ascontiguousarray(b.qr.colsPermutation(), dtype=np.int32)
        y, d = np.ascontiguousarray(b.y), np.ascontiguousarray(b.diag)
        x, sums = np.zeros(b.mat_cols), np.zeros(3)
        capi.check(capi.lib().qrk_bd_lm_solve(b.qr._plan, ptr(r), ptr(p), ptr(y), ptr(d), 1.0, ptr(x), ptr(sums), capi.MEM_HOST), ctx.handle)
        dx, dsums = b.qr.lmSolve(b.y, b.diag, 1.0, returnSums=True)
        np.testing.assert_array_equal(x, dx)
        np.testing.assert_array_equal(sums, dsums)
        g, n2 = np.zeros(b.mat_cols), np.zeros(1)
        capi.check(capi.lib().qrk_bd_lm_gradient(b.qr._plan, ptr(r), ptr(p), ptr(y), None, ptr(g), ptr(n2), capi.MEM_HOST), ctx.handle)
        dg, dn = b.qr.lmGradient(b.y, None)
        np.testing.assert_array_equal(g, dg)
        assert float(np.sqrt(n2[0])) == dn
        nrm = np.zeros(b.mat_cols)
        capi.check(capi.lib().qrk_bd_r_col_norms(b.qr._plan, ptr(r), ptr(p), ptr(nrm), capi.MEM_HOST), ctx.handle)
        np.testing.assert_array_equal(nrm, b.norms)


# ---- dispatch and refusals ------------------------------------------------------------------------------------------------------

def analysed(qa, ctx, B, r, c, q_format=FULL_Q):
    rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    qr = qa.BlockDiagonalSparseQR(context=ctx, qFormat=q_format)
    qr.analyzePattern(qa.SparseBlockDiagonal.fromTiles(rows, cols, np.zeros(B * r * c)))
    return qr


def test_dispatch_names_the_kernels(qa, ctx):
    """Without this a build that sends everything through one kernel would pass the rest."""
    want = {(5, 1): "bd_lm_thin_kernel", (7, 2): "bd_lm_thin_kernel", (9, 2): "bd_lm_thin_kernel", (8, 3): "bd_lm_group_kernel<8>",
            (8, 6): "bd_lm_group_kernel<8>", (12, 8): "bd_lm_group_kernel<16>", (16, 9): "bd_lm_group_kernel<16>",
            (16, 16): "bd_lm_group_kernel<32>", (40, 17): "bd_lm_group_kernel<32>", (40, 32): "bd_lm_group_kernel<64>",
            (32, 32): "bd_lm_group_kernel<64>", (8, 7): "bd_lm_group_kernel<8>", (16, 15): "bd_lm_group_kernel<16>",
            (32, 31): "bd_lm_group_kernel<32>"}
    assert set(SHAPES) <= set(want)
    for (r, c), name in want.items():
        got = analysed(qa, ctx, 10, r, c).lmKernelName()
        assert name in got and "unsupported" not in got, (r, c, got)


def test_unsupported_plans_are_refused(qa, ctx):
    import torch
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    for qr, n, nr, why in ((analysed(qa, ctx, 2, 64, 64), 128, 2 * 64 * 65 // 2, b"more than 32 columns"),
                           (analysed(qa, ctx, 10, 7, 2, BLOCK_DIAGONAL_Q), 20, 30, b"FullQ")):
        assert "unsupported" in qr.lmKernelName()
        r = torch.ones(nr, dtype=torch.float64, device=ctx.device)
        p = torch.arange(n, dtype=torch.int32, device=ctx.device)
        y, x = torch.ones(n, dtype=torch.float64, device=ctx.device), torch.zeros(n, dtype=torch.float64, device=ctx.device)
        one = torch.zeros(4, dtype=torch.float64, device=ctx.device)
        U = capi.STATUS_UNSUPPORTED
        assert lib.qrk_bd_lm_solve(qr._plan, r.data_ptr(), p.data_ptr(), y.data_ptr(), None, 1.0, x.data_ptr(), None, capi.MEM_DEVICE) == U
        assert b"qrk_bd_lm_solve" in lib.qrk_last_error(ctx.handle) and why in lib.qrk_last_error(ctx.handle)
        assert lib.qrk_bd_lm_gradient(qr._plan, r.data_ptr(), p.data_ptr(), y.data_ptr(), None, x.data_ptr(), one.data_ptr(), capi.MEM_DEVICE) == U
        assert lib.qrk_bd_r_col_norms(qr._plan, r.data_ptr(), p.data_ptr(), x.data_ptr(), capi.MEM_DEVICE) == U
        par = C.c_double(0.0)
        assert lib.qrk_bd_lmpar(qr._plan, r.data_ptr(), p.data_ptr(), y.data_ptr(), None, 1.0, C.byref(par), x.data_ptr(), None, None) == U


def test_argument_checks(qa, ctx):
    import torch
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    qr = analysed(qa, ctx, 10, 7, 2)
    r = torch.ones(30, dtype=torch.float64, device=ctx.device)
    p = torch.arange(20, dtype=torch.int32, device=ctx.device)
    y, x = torch.ones(20, dtype=torch.float64, device=ctx.device), torch.zeros(20, dtype=torch.float64, device=ctx.device)
    I = capi.STATUS_INVALID_ARGUMENT
    solve = lambda rr, pp, yy, par, xx: lib.qrk_bd_lm_solve(qr._plan, rr, pp, yy, None, par, xx, None, capi.MEM_DEVICE)
    assert solve(None, p.data_ptr(), y.data_ptr(), 1.0, x.data_ptr()) == I
    assert solve(r.data_ptr(), None, y.data_ptr(), 1.0, x.data_ptr()) == I
    assert solve(r.data_ptr(), p.data_ptr(), None, 1.0, x.data_ptr()) == I
    assert solve(r.data_ptr(), p.data_ptr(), y.data_ptr(), 1.0, None) == I
    assert solve(r.data_ptr(), p.data_ptr(), y.data_ptr(), -1.0, x.data_ptr()) == I
    assert solve(r.data_ptr(), p.data_ptr(), y.data_ptr(), float("nan"), x.data_ptr()) == I
    assert solve(r.data_ptr(), p.data_ptr(), y.data_ptr(), 0.0, x.data_ptr()) == capi.STATUS_OK      # the arrays are the caller's: no factorize() needed
    par = C.c_double(0.0)
    lmpar = lambda delta: lib.qrk_bd_lmpar(qr._plan, r.data_ptr(), p.data_ptr(), y.data_ptr(), None, delta, C.byref(par), x.data_ptr(), None, None)
    assert lmpar(0.0) == I and lmpar(-1.0) == I and lmpar(float("nan")) == I
    par = C.c_double(-1.0)
    assert lmpar(1.0) == I


# ---- after the Q-less route -------------------------------------------------------------------------------------------------------

def test_after_factorize_and_solve(qa, ctx):
    """R, the permutation and Q^T b of factorizeAndSolve() are all the step needs: lmSolve at par = 0 is its x."""
    for (B, r, c, kernel) in ((300, 7, 2, "bdqr_thin_rhs_kernel"), (33, 32, 32, "bdqr_pair4_rhs_kernel")):
        lo, hi = data_range(c)
        rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, seeded_tiles(1 + r + c, lo, hi, B * r * c), rows=B * r + EXTRA)
        qr = qa.BlockDiagonalSparseQR(context=ctx)
        rhs = np.random.default_rng(3).uniform(-1.0, 1.0, B * r + EXTRA)
        x, qtb = qr.computeAndSolve(mat, rhs, returnQtB=True)
        assert kernel in qr.rhsKernelName(1)
        with pytest.raises(RuntimeError, match="factorised without Q"):
            qr.solve(rhs)
        t = judge.Tiles(cols, qr.rValues().cpu().numpy(), qr.colsPermutation(), qtb)
        x0 = qr.lmSolve(qtb, None, 0.0)
        err = judge.per_tile_rel(x0, x, t)
        print(f"{r}x{c}: lmSolve(par = 0) against factorizeAndSolve's x, per tile {err:.2e}")
        assert err <= 2 * x_tol(c)
        assert qr.lmpar(qtb, None, 2.0 * np.linalg.norm(x0))[0] == 0.0


def test_damped_solve_equals_the_refactorised_damped_tiles(qa, ctx):
    """The 7 x 2 tiles damped to 9 x 2 as test_lm_gpu.py damps them, factorised again for the trial lambda, against lmSolve on the
    undamped factors: the route the primitive replaces."""
    B, lam = 300, 1e-2
    J = seeded_tiles(10, 0.5, 5.0, B * 14).reshape(B, 2, 7)
    f = np.random.default_rng(4).uniform(-1.0, 1.0, (B, 7))
    damped = np.zeros((B, 2, 9))
    damped[:, :, :7] = J
    damped[:, 0, 7] = damped[:, 1, 8] = np.sqrt(lam)
    fd = np.zeros((B, 9)); fd[:, :7] = f
    qd = qa.BlockDiagonalSparseQR(context=ctx)
    xd = qd.computeAndSolve(qa.SparseBlockDiagonal.fromTiles(np.full(B, 9, np.int32), np.full(B, 2, np.int32), damped.ravel()), fd.ravel())
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    cols = np.full(B, 2, np.int32)
    _, qtb = qr.computeAndSolve(qa.SparseBlockDiagonal.fromTiles(np.full(B, 7, np.int32), cols, J.ravel()), f.ravel(), returnQtB=True)
    x = qr.lmSolve(qtb, np.ones(2 * B), lam)
    t = judge.Tiles(cols, qr.rValues().cpu().numpy(), qr.colsPermutation(), qtb)
    err = judge.per_tile_rel(x, xd, t)
    print(f"lmSolve(lambda) against factorizeAndSolve of the damped tiles, per tile {err:.2e}")
    assert err <= 2e-11
