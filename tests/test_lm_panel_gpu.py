"""GPU: qrk_bd_lm_panel alone -- the reflectors of the damped solve over a strided panel.

Inputs come from qrk_bd_factorize_rhs (BlockDiagonalSparseQR.computeAndSolve) on seeded Gaussian tiles.  The judge is numpy per tile
(lm_panel_reference.py) on the device's own R, permutation and panel, and shares nothing with the product:
    S_t^T S_t = R_t^T R_t + par Dt^2;   top_t = numpy's Q^T [C_t; 0] with rows sign-matched to the device's S;
    top_t^T top_t + F_t^T F_t = C_t^T C_t;   with ncols = 1 and c = y: qrk_bd_solve_r(s_vals, top) = qrk_bd_lm_solve's x per tile.
Each is judged at 1e-11 per tile (tests/test_lm_solve_gpu.py's bound); the worst seen is printed.
"""
import functools

import numpy as np
import pytest

import lm_panel_reference as judge
from helpers import seeded_tiles

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1
PARS = [1e-3, 1.0, 1e3]
TOL = 1e-11
SENT = -7.25                       # what the output buffers hold before a call


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


class Batch:
    """One factorised batch: the solver and R / the permutation / y as the device holds them."""

    def __init__(self, qa, ctx, rows, cols, tiles, seed):
        import torch
        self.qa, self.ctx = qa, ctx
        self.rows, self.cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
        self.mat_rows, self.mat_cols = int(self.rows.sum()), int(self.cols.sum())
        self.nnz_r = int((self.cols.astype(np.int64) * (self.cols + 1) // 2).sum())
        self.base = np.concatenate([[0], np.cumsum(self.cols)]).astype(np.int64)
        self.mat = qa.SparseBlockDiagonal.fromTiles(self.rows, self.cols, tiles, rows=self.mat_rows)
        self.qr = qa.BlockDiagonalSparseQR(blockSolver=0, qFormat=FULL_Q, context=ctx)
        rng = np.random.default_rng(2000 + seed)
        _, qtb = self.qr.computeAndSolve(self.mat, rng.standard_normal(self.mat_rows), returnQtB=True)     # qrk_bd_factorize_rhs
        self.y = np.ascontiguousarray(qtb[:self.mat_cols])
        assert self.qr.info() == 0
        self.r = self.qr.rValues().cpu().numpy()
        self.perm = self.qr.colsPermutation()
        self.Rs = judge.unpack_tiles(self.cols, self.r)
        self.norms = np.array([np.linalg.norm(R[:, k]) for R in self.Rs for k in range(R.shape[0])])
        self.diag = np.empty(self.mat_cols)
        self.diag[self.perm] = self.norms                            # column norms of J in the matrix's own column order
        self.torch = torch

    def panel(self, par, diag, Cmat, ncols, colidx=None, pad=0):
        """qrk_bd_lm_panel on the panel Cmat ((mat_cols + pad) x nsrc, numpy); returns (status, s_vals, top, fill) with top and fill
        as (mat_cols + pad) x ncols numpy arrays -- rows beyond mat_cols must still hold SENT."""
        torch, capi = self.torch, self.qa._capi
        dev = self.ctx.device
        ld = self.mat_cols + pad
        dc = torch.from_numpy(np.ascontiguousarray(Cmat.T)).to(dev) if Cmat is not None else None
        dd = torch.from_numpy(np.ascontiguousarray(diag)).to(dev) if diag is not None else None
        di = torch.from_numpy(np.ascontiguousarray(colidx, dtype=np.int32)).to(dev) if colidx is not None else None
        s = torch.full((max(self.nnz_r, 1),), SENT, dtype=torch.float64, device=dev)
        top = torch.full((max(ncols, 1), ld), SENT, dtype=torch.float64, device=dev)
        fill = torch.full((max(ncols, 1), ld), SENT, dtype=torch.float64, device=dev)
        self.ctx.use_current_stream()
        st = capi.lib().qrk_bd_lm_panel(self.qr._plan, self.qr._r.data_ptr(), self.qr._perm.data_ptr(),
                                        dd.data_ptr() if dd is not None else None, float(par),
                                        dc.data_ptr() if dc is not None else None, ld, ncols,
                                        di.data_ptr() if di is not None else None, s.data_ptr(), top.data_ptr(), ld, fill.data_ptr(), ld)
        torch.cuda.synchronize()
        return st, s.cpu().numpy()[:self.nnz_r], top.cpu().numpy().T, fill.cpu().numpy().T

    def kernel_name(self, ncols=1):
        return self.qa._capi.lib().qrk_bd_lm_panel_kernel_name(self.qr._plan, ncols).decode()


def gaussian_batch(qa, ctx, rows, cols, seed):
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    n = int((rows.astype(np.int64) * cols).sum())
    return Batch(qa, ctx, rows, cols, np.random.default_rng(seed).standard_normal(n), seed)


@functools.lru_cache(maxsize=None)
def uniform_batch(qa, ctx, B, r, c):
    return gaussian_batch(qa, ctx, np.full(B, r), np.full(B, c), 100 * r + c + B)


@functools.lru_cache(maxsize=None)
def thin_mixed_batch(qa, ctx):
    cols = np.random.default_rng(3).integers(1, 3, 300)
    return gaussian_batch(qa, ctx, cols + 4, cols, 31)


@functools.lru_cache(maxsize=None)
def mixed_batch(qa, ctx):
    rng = np.random.default_rng(7)                           # the 400-tile mixed batch of tests/test_lm_solve_gpu.py
    B = 400
    cols = rng.integers(1, 33, B).astype(np.int32)
    rows = (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32)
    tiles = seeded_tiles(11, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    return Batch(qa, ctx, rows, cols, tiles, 7)


def rel(a, b):
    den = np.linalg.norm(b)
    return np.linalg.norm(a - b) / den if den > 0 else np.linalg.norm(a - b)


def check_panel(b, par, mode, ncols, colidx=None, pad=0, nsrc=None, seed=0):
    """One call against the three per-tile identities; returns the worst relative errors (S, top, Gram)."""
    diag = b.diag if mode == "norms" else None
    nsrc = ncols if nsrc is None else nsrc
    rng = np.random.default_rng(4000 + seed)
    Cmat = np.full((b.mat_cols + pad, max(nsrc, 1)), 3.5)
    Cmat[:b.mat_cols] = rng.standard_normal((b.mat_cols, max(nsrc, 1)))
    st, s, top, fill = b.panel(par, diag, Cmat if ncols > 0 else None, ncols, colidx, pad)
    assert st == 0
    src = np.arange(ncols) if colidx is None else np.asarray(colidx)
    if pad:                                                   # the rows beyond mat_cols are not touched
        assert np.all(top[b.mat_cols:] == SENT) and np.all(fill[b.mat_cols:] == SENT)
    if ncols == 0:
        assert np.all(top == SENT) and np.all(fill == SENT)
    D = np.ones(b.mat_cols) if diag is None else diag
    Ss = judge.unpack_tiles(b.cols, s)
    worst = np.zeros(3)
    for t, (R, S) in enumerate(zip(b.Rs, Ss)):
        lo, hi = int(b.base[t]), int(b.base[t + 1])
        dt = D[b.perm[lo:hi]]
        want = R.T @ R + par * np.diag(dt * dt)
        worst[0] = max(worst[0], rel(S.T @ S, want))
        if ncols > 0:
            Ct = Cmat[lo:hi][:, src]
            Sn, topn, _ = judge.tile_step(R, dt, par, Ct)
            _, topn = judge.match_signs(Sn, topn, np.diag(S))
            worst[1] = max(worst[1], rel(top[lo:hi, :ncols], topn))
            gram = top[lo:hi, :ncols].T @ top[lo:hi, :ncols] + fill[lo:hi, :ncols].T @ fill[lo:hi, :ncols]
            worst[2] = max(worst[2], rel(gram, Ct.T @ Ct))
    print(f"B {len(b.cols)} par {par:g} diag {mode} ncols {ncols} pad {pad}: S^T S {worst[0]:.2e}  top {worst[1]:.2e}  Gram {worst[2]:.2e}")
    assert worst.max() <= TOL
    return worst


# ---- the thin kernel: tiles of 1 or 2 columns ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c", [(2, 1), (7, 2)])
@pytest.mark.parametrize("B", [1, 257, 1024])
def test_thin_batches(qa, ctx, r, c, B):
    b = uniform_batch(qa, ctx, B, r, c)
    assert b.kernel_name(6) == "qrk::lm::bd_lm_panel_thin_kernel"
    for i, par in enumerate(PARS):
        check_panel(b, par, ("none", "norms")[i % 2], 6, seed=i)
        check_panel(b, par, ("norms", "none")[i % 2], 1, seed=10 + i)


@pytest.mark.parametrize("ncols", [0, 1, 6, 385])
def test_thin_widths(qa, ctx, ncols):
    """385 columns of 257 tiles: two chunks, so the columns are cut into slices of whole batches and the last slice is ragged."""
    for (r, c) in ((2, 1), (7, 2)):
        b = uniform_batch(qa, ctx, 257, r, c)
        check_panel(b, 1.0, "norms", ncols)


def test_thin_mixed_plan(qa, ctx):
    b = thin_mixed_batch(qa, ctx)
    assert set(b.cols.tolist()) == {1, 2}
    assert b.kernel_name(5) == "qrk::lm::bd_lm_panel_thin_kernel"
    for par in PARS:
        check_panel(b, par, "norms", 5)
        check_panel(b, par, "none", 5)


def test_thin_colidx_and_padding(qa, ctx):
    """A seeded permutation of more source columns than the call takes; leading dimensions 3 above mat_cols with a sentinel behind."""
    for (r, c) in ((2, 1), (7, 2)):
        b = uniform_batch(qa, ctx, 257, r, c)
        idx = np.random.default_rng(9).permutation(11)[:7]
        check_panel(b, 1.0, "norms", 7, colidx=idx, nsrc=11)
        check_panel(b, 1e-3, "none", 6, pad=3)
        check_panel(b, 1e3, "norms", 7, colidx=idx, nsrc=11, pad=3)


# ---- the general kernel: 3 <= c <= 32 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 7, 8, 15, 16, 31, 32])
def test_general_widths_of_tiles(qa, ctx, c):
    b = uniform_batch(qa, ctx, 37, c + 8, c)
    cap = 8 if c <= 8 else (16 if c <= 16 else 32)
    assert b.kernel_name(5) == f"qrk::lm::bd_lm_panel_group_kernel<{cap}>"
    for i, par in enumerate(PARS):
        check_panel(b, par, ("norms", "none")[i % 2], 5, seed=i)
        check_panel(b, par, ("none", "norms")[i % 2], 5, seed=10 + i)


@pytest.mark.parametrize("ncols", [1, 5, 70])
def test_general_widths_of_panel(qa, ctx, ncols):
    for c in (6, 12, 20):
        b = uniform_batch(qa, ctx, 37, c + 8, c)
        check_panel(b, 1.0, "norms", ncols, pad=3)
    idx = np.random.default_rng(5).permutation(ncols + 4)[:ncols]
    check_panel(uniform_batch(qa, ctx, 37, 14, 6), 1e-3, "none", ncols, colidx=idx, nsrc=ncols + 4)


def test_general_mixed_batch(qa, ctx):
    b = mixed_batch(qa, ctx)
    assert b.kernel_name(5) == "qrk::lm::bd_lm_panel_group_kernel<32>"
    for par in PARS:
        check_panel(b, par, "norms", 5)
    check_panel(b, 1.0, "none", 5)


# ---- against qrk_bd_lm_solve ------------------------------------------------------------------------------------------------------------------

def lm_solve_case(b, par, mode):
    """ncols = 1 and c = y: the damped factors and the top of the transformed right-hand side give qrk_bd_lm_solve's x."""
    diag = b.diag if mode == "norms" else None
    st, s, top, _ = b.panel(par, diag, b.y[:, None], 1)
    assert st == 0
    torch = b.torch
    sv = torch.from_numpy(s).to(b.ctx.device)
    z = torch.empty(b.mat_cols, dtype=torch.float64, device=b.ctx.device)
    rhs = torch.from_numpy(np.ascontiguousarray(top[:, 0])).to(b.ctx.device)
    capi = b.qa._capi
    capi.check(capi.lib().qrk_bd_solve_r(b.qr._plan, sv.data_ptr(), rhs.data_ptr(), 1, z.data_ptr(), capi.MEM_DEVICE), b.ctx.handle)
    x = np.empty(b.mat_cols)
    x[b.perm] = z.cpu().numpy()
    want = b.qr.lmSolve(b.y, diag, par)
    worst = max(rel(x[b.perm[int(b.base[t]):int(b.base[t + 1])]], want[b.perm[int(b.base[t]):int(b.base[t + 1])]]) for t in range(len(b.cols)))
    print(f"par {par:g} diag {mode}: x against qrk_bd_lm_solve per tile {worst:.2e}")
    assert worst <= TOL


def test_agrees_with_lm_solve(qa, ctx):
    for b in (uniform_batch(qa, ctx, 257, 2, 1), uniform_batch(qa, ctx, 257, 7, 2), thin_mixed_batch(qa, ctx),
              uniform_batch(qa, ctx, 37, 15, 7), uniform_batch(qa, ctx, 37, 24, 16), uniform_batch(qa, ctx, 37, 40, 32)):
        for par in PARS:
            lm_solve_case(b, par, "norms")
        lm_solve_case(b, 1.0, "none")


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------------

def bit_batches(qa, ctx):
    return (uniform_batch(qa, ctx, 257, 2, 1), uniform_batch(qa, ctx, 257, 7, 2), thin_mixed_batch(qa, ctx),
            uniform_batch(qa, ctx, 37, 15, 7), uniform_batch(qa, ctx, 37, 24, 16), uniform_batch(qa, ctx, 37, 40, 32), mixed_batch(qa, ctx))


def test_par_zero_is_the_identity_bit_for_bit(qa, ctx):
    for b in bit_batches(qa, ctx):
        Cmat = np.random.default_rng(1).standard_normal((b.mat_cols, 9))
        idx = np.array([4, 0, 8, 2, 6], np.int32)
        st, s, top, fill = b.panel(0.0, b.diag, Cmat, 5, colidx=idx)
        assert st == 0
        np.testing.assert_array_equal(s.view(np.int64), b.r.view(np.int64))
        np.testing.assert_array_equal(np.ascontiguousarray(top).view(np.int64), np.ascontiguousarray(Cmat[:, idx]).view(np.int64))
        np.testing.assert_array_equal(np.ascontiguousarray(fill).view(np.int64), np.zeros_like(fill).view(np.int64))


def test_null_diag_is_ones_and_calls_repeat_bit_for_bit(qa, ctx):
    for b in bit_batches(qa, ctx):
        Cmat = np.random.default_rng(2).standard_normal((b.mat_cols, 6))
        first = b.panel(0.5, None, Cmat, 6)
        ones = b.panel(0.5, np.ones(b.mat_cols), Cmat, 6)
        again = b.panel(0.5, None, Cmat, 6)
        for a, o, g in zip(first[1:], ones[1:], again[1:]):
            np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(o).view(np.int64))
            np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(g).view(np.int64))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_unsupported_plans_and_bad_arguments(qa, ctx):
    import torch
    capi = qa._capi
    lib, I = capi.lib(), capi.STATUS_INVALID_ARGUMENT
    # a tile of 33 columns; a BlockDiagonalQ plan: analysed only, the arrays are never read
    for rows, cols, fmt in (([40, 40], [33, 5], FULL_Q), ([7] * 5, [2] * 5, BLOCK_DIAGONAL_Q)):
        rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, np.ones(int((rows * cols).sum())))
        qr = qa.BlockDiagonalSparseQR(blockSolver=0, qFormat=fmt, context=ctx)
        qr.analyzePattern(mat)
        n = int(cols.sum())
        assert "unsupported" in lib.qrk_bd_lm_panel_kernel_name(qr._plan, 2).decode()
        buf = torch.ones(n * 34, dtype=torch.float64, device=ctx.device)
        pm = torch.arange(n, dtype=torch.int32, device=ctx.device)
        st = lib.qrk_bd_lm_panel(qr._plan, buf.data_ptr(), pm.data_ptr(), None, 1.0, buf.data_ptr(), n, 2, None, buf.data_ptr(), buf.data_ptr(),
                                 n, buf.data_ptr(), n)
        assert st == capi.STATUS_UNSUPPORTED
    b = uniform_batch(qa, ctx, 257, 7, 2)
    p, r, pm = b.qr._plan, b.qr._r.data_ptr(), b.qr._perm.data_ptr()
    assert lib.qrk_bd_lm_panel(p, None, pm, None, 1.0, None, 0, 0, None, r, None, 0, None, 0) == I        # r_vals
    assert lib.qrk_bd_lm_panel(p, r, None, None, 1.0, None, 0, 0, None, r, None, 0, None, 0) == I         # perm
    assert lib.qrk_bd_lm_panel(p, r, pm, None, 1.0, None, 0, 0, None, None, None, 0, None, 0) == I        # s_vals
    assert lib.qrk_bd_lm_panel(p, r, pm, None, 1.0, None, b.mat_cols, 2, None, r, None, b.mat_cols, None, b.mat_cols) == I   # panel
    assert lib.qrk_bd_lm_panel(p, r, pm, None, -1.0, None, 0, 0, None, r, None, 0, None, 0) == I          # par < 0
    assert lib.qrk_bd_lm_panel(p, r, pm, None, float("nan"), None, 0, 0, None, r, None, 0, None, 0) == I
    assert lib.qrk_bd_lm_panel(p, r, pm, None, 1.0, None, 0, -1, None, r, None, 0, None, 0) == I          # ncols < 0
