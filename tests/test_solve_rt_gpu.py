"""GPU: qrk_bd_solve_rt alone -- w_t = R_t^-T u_t tile by tile with its two sums.

The judge is numpy per tile (numpy.linalg.solve on the transposed triangle) on the device's own packed arrays.  Fed with the damped
factors s_vals of qrk_bd_lm_panel at par = 1, diag = ones (S^T S = R^T R + I: well conditioned) the bound is 1e-11 per tile; fed with
r_vals themselves on the tall shapes 7 x 2 and 8 x 6 it is 1e-9 -- the pair of bounds of tests/test_lm_solve_gpu.py.  || w ||^2 is
judged at 1e-9 relative.  The worst seen is printed.
"""
import functools

import numpy as np
import pytest

import lm_panel_reference as judge
from helpers import seeded_tiles

pytestmark = pytest.mark.gpu

FULL_Q, BLOCK_DIAGONAL_Q = 0, 1


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


class Batch:
    """One factorised batch and its damped factors at par = 1, diag = ones, as the device holds them."""

    def __init__(self, qa, ctx, rows, cols, tiles, seed, q_format=FULL_Q):
        import torch
        self.qa, self.ctx, self.torch = qa, ctx, torch
        self.rows, self.cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
        self.mat_rows, self.mat_cols = int(self.rows.sum()), int(self.cols.sum())
        self.nnz_r = int((self.cols.astype(np.int64) * (self.cols + 1) // 2).sum())
        self.base = np.concatenate([[0], np.cumsum(self.cols)]).astype(np.int64)
        mat = qa.SparseBlockDiagonal.fromTiles(self.rows, self.cols, tiles, rows=self.mat_rows)
        self.qr = qa.BlockDiagonalSparseQR(blockSolver=0, qFormat=q_format, context=ctx)
        self.qr.compute(mat)
        assert self.qr.info() == 0
        self.u = np.random.default_rng(3000 + seed).standard_normal(self.mat_cols)
        self.s_dev = None
        if q_format == FULL_Q and int(self.cols.max()) <= 32:
            self.s_dev = torch.empty(max(self.nnz_r, 1), dtype=torch.float64, device=ctx.device)
            ctx.use_current_stream()
            st = qa._capi.lib().qrk_bd_lm_panel(self.qr._plan, self.qr._r.data_ptr(), self.qr._perm.data_ptr(), None, 1.0, None, 0, 0, None,
                                                self.s_dev.data_ptr(), None, 0, None, 0)
            assert st == 0

    def solve_rt(self, vals_dev, u=None, sums=True):
        """(status, w, sums2) of one call on the packed device array vals_dev"""
        torch, dev = self.torch, self.ctx.device
        du = torch.from_numpy(np.ascontiguousarray(self.u if u is None else u)).to(dev)
        w = torch.full((max(self.mat_cols, 1),), -7.25, dtype=torch.float64, device=dev)
        s2 = torch.full((2,), -7.25, dtype=torch.float64, device=dev)
        self.ctx.use_current_stream()
        st = self.qa._capi.lib().qrk_bd_solve_rt(self.qr._plan, vals_dev.data_ptr(), du.data_ptr(), w.data_ptr(), s2.data_ptr() if sums else None)
        torch.cuda.synchronize()
        return st, w.cpu().numpy()[:self.mat_cols], s2.cpu().numpy()

    def kernel_name(self):
        return self.qa._capi.lib().qrk_bd_solve_rt_kernel_name(self.qr._plan).decode()


def gaussian_batch(qa, ctx, rows, cols, seed, q_format=FULL_Q):
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    n = int((rows.astype(np.int64) * cols).sum())
    return Batch(qa, ctx, rows, cols, np.random.default_rng(seed).standard_normal(n), seed, q_format)


@functools.lru_cache(maxsize=None)
def uniform_batch(qa, ctx, B, r, c):
    return gaussian_batch(qa, ctx, np.full(B, r), np.full(B, c), 100 * r + c + B)


@functools.lru_cache(maxsize=None)
def thin_mixed_batch(qa, ctx, B):
    cols = np.random.default_rng(3 + B).integers(1, 3, B)
    return gaussian_batch(qa, ctx, cols + 4, cols, 31 + B)


@functools.lru_cache(maxsize=None)
def mixed_batch(qa, ctx):
    rng = np.random.default_rng(7)                           # the 400-tile mixed batch of tests/test_lm_solve_gpu.py
    B = 400
    cols = rng.integers(1, 33, B).astype(np.int32)
    rows = (cols + rng.integers(0, 6, B)).clip(max=32).astype(np.int32)
    tiles = seeded_tiles(11, -1.0, 1.0, int((rows.astype(np.int64) * cols).sum()))
    return Batch(qa, ctx, rows, cols, tiles, 7)


def check(b, vals_dev, tol, what):
    """One call on vals_dev against numpy per tile; returns (worst per-tile error, error of the sum)."""
    vals = vals_dev.cpu().numpy()[:b.nnz_r]
    st, w, s2 = b.solve_rt(vals_dev)
    assert st == 0
    worst, total = 0.0, 0.0
    for t, T in enumerate(judge.unpack_tiles(b.cols, vals)):
        lo, hi = int(b.base[t]), int(b.base[t + 1])
        want = np.linalg.solve(T.T, b.u[lo:hi])
        worst = max(worst, np.linalg.norm(w[lo:hi] - want) / np.linalg.norm(want))
        total += float(want @ want)
    esum = abs(s2[0] - total) / total
    print(f"{what}: {len(b.cols)} tiles, widest {int(b.cols.max())}: per tile {worst:.2e}, |w|^2 {esum:.2e}, kernel {b.kernel_name()}")
    assert worst <= tol and esum <= 1e-9 and s2[1] == 0.0
    # repeatable to the bit, with and without the sums
    st, w2, s22 = b.solve_rt(vals_dev)
    assert st == 0 and w2.tobytes() == w.tobytes() and s22.tobytes() == s2.tobytes()
    st, w3, s23 = b.solve_rt(vals_dev, sums=False)
    assert st == 0 and w3.tobytes() == w.tobytes() and np.all(s23 == -7.25)
    return worst, esum


@pytest.mark.parametrize("B", [1, 257, 1024])
@pytest.mark.parametrize("c", [1, 2, "mixed"])
def test_thin_tiles_on_damped_factors(qa, ctx, c, B):
    b = thin_mixed_batch(qa, ctx, B) if c == "mixed" else uniform_batch(qa, ctx, B, c + 4, c)
    assert b.kernel_name() == "qrk::lm::bd_solve_rt_thin_kernel"
    check(b, b.s_dev, 1e-11, f"thin c = {c}, B = {B}")


@pytest.mark.parametrize("c", list(range(3, 33)))
def test_group_tiles_on_damped_factors(qa, ctx, c):
    b = uniform_batch(qa, ctx, 37, min(c + 3, 32), c)
    assert b.kernel_name() == "qrk::lm::bd_solve_rt_group_kernel"
    check(b, b.s_dev, 1e-11, f"group c = {c}, B = 37")


def test_mixed_batch_on_damped_factors(qa, ctx):
    b = mixed_batch(qa, ctx)
    assert b.kernel_name() == "qrk::lm::bd_solve_rt_group_kernel"
    check(b, b.s_dev, 1e-11, "mixed batch of 400")


@pytest.mark.parametrize("shape", [(7, 2), (8, 6)])
def test_undamped_factors_of_tall_tiles(qa, ctx, shape):
    b = uniform_batch(qa, ctx, 300, *shape)
    check(b, b.qr._r, 1e-9, f"r_vals of 300 x ({shape[0]} x {shape[1]})")


@pytest.mark.parametrize("shape", [(6, 1), (7, 2), (8, 6), (32, 32)])
def test_a_planted_zero_diagonal(qa, ctx, shape):
    """A tile with an exact zero on the diagonal gets w_t = 0, counts once in sums2[1] and adds nothing to sums2[0]."""
    r, c = shape
    b = uniform_batch(qa, ctx, 37, r, c)
    vals = b.s_dev.clone()
    per = c * (c + 1) // 2
    t, k = 20, c - 1
    vals[t * per + k * (k + 1) // 2 + k] = 0.0
    st, w, s2 = b.solve_rt(vals)
    assert st == 0 and s2[1] == 1.0
    assert np.all(w[t * c:(t + 1) * c] == 0.0)
    st, w0, s20 = b.solve_rt(b.s_dev)
    keep = np.ones(b.mat_cols, bool); keep[t * c:(t + 1) * c] = False
    assert w[keep].tobytes() == w0[keep].tobytes()
    assert np.isfinite(s2[0]) and abs(s2[0] - np.sum(w0[keep] ** 2)) <= 1e-9 * s2[0]


def test_unsupported_plans_are_refused(qa, ctx):
    U = qa._capi.STATUS_UNSUPPORTED
    wide = gaussian_batch(qa, ctx, [40, 8], [33, 4], 5)
    assert "unsupported" in wide.kernel_name()
    assert wide.solve_rt(wide.qr._r)[0] == U
    bdq = gaussian_batch(qa, ctx, np.full(5, 7), np.full(5, 2), 6, q_format=BLOCK_DIAGONAL_Q)
    assert "unsupported" in bdq.kernel_name()
    assert bdq.solve_rt(bdq.qr._r)[0] == U
