"""GPU: qrk_dense_qless_r -- the R factor of a tall-skinny device matrix without Q, through the raw C ABI.

Bounds: max | R^T R - A^T A | <= 1e-11 max(1, max | A^T A |) and, for rows >= 4 cols, the relative Frobenius distance from numpy's
qr(A, mode="r") with both diagonals made positive <= 1e-11: the project's bound for a kernel against numpy (K11 / K12).  The
stability test plants singular values down to 1e-6 and asks for them back to 1e-9 relative: a Gram matrix + Cholesky gives >= 5e-7
there, a chunked Householder TSQR <= 3.3e-12 (numpy, chunks of 64 / 256 / 1024 rows).

The shapes are the edges of a lane, a slab of 64 rows, a chunk of 256, a second level, and of every column class (8 / 16 / 32), plus
two tall shapes with three levels, one of them with a level-1 chunk of 512 rows.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 5, 63, 64, 65, 255, 256, 257, 1025, 4097]
COLS = [1, 2, 6, 8, 9, 16, 17, 32]
TALL = [(300001, 6), (70001, 32)]
BOUND = 1e-11


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


def levels_of(qa, rows, cols):
    L = qa._capi.lib()
    lr, lc = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    n = L.qrk_dense_qless_r_levels(rows, cols, lr, lc, 8)
    return n, list(lr[:max(n, 0)]), list(lc[:max(n, 0)])


def qless_r(qa, ctx, A, lda, rows, cols, ldr=None, sentinel=7.5):
    """One call on the column-major array A (lda x cols, numpy).  Returns (status, R (cols x cols), the rows of r beyond cols)."""
    import torch
    dev, L = ctx.device, qa._capi.lib()
    ldr = cols if ldr is None else ldr
    dA = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)                 # column j at j * lda
    r = torch.full((max(cols, 1), max(ldr, 1)), sentinel, dtype=torch.float64, device=dev)     # column j at j * ldr
    work = torch.full((int(L.qrk_dense_qless_r_work(rows, cols)),), np.nan, dtype=torch.float64, device=dev)
    ctx.use_current_stream()
    st = L.qrk_dense_qless_r(ctx.handle, dA.data_ptr(), lda, rows, cols, r.data_ptr(), ldr, work.data_ptr())
    torch.cuda.synchronize()
    full = r.cpu().numpy().T                                                 # ldr x cols
    return st, full[:cols, :cols].copy(), full[cols:ldr, :cols].copy()


def positive(R):
    s = np.where(np.diag(R) < 0, -1.0, 1.0)
    return R * s[:, None]


def assert_r(A, R, what, full_rank=True):
    """The assertions every result has to meet; returns (gram error / bound scale, distance from numpy's R or None).  R is compared
    with numpy's only where it is unique up to the signs of its rows: A of full column rank."""
    rows, cols = A.shape
    assert np.all(np.isfinite(R)), what
    low = np.tril(R, -1)
    assert not low.any() and not np.signbit(low).any(), f"{what}: not exact +0.0 below the diagonal"
    G = A.T @ A
    scale = max(1.0, float(np.max(np.abs(G)))) if G.size else 1.0
    gram = float(np.max(np.abs(R.T @ R - G))) / scale if G.size else 0.0
    assert gram <= BOUND, f"{what}: | R^T R - A^T A | = {gram:.2e} of the scale"
    dist = None
    if rows >= 4 * cols and cols > 0 and full_rank:
        want = positive(np.linalg.qr(A, mode="r"))
        dist = float(np.linalg.norm(positive(R) - want) / np.linalg.norm(want))
        assert dist <= BOUND, f"{what}: R differs from numpy's by {dist:.2e}"
    return gram, dist


def check(qa, ctx, rows, cols, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, cols))
    st, R, _ = qless_r(qa, ctx, A, rows, rows, cols)
    assert st == 0
    gram, dist = assert_r(A, R, f"{rows} x {cols}")
    st, again, _ = qless_r(qa, ctx, A, rows, rows, cols)
    assert st == 0 and again.tobytes() == R.tobytes(), "two identical calls gave different bits"
    # lda > rows with NaN below every column; r as a window of a taller array whose extra rows must survive
    lda, ldr = rows + 5, cols + 3
    Ap = np.full((lda, cols), np.nan)
    Ap[:rows] = A
    st, R2, extra = qless_r(qa, ctx, Ap, lda, rows, cols, ldr=ldr, sentinel=-3.25)
    assert st == 0
    assert np.all(np.isfinite(R2)), "the padding below the columns was read"
    assert R2.tobytes() == R.tobytes(), "lda / ldr changed the result"
    assert extra.shape == (3, cols) and np.all(extra == -3.25), "rows of r beyond cols were written"
    return gram, dist


@pytest.mark.parametrize("rows", ROWS)
def test_qless_r_against_numpy(qa, ctx, rows):
    res = [check(qa, ctx, rows, cols, 1000 * rows + cols) for cols in COLS]
    dists = [d for _, d in res if d is not None]
    print(f"rows {rows}: worst gram error {max(g for g, _ in res):.2e}, worst distance from numpy's R "
          f"{max(dists) if dists else float('nan'):.2e} over cols {COLS}")


@pytest.mark.parametrize("shape", TALL)
def test_qless_r_tall_three_levels(qa, ctx, shape):
    rows, cols = shape
    n, lr, lc = levels_of(qa, rows, cols)
    assert n >= 3, (n, lr, lc)
    if shape == TALL[0]:
        assert lc[0] > 256, "the level-1 chunk was meant to grow at this size"
    gram, dist = check(qa, ctx, rows, cols, 77)
    print(f"{rows} x {cols}: levels {lr} in chunks {lc}: gram error {gram:.2e}, distance from numpy's R {dist:.2e}")


def test_qless_r_zeros(qa, ctx):
    rng = np.random.default_rng(5)
    # all zero: exact zeros, no NaN
    st, R, _ = qless_r(qa, ctx, np.zeros((600, 6)), 600, 600, 6)
    assert st == 0 and not R.any() and not np.signbit(R).any()
    # rows = 0
    st, R, _ = qless_r(qa, ctx, np.zeros((0, 6)), 0, 0, 6)
    assert st == 0 and not R.any() and not np.signbit(R).any()
    # the first 300 rows zero (a whole chunk and part of the next)
    A = rng.standard_normal((600, 6))
    A[:300] = 0.0
    st, R, _ = qless_r(qa, ctx, A, 600, 600, 6)
    assert st == 0
    assert_r(A, R, "300 zero rows first")
    # one column exactly zero: that column of R is zero, the rest meets the bound
    for cols, z in ((6, 0), (6, 3), (17, 16), (32, 11)):
        A = rng.standard_normal((600, cols))
        A[:, z] = 0.0
        st, R, _ = qless_r(qa, ctx, A, 600, 600, cols)
        assert st == 0 and not R[:, z].any(), (cols, z)
        assert_r(A, R, f"zero column {z} of {cols}", full_rank=False)
    # fewer rows than columns: the missing rows count as zero
    for rows, cols in ((1, 6), (5, 9), (3, 32), (31, 32)):
        A = rng.standard_normal((rows, cols))
        st, R, _ = qless_r(qa, ctx, A, rows, rows, cols)
        assert st == 0
        assert_r(A, R, f"{rows} x {cols}")


@pytest.mark.parametrize("n", [6, 17, 32])
def test_qless_r_is_stable(qa, ctx, n):
    """Fails for a Gram-matrix shortcut: singular values planted down to 1e-6 come back to 1e-9 relative."""
    worst = 0.0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        U = np.linalg.qr(rng.standard_normal((4097, n)))[0]
        V = np.linalg.qr(rng.standard_normal((n, n)))[0]
        sv = np.logspace(0, -6, n)
        A = (U * sv) @ V.T
        st, R, _ = qless_r(qa, ctx, A, 4097, 4097, n)
        assert st == 0
        got = np.linalg.svd(R, compute_uv=False)
        err = float(np.max(np.abs(got - sv) / sv))
        worst = max(worst, err)
        assert err <= 1e-9, (n, seed, err)
    print(f"n = {n}: planted singular values back to {worst:.2e} relative")


def test_qless_r_refusals_noops_and_names(qa, ctx):
    import torch
    cap, L = qa._capi, qa._capi.lib()
    I, U = cap.STATUS_INVALID_ARGUMENT, cap.STATUS_UNSUPPORTED
    t = torch.full((4096,), 2.5, dtype=torch.float64, device=ctx.device)
    p, h = t.data_ptr(), ctx.handle
    assert L.qrk_dense_qless_r(None, p, 8, 8, 2, p, 2, p) == I          # handle
    assert L.qrk_dense_qless_r(h, None, 8, 8, 2, p, 2, p) == I          # A
    assert L.qrk_dense_qless_r(h, p, 8, 8, 2, None, 2, p) == I          # r
    assert L.qrk_dense_qless_r(h, p, 8, 8, 2, p, 2, None) == I          # work
    assert L.qrk_dense_qless_r(h, p, 7, 8, 2, p, 2, p) == I             # lda < rows
    assert L.qrk_dense_qless_r(h, p, 8, 8, 2, p, 1, p) == I             # ldr < cols
    assert L.qrk_dense_qless_r(h, p, 8, -1, 2, p, 2, p) == I            # rows < 0
    assert L.qrk_dense_qless_r(h, p, 8, 8, -1, p, 2, p) == I            # cols < 0
    assert L.qrk_dense_qless_r(h, p, 64, 64, 33, p, 33, p) == U         # cols > 32
    assert L.qrk_dense_qless_r(h, None, 8, 8, 0, None, 0, None) == 0    # cols = 0: nothing to do
    torch.cuda.synchronize()
    assert bool(torch.all(t == 2.5)), "a refused call or a no-op wrote something"
    for cols, nc in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32)):
        assert L.qrk_dense_qless_r_kernel_name(1000, cols) == f"qrk::qless::dense_qless_r_kernel<{nc}>".encode()
    assert b"unsupported" in L.qrk_dense_qless_r_kernel_name(1000, 33)
    assert L.qrk_dense_qless_r_kernel_name(-1, 3) == b""


@contextlib.contextmanager
def capture(graph):
    """What `with torch.cuda.graph(graph):` does -- capture_begin() / capture_end() on a side stream that joins the current one --
    without its torch.cuda.empty_cache() (as tests/test_lmpar_device_gpu.py captures)."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            yield
        finally:
            graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)


def test_qless_r_can_be_captured(qa, ctx):
    """One stream, no branches: captured once, replayed after A was overwritten, equal to an eager call's bytes."""
    import torch
    dev, L = ctx.device, qa._capi.lib()
    rows, cols = 4097, 9
    rng = np.random.default_rng(11)
    A1, A2 = rng.standard_normal((rows, cols)), rng.standard_normal((rows, cols))
    st, want, _ = qless_r(qa, ctx, A2, rows, rows, cols)
    assert st == 0
    dA = torch.from_numpy(np.ascontiguousarray(A1.T)).to(dev)
    r = torch.zeros(cols, cols, dtype=torch.float64, device=dev)
    work = torch.empty(int(L.qrk_dense_qless_r_work(rows, cols)), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        ctx.use_current_stream()
        st = L.qrk_dense_qless_r(ctx.handle, dA.data_ptr(), rows, rows, cols, r.data_ptr(), cols, work.data_ptr())
    ctx.use_current_stream()
    assert st == 0
    dA.copy_(torch.from_numpy(np.ascontiguousarray(A2.T)))
    r.fill_(np.nan)
    graph.replay()
    torch.cuda.synchronize()
    got = r.cpu().numpy().T.copy()
    assert got.tobytes() == want.tobytes()
    assert_r(A2, got, "replayed")
