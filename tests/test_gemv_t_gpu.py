"""GPU: qrk_dense_gemv_t -- out[j] = alpha sum_i A(i, colidx[j]) w[i] + add[j], the deterministic tall-skinny A^T w.

The bound per column is | got - want | <= rows 2^-52 sum_i | A_ij w_i | against numpy's float64 product: the summation bound of
both sides (rows terms each, in whatever order), nothing measured.  The shapes are the edges of a lane, a wavefront, a workgroup's
chunk of rows (256 at these sizes) and its batch of 8 columns, plus two tall single-column shapes at which the kernel's chunk grows
(512 rows from 262 145 row-slices on, capped at 4 096).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
COLS = [1, 5, 6, 7, 8, 9, 70, 385]
TALL = [(300001, 5), (4096 * 1024 + 257, 1)]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


def gemv_t(qa, ctx, A, lda, rows, cols, colidx, w, alpha, add):
    """One call on the column-major array A (lda x source columns, numpy); returns (status, out)."""
    import torch
    dev, L = ctx.device, qa._capi.lib()
    dA = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)                 # column j at j * lda
    dw = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    di = torch.from_numpy(np.ascontiguousarray(colidx, dtype=np.int32)).to(dev) if colidx is not None else None
    da = torch.from_numpy(np.ascontiguousarray(add)).to(dev) if add is not None else None
    out = torch.full((max(cols, 1),), np.nan, dtype=torch.float64, device=dev)
    work = torch.full((int(L.qrk_dense_gemv_t_work(rows, cols)),), np.nan, dtype=torch.float64, device=dev)
    ctx.use_current_stream()
    st = L.qrk_dense_gemv_t(ctx.handle, dA.data_ptr(), lda, rows, cols, di.data_ptr() if di is not None else None, dw.data_ptr(),
                            float(alpha), da.data_ptr() if da is not None else None, out.data_ptr(), work.data_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy()[:cols]


def check(qa, ctx, rows, cols, seed):
    rng = np.random.default_rng(seed)
    worst = 0.0
    # plain: every column in place, lda = rows, alpha = +1, nothing added
    A = rng.standard_normal((rows, cols))
    w = rng.standard_normal(rows)
    st, got = gemv_t(qa, ctx, A, max(rows, 1) if rows else 0, rows, cols, None, w, 1.0, None)
    assert st == 0
    want, bound = A.T @ w, rows * 2.0 ** -52 * (np.abs(A).T @ np.abs(w))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound), (rows, cols, np.max(np.abs(got - want) - bound))
    if rows:
        worst = max(worst, float(np.max(np.abs(got - want) / bound)))
    st, again = gemv_t(qa, ctx, A, max(rows, 1) if rows else 0, rows, cols, None, w, 1.0, None)
    assert st == 0 and again.tobytes() == got.tobytes()
    # permuted columns out of a wider matrix, lda > rows with NaN below every column, alpha = -1, a vector added
    src, lda = cols + 3, rows + 5
    A = np.full((lda, src), np.nan)
    A[:rows] = rng.standard_normal((rows, src))
    idx = rng.permutation(src)[:cols]
    add = rng.standard_normal(cols)
    st, got = gemv_t(qa, ctx, A, lda, rows, cols, idx, w, -1.0, add)
    assert st == 0
    Asel = A[:rows][:, idx]
    want, bound = -(Asel.T @ w) + add, rows * 2.0 ** -52 * (np.abs(Asel).T @ np.abs(w))
    assert np.all(np.isfinite(got)), "the padding below the columns was read"
    assert np.all(np.abs(got - want) <= bound), (rows, cols, np.max(np.abs(got - want) - bound))
    if rows:
        worst = max(worst, float(np.max(np.abs(got - want) / bound)))
    st, again = gemv_t(qa, ctx, A, lda, rows, cols, idx, w, -1.0, add)
    assert st == 0 and again.tobytes() == got.tobytes()
    # the two options on their own: alpha = -1 without add, alpha = +1 with add
    st, neg = gemv_t(qa, ctx, A, lda, rows, cols, idx, w, -1.0, None)
    st2, pos = gemv_t(qa, ctx, A, lda, rows, cols, idx, w, 1.0, add)
    assert st == 0 and st2 == 0 and np.all(np.abs(neg + Asel.T @ w) <= bound) and np.all(np.abs(pos - (Asel.T @ w + add)) <= bound)
    return worst


@pytest.mark.parametrize("rows", ROWS)
def test_gemv_t_against_numpy(qa, ctx, rows):
    worst = max(check(qa, ctx, rows, cols, 1000 * rows + cols) for cols in COLS)
    print(f"rows {rows}: worst error over cols {COLS}: {worst:.2e} of the bound")


@pytest.mark.parametrize("shape", TALL)
def test_gemv_t_tall(qa, ctx, shape):
    worst = check(qa, ctx, shape[0], shape[1], 77)
    print(f"{shape[0]} x {shape[1]}: worst error {worst:.2e} of the bound")


def test_gemv_t_refuses_bad_arguments(qa, ctx):
    import torch
    I, L = qa._capi.STATUS_INVALID_ARGUMENT, qa._capi.lib()
    t = torch.zeros(64, dtype=torch.float64, device=ctx.device)
    p = t.data_ptr()
    assert L.qrk_dense_gemv_t(ctx.handle, p, 3, 4, 2, None, p, 1.0, None, p, p) == I          # lda < rows
    assert L.qrk_dense_gemv_t(ctx.handle, p, 4, 4, 2, None, p, 2.0, None, p, p) == I          # alpha
    assert L.qrk_dense_gemv_t(ctx.handle, p, 4, 4, 2, None, p, 1.0, None, None, p) == I       # out
    assert L.qrk_dense_gemv_t(ctx.handle, p, 4, 4, 2, None, p, 1.0, None, p, None) == I       # work
    assert L.qrk_dense_gemv_t(ctx.handle, None, 4, 4, 2, None, p, 1.0, None, p, p) == I       # A
    assert L.qrk_dense_gemv_t(ctx.handle, None, 0, 0, 0, None, None, 1.0, None, None, None) == 0     # nothing to do
