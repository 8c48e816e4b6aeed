"""GPU: qrk_dense_solve_rt (b <- R^-T b) and qrk_dense_trmv_t (out += R^T y) on the upper triangle of a packed QR.

Everything below the diagonal is NaN: a packed QR keeps reflectors there and neither call may read them.  The triangles are built
well conditioned (diagonal entries of modulus 1 .. 2 next to an off-diagonal part of norm about 1/2), and the test first asserts on
the CPU that numpy's float64 solve agrees with a longdouble forward substitution to 1e-13, so that the bound rel_fro <= 1e-11
against scipy.linalg.solve_triangular(trans='T') and the triangular product judges the kernel and not the problem.
"""
import numpy as np
import pytest
import scipy.linalg

from helpers import rel_fro

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 5, 64, 65, 257]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


def triangle(n, seed):
    rng = np.random.default_rng(seed)
    R = np.triu(rng.standard_normal((n, n)), 1) * (0.5 / np.sqrt(max(n, 1)))
    R[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n)
    return R, rng.standard_normal(n), rng.standard_normal(n)


def longdouble_solve_t(R, b):
    """R^T w = b by forward substitution in longdouble"""
    n = len(b)
    Rl, w = R.astype(np.longdouble), np.zeros(n, np.longdouble)
    for j in range(n):
        w[j] = (np.longdouble(b[j]) - Rl[:j, j] @ w[:j]) / Rl[j, j]
    return w


def packed(R, lda):
    """R's upper triangle in an lda x n column-major array with NaN everywhere else"""
    n = R.shape[0]
    A = np.full((lda, n), np.nan)
    iu = np.triu_indices(n)
    A[iu] = R[iu]
    return A


@pytest.mark.parametrize("n", SIZES)
def test_solve_rt_and_trmv_t(qa, ctx, n):
    import torch
    dev, L = ctx.device, qa._capi.lib()
    R, b, y = triangle(n, 50 + n)
    want = scipy.linalg.solve_triangular(R, b, trans="T", lower=False) if n else np.zeros(0)
    if n:
        exact = longdouble_solve_t(R, b)
        agree = float(np.linalg.norm(want - exact) / np.linalg.norm(exact))
        assert agree <= 1e-13, f"the problem itself is too ill conditioned for the bound: {agree:.2e}"
    for lda in (n, n + 3):
        dA = torch.from_numpy(np.ascontiguousarray(packed(R, lda).T)).to(dev)
        db = torch.full((n + 2,), -7.25, dtype=torch.float64, device=dev)
        db[:n] = torch.from_numpy(b).to(dev)
        ctx.use_current_stream()
        assert L.qrk_dense_solve_rt(ctx.handle, dA.data_ptr(), lda, n, db.data_ptr()) == 0
        torch.cuda.synchronize()
        got = db.cpu().numpy()
        assert np.all(got[n:] == -7.25)
        out0 = np.random.default_rng(n).standard_normal(n)
        dy = torch.from_numpy(y).to(dev)
        do = torch.full((n + 2,), -7.25, dtype=torch.float64, device=dev)
        do[:n] = torch.from_numpy(out0).to(dev)
        assert L.qrk_dense_trmv_t(ctx.handle, dA.data_ptr(), lda, n, dy.data_ptr(), do.data_ptr()) == 0
        torch.cuda.synchronize()
        prod = do.cpu().numpy()
        assert np.all(prod[n:] == -7.25)
        if n:
            e1, e2 = rel_fro(got[:n], want), rel_fro(prod[:n], out0 + np.triu(R).T @ y)
            print(f"n {n} lda {lda}: solve_rt {e1:.2e}  trmv_t {e2:.2e}")
            assert np.all(np.isfinite(got[:n])) and np.all(np.isfinite(prod[:n])), "something below the diagonal was read"
            assert e1 <= 1e-11 and e2 <= 1e-11
            # repeatable to the bit
            db2 = torch.from_numpy(b).to(dev)
            assert L.qrk_dense_solve_rt(ctx.handle, dA.data_ptr(), lda, n, db2.data_ptr()) == 0
            torch.cuda.synchronize()
            assert db2.cpu().numpy().tobytes() == got[:n].tobytes()


def test_refusals(qa, ctx):
    import torch
    I, L = qa._capi.STATUS_INVALID_ARGUMENT, qa._capi.lib()
    p = torch.zeros(16, dtype=torch.float64, device=ctx.device).data_ptr()
    assert L.qrk_dense_solve_rt(ctx.handle, p, 2, 3, p) == I             # lda < n
    assert L.qrk_dense_solve_rt(ctx.handle, None, 3, 3, p) == I
    assert L.qrk_dense_solve_rt(ctx.handle, p, 3, -1, p) == I
    assert L.qrk_dense_trmv_t(ctx.handle, p, 2, 3, p, p) == I
    assert L.qrk_dense_trmv_t(ctx.handle, p, 3, 3, None, p) == I
    assert L.qrk_dense_trmv_t(ctx.handle, p, 3, 3, p, None) == I
