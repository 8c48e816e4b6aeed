"""GPU: the entry points of the block-angular lmpar (qrk_bd_solve_rt, qrk_dense_gemv_t, qrk_dense_solve_rt, qrk_dense_trmv_t;
DESIGN.md K12) with EVERY caller-owned array, gemv_t's workspace included, at exactly its documented extent between NaN guard bands
(tests/guarded.py), at shift 0 and shift 1, as tests/test_guarded_gpu.py does for the other calls -- whose batches, plans and
Levenberg-Marquardt inputs (the oracle's well-conditioned R of every tile class) this file uses.  Values are judged by numpy at the
bounds of the stand-alone tests of each call."""
import numpy as np
import pytest
import scipy.linalg as sl

import lm_panel_reference as panel_judge
import test_guarded_gpu as gg
from guarded import Net
from helpers import rel_fro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.mark.parametrize("case", gg.LM, ids=gg.ids_of(gg.LM))
def test_bd_solve_rt(qa, monkeypatch, case):
    label, kind, r, c, _, _ = case
    ctx = gg.context_for(qa, monkeypatch, {})
    L = qa._capi.lib()
    for B in gg.batch_sizes(kind, r):
        ref = gg.ref_for(kind, r, c, B, gg.extra_rows(kind, B), gg.FULL_Q, 0)
        u = ref.rng(91).uniform(-1.0, 1.0, ref.mat_cols)
        base = np.concatenate([[0], np.cumsum(ref.cols)]).astype(np.int64)
        want = np.concatenate([np.linalg.solve(R.T, u[base[t]:base[t + 1]])
                               for t, R in enumerate(panel_judge.unpack_tiles(ref.cols, ref.r_vals))])
        with gg.bd_plan(ctx, ref) as plan:
            name = L.qrk_bd_solve_rt_kernel_name(plan).decode()
            assert name == ("qrk::lm::bd_solve_rt_thin_kernel" if int(ref.cols.max()) <= 2 else "qrk::lm::bd_solve_rt_group_kernel")
            for with_sums in (True, False):
                runs = []
                for shift in gg.SHIFTS:
                    net = Net(ctx.device, shift)
                    rv, uu = net.inp("r_vals", ref.r_vals), net.inp("u", u)
                    w = net.out("w", ref.mat_cols)
                    s2 = net.out("sums2", 2) if with_sums else None
                    gg.ok(ctx, L.qrk_bd_solve_rt(plan, rv.ptr, uu.ptr, w.ptr, gg.ptr(s2)))
                    gg.sync()
                    net.check()
                    got = w.get()
                    worst = max(np.linalg.norm(got[base[t]:base[t + 1]] - want[base[t]:base[t + 1]]) / np.linalg.norm(want[base[t]:base[t + 1]])
                                for t in range(len(ref.cols)))
                    print(f"{label} B {B} sums {with_sums} shift {shift}: per tile {worst:.2e}")
                    assert worst <= gg.LM_TOL
                    if with_sums:
                        s = s2.get()
                        assert abs(s[0] - want @ want) <= 1e-9 * (want @ want) and s[1] == 0.0
                    runs.append([got] + ([s2.get()] if with_sums else []))
                assert gg.same_bits(*runs), "shift 0 and shift 1 differ"


@pytest.mark.parametrize("rows,cols", [(0, 3), (40, 7), (300, 40), (641, 9)])
def test_dense_gemv_t(qa, monkeypatch, rows, cols):
    """A on a window with lda > rows (the rows between are guards), w, colidx, add, out and the workspace at
    qrk_dense_gemv_t_work(rows, cols) doubles -- all of which the call writes at these sizes (chunks of 256 rows)."""
    ctx = gg.context_for(qa, monkeypatch, {})
    ctx.use_current_stream()
    L = qa._capi.lib()
    rng = np.random.default_rng(rows + cols)
    lda = (rows + 3) | 1
    w = rng.uniform(-1.0, 1.0, rows)
    nwork = int(L.qrk_dense_gemv_t_work(rows, cols))
    used = -(-rows // 256) * cols
    assert nwork >= used
    for with_opt in (False, True):
        nsrc = cols + 2 if with_opt else cols
        A = rng.uniform(-1.0, 1.0, (rows, nsrc))
        colidx = (rng.permutation(nsrc)[:cols] if with_opt else np.arange(cols)).astype(np.int32)
        add = rng.uniform(-1.0, 1.0, cols)
        alpha = -1.0 if with_opt else 1.0
        want = alpha * (A[:, colidx].T @ w) + (add if with_opt else 0.0)
        bound = rows * 2.0 ** -52 * (np.abs(A[:, colidx]).T @ np.abs(w))
        runs = []
        for shift in gg.SHIFTS:
            net = Net(ctx.device, shift)
            a, ww = net.panel_in("A", A, lda), net.inp("w", w)
            ci = net.inp("colidx", colidx, dtype=gg._i32()) if with_opt else None
            ad = net.inp("add", add) if with_opt else None
            out = net.out("out", cols)
            work = net.out("work", nwork, untouched=np.arange(nwork) >= used)
            gg.ok(ctx, L.qrk_dense_gemv_t(ctx.handle, a.ptr, lda, rows, cols, gg.ptr(ci), ww.ptr, alpha, gg.ptr(ad), out.ptr, work.ptr))
            gg.sync()
            net.check()
            assert np.all(np.abs(out.get() - want) <= bound)
            runs.append([out.get()])
        assert gg.same_bits(*runs), "shift 0 and shift 1 differ"


@pytest.mark.parametrize("n", [0, 1, 7, 65, 130])
def test_dense_solve_rt_and_trmv_t(qa, monkeypatch, n):
    """qr on a window with lda > n and NaN below the diagonal; b is updated in place, out accumulates."""
    ctx = gg.context_for(qa, monkeypatch, {})
    ctx.use_current_stream()
    L = qa._capi.lib()
    rng = np.random.default_rng(n)
    R = np.triu(rng.standard_normal((n, n)), 1) * (0.5 / np.sqrt(max(n, 1)))
    R[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n)
    qr = np.where(np.tri(n, k=-1, dtype=bool), np.nan, R)
    b, y, out0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    lda = n + 3
    runs = []
    for shift in gg.SHIFTS:
        net = Net(ctx.device, shift)
        a = net.panel_in("qr", qr, lda)
        bb, yy, oo = net.inp("b", b, role="inout"), net.inp("y", y), net.inp("out", out0, role="inout")
        gg.ok(ctx, L.qrk_dense_solve_rt(ctx.handle, a.ptr, lda, n, bb.ptr))
        gg.ok(ctx, L.qrk_dense_trmv_t(ctx.handle, a.ptr, lda, n, yy.ptr, oo.ptr))
        gg.sync()
        net.check()
        if n:
            assert rel_fro(bb.get(), sl.solve_triangular(R, b, trans="T", lower=False)) <= 1e-11
            assert rel_fro(oo.get(), out0 + R.T @ y) <= 1e-11
        runs.append([bb.get(), oo.get()])
    assert gg.same_bits(*runs), "shift 0 and shift 1 differ"
