"""GPU: qrk_dense_qless_r with A, r and the workspace at exactly their documented extents between NaN guard bands
(tests/guarded.py), payload aligned (shift 0) and 8 bytes off (shift 1), as tests/test_guarded_angular_lmpar_gpu.py does for
qrk_dense_gemv_t and its workspace.  A is a window with lda > rows and r a window with ldr > cols, so the rows between are guards too;
the workspace has qrk_dense_qless_r_work(rows, cols) doubles, every one of which the call writes once there is a second level.
One shape per column class (8 / 16 / 32), one with a single level, one with fewer rows than columns and one with three levels."""
import ctypes as C

import numpy as np
import pytest

import test_guarded_gpu as gg
from guarded import Net

pytestmark = pytest.mark.gpu

SHAPES = [(0, 3), (5, 9), (200, 6), (700, 6), (641, 13), (1025, 32), (70001, 32)]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_dense_qless_r(qa, monkeypatch, rows, cols):
    ctx = gg.context_for(qa, monkeypatch, {})
    ctx.use_current_stream()
    L = qa._capi.lib()
    rng = np.random.default_rng(rows + cols)
    A = rng.uniform(-1.0, 1.0, (rows, cols))
    lda, ldr = (rows + 3) | 1, cols + 3
    lr = (C.c_int64 * 4)()
    levels = L.qrk_dense_qless_r_levels(rows, cols, lr, None, 4)
    nwork = int(L.qrk_dense_qless_r_work(rows, cols))
    used = (lr[1] * cols if levels >= 2 else 0) + (lr[2] * cols if levels >= 3 else 0)
    assert nwork == max(used, 1) and levels == {70001: 3, 1025: 2, 700: 2, 641: 2}.get(rows, 1)
    G = A.T @ A
    runs = []
    for shift in gg.SHIFTS:
        net = Net(ctx.device, shift)
        a = net.panel_in("A", A, lda)
        r = net.panel_out("r", cols, cols, ldr)
        work = net.out("work", nwork, untouched=np.arange(nwork) >= used)
        gg.ok(ctx, L.qrk_dense_qless_r(ctx.handle, a.ptr, lda, rows, cols, r.ptr, ldr, work.ptr))
        gg.sync()
        net.check()
        R = r.get()
        assert np.all(np.isfinite(R)) and not np.tril(R, -1).any()
        assert np.max(np.abs(R.T @ R - G)) <= 1e-11 * max(1.0, np.max(np.abs(G)))
        runs.append([R])
    assert gg.same_bits(*runs), "shift 0 and shift 1 differ"
