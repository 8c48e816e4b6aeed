"""GPU: the device-side lmpar (qrk_bd_lmpar_device; BlockDiagonalSparseQR.lmparDevice) -- MINPACK's lmpar as one enqueue, its scalar
steps run by one lane behind the sums of every evaluation -- against the host loop (qrk_bd_lmpar) and the numpy judge of
lm_reference.py.

Both loops apply the same handful of correctly rounded scalar operations to sums that come from the same kernels on the same grid:
iters is equal, par and every traced (par, s0, s1) agree to 1e-12 (the margin only covers a differing contraction in the host
compile; whether the bits were identical is printed).  Against the judge the tolerances are those of test_lmpar_gpu.py: par 1e-9,
the traced sums 1e-9 at the traced par, x per tile 1e-11 on (0.5, 5.0) data and 1e-9 on (-1, 1) data at the returned par,
| || D x || - delta | <= 0.1 delta.  One batch per solve kernel, each with more than one workgroup; then one workgroup, the capped
grid, start values, values only the device can refuse, determinism, a graph capture (torch.cuda.CUDAGraph) replayed with new radii, and the
trust-region fit of test_lmpar_gpu.py with one read-back per trial step.
"""
import contextlib
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import lm_reference as judge
from helpers import seeded_tiles

pytestmark = pytest.mark.gpu

# kernel, tiles, rows, cols, data range, x tolerance per tile
CASES = [("bd_lm_thin_kernel", 600, 7, 2, 0.5, 5.0, 1e-11), ("bd_lm_group_kernel<8>", 300, 8, 6, -1.0, 1.0, 1e-9),
         ("bd_lm_group_kernel<16>", 100, 16, 12, -1.0, 1.0, 1e-9), ("bd_lm_group_kernel<32>", 40, 32, 20, -1.0, 1.0, 1e-9),
         ("bd_lm_group_kernel<64>", 20, 32, 32, -1.0, 1.0, 1e-9)]
FACTORS = [2.0, 0.5, 0.1, 0.01]


@pytest.fixture(scope="module")
def qa():
    import qrkit_amd
    return qrkit_amd


@pytest.fixture(scope="module")
def ctx(qa):
    return qa.Context(0)


class Problem:
    """test_lmpar_gpu.Problem: a uniform batch factorised on the Q-less route, with the judge's view of the same factors"""

    def __init__(self, qa, ctx, B, r, c, lo, hi):
        rows, self.cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, self.cols, seeded_tiles(1 + r + c, lo, hi, B * r * c))
        self.qr = qa.BlockDiagonalSparseQR(context=ctx)
        f = np.random.default_rng(10 * r + c).uniform(-1.0, 1.0, B * r)
        self.x0, self.qtb = self.qr.computeAndSolve(mat, f, returnQtB=True)
        self.t = judge.Tiles(self.cols, self.qr.rValues().cpu().numpy(), self.qr.colsPermutation(), self.qtb)
        norms = self.qr.colNorms()
        self.diag = np.where(norms == 0.0, 1.0, norms)
        self.dx0 = float(np.linalg.norm(self.diag * judge.solve(self.t, self.diag, 0.0)[0]))


class MixedProblem:
    """the 400-tile mixed batch of test_lm_solve_gpu.py (1 .. 32 columns, (-1, 1) data), diag = its column norms"""

    def __init__(self, qa, ctx):
        import test_lm_solve_gpu as solve_tests
        b = solve_tests.mixed_batch(qa, ctx)
        self.qr, self.qtb, self.t, self.diag = b.qr, b.y, b.t, b.diag
        self.dx0 = float(np.linalg.norm(self.diag * judge.solve(self.t, self.diag, 0.0)[0]))


@functools.lru_cache(maxsize=None)
def problem(qa, ctx, B, r, c, lo, hi):
    return Problem(qa, ctx, B, r, c, lo, hi)


@functools.lru_cache(maxsize=None)
def mixed_problem(qa, ctx):
    return MixedProblem(qa, ctx)


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@contextlib.contextmanager
def capture(graph):
    """What `with torch.cuda.graph(graph):` does -- capture_begin() / capture_end() on a side stream that joins the current one --
    without its torch.cuda.empty_cache(): handing the allocator's cached segments back in the middle of the suite changes where the
    tensors of every later test land."""
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


@pytest.fixture(scope="module", autouse=True)
def release_the_batches():
    """The cached batches (one of 10^6 tiles) go back to the allocator when the module is done."""
    yield
    for cached in (problem, mixed_problem, plain):
        cached.cache_clear()
    gc.collect()


def device_lmpar(qr, qtb, diag, delta, par=0.0):
    """(par, x, iters, trace) of lmparDevice on the host: trace cut to the evaluations that ran, after checking the rest is zero"""
    pv, x, it, trace = qr.lmparDevice(qtb, diag, delta, par, returnTrace=True)
    assert pv.is_cuda and x.is_cuda and it.is_cuda and trace.is_cuda and trace.shape == (11, 3)
    pv, x, it, trace = pv.item(), x.cpu().numpy(), int(it.item()), trace.cpu().numpy()
    assert 0 <= it <= 10
    assert np.all(trace[it + 1:] == 0.0)                      # rows past iters + 1 are zero
    return pv, x, it, trace[:it + 1]


def check_against_host(p, delta, par=0.0, label=""):
    """lmparDevice against qrk_bd_lmpar on the same inputs; returns the device's (par, x, iters, trace)"""
    got = device_lmpar(p.qr, p.qtb, p.diag, delta, par)
    want = p.qr.lmpar(p.qtb, p.diag, delta, par, returnTrace=True)
    same = got[0] == want[0] and np.array_equal(got[3], want[3]) and np.array_equal(got[1], want[1])
    print(f"{label}par {got[0]:.17g} (host {want[0]:.17g}), passes {got[2]} (host {want[2]}), "
          f"par / trace / x bit-identical to the host loop: {same}")
    assert got[2] == want[2]
    assert rel(got[0], want[0]) <= 1e-12
    assert got[3].shape == want[3].shape
    for a, b in zip(got[3].ravel(), want[3].ravel()):
        assert rel(a, b) <= 1e-12, (got[3], want[3])
    return got


def check_against_judge(p, f, xtol, got):
    par, x, iters, trace = got
    delta = f * p.dx0
    want_par, _, want_iters, _ = judge.lmpar(p.t, p.diag, delta)
    print(f"f = {f}: par {par:.6e} (judge {want_par:.6e}), passes {iters} (judge {want_iters})")
    assert iters == want_iters and trace[0, 0] == 0.0
    if f == 2.0:
        assert par == 0.0 and iters == 0
        np.testing.assert_array_equal(x, p.qr.lmSolve(p.qtb, p.diag, 0.0))      # the Gauss-Newton step
    else:
        assert par > 0.0 and par == trace[-1, 0]
        assert abs(np.linalg.norm(p.diag * x) - delta) <= 0.1 * delta
        assert rel(par, want_par) <= 1e-9
    for pv, s0, s1 in trace:                                  # every evaluation, at the par the device used
        _, s, _ = judge.solve(p.t, p.diag, pv)
        print(f"  par {pv:.6e}: s0 {rel(s0, s[0]):.2e}, s1 {rel(s1, s[1]):.2e}")
        assert rel(s0, s[0]) <= 1e-9 and rel(s1, s[1]) <= 1e-9, (pv, s0, s1, s)
    want_x, _, _ = judge.solve(p.t, p.diag, par)
    err = judge.per_tile_rel(x, want_x, p.t)
    print(f"  x per tile {err:.2e}")
    assert err <= xtol


# ---- 1. against the host loop and the judge ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,B,r,c,lo,hi,xtol", CASES)
@pytest.mark.parametrize("f", FACTORS)
def test_matches_the_host_loop_and_the_judge(qa, ctx, kernel, B, r, c, lo, hi, xtol, f):
    p = problem(qa, ctx, B, r, c, lo, hi)
    assert kernel in p.qr.lmKernelName()
    check_against_judge(p, f, xtol, check_against_host(p, f * p.dx0))


@pytest.mark.parametrize("f", FACTORS)
def test_mixed_batch_matches_the_host_loop_and_the_judge(qa, ctx, f):
    p = mixed_problem(qa, ctx)
    assert "bd_lm_group_kernel<64>" in p.qr.lmKernelName()
    check_against_judge(p, f, 1e-9, check_against_host(p, f * p.dx0))


# ---- 2. one workgroup, and the capped grid -----------------------------------------------------------------------------------------

class Plain:
    """a batch for the comparisons with the host loop alone (no judge)"""

    def __init__(self, qa, ctx, B, r, c, lo, hi):
        rows, cols = np.full(B, r, np.int32), np.full(B, c, np.int32)
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, seeded_tiles(7 + r + c, lo, hi, B * r * c))
        self.qr = qa.BlockDiagonalSparseQR(context=ctx)
        f = np.random.default_rng(B + r + c).uniform(-1.0, 1.0, B * r)
        _, self.qtb = self.qr.computeAndSolve(mat, f, returnQtB=True)
        norms = self.qr.colNorms()
        self.diag = np.where(norms == 0.0, 1.0, norms)
        self.dx0 = float(np.linalg.norm(self.diag * self.qr.lmSolve(self.qtb, self.diag, 0.0)))


@functools.lru_cache(maxsize=None)
def plain(qa, ctx, B, r, c, lo, hi):
    return Plain(qa, ctx, B, r, c, lo, hi)


@pytest.mark.parametrize("r,c,lo,hi", [(7, 2, 0.5, 5.0), (8, 6, -1.0, 1.0)])
def test_one_tile_is_one_workgroup(qa, ctx, r, c, lo, hi):
    p = plain(qa, ctx, 1, r, c, lo, hi)
    for f in FACTORS:
        par, x, iters, _ = check_against_host(p, f * p.dx0, label=f"f = {f}: ")
        assert (par == 0.0 and iters == 0) if f == 2.0 else (par > 0.0 and abs(np.linalg.norm(p.diag * x) - f * p.dx0) <= 0.1 * f * p.dx0)


def test_more_tiles_than_the_grid_cap(qa, ctx):
    """4097 * 256 tiles of 2 x 1: one more workgroup's worth than the 4096 the thin kernel is launched with, so it strides over the
    grid and the partials of a pass are the capped grid's."""
    p = plain(qa, ctx, 4097 * 256, 2, 1, 0.5, 5.0)
    assert "bd_lm_thin_kernel" in p.qr.lmKernelName()
    for f in (0.1, 2.0):
        par, x, iters, _ = check_against_host(p, f * p.dx0, label=f"f = {f}: ")
        assert (par == 0.0 and iters == 0) if f == 2.0 else (par > 0.0 and abs(np.linalg.norm(p.diag * x) - f * p.dx0) <= 0.1 * f * p.dx0)


def test_the_last_arriver_shape_gives_the_same_bits(qa, ctx, monkeypatch):
    """QRK_LMPAR_CONTROL=last (read at every call) hands the sums and the control step to the last-arriving workgroup of each solve
    instead of a kernel of its own: the same partials added in the same order, so par, x, iters and trace keep their bits -- with
    one workgroup, with several, with the capped grid, in every solve kernel."""
    ps = [problem(qa, ctx, *case[1:6]) for case in CASES] + [mixed_problem(qa, ctx), plain(qa, ctx, 1, 8, 6, -1.0, 1.0),
                                                              plain(qa, ctx, 4097 * 256, 2, 1, 0.5, 5.0)]
    for p in ps:
        for f in (2.0, 0.1):
            monkeypatch.delenv("QRK_LMPAR_CONTROL", raising=False)
            want = device_lmpar(p.qr, p.qtb, p.diag, f * p.dx0)
            monkeypatch.setenv("QRK_LMPAR_CONTROL", "last")
            got = device_lmpar(p.qr, p.qtb, p.diag, f * p.dx0)
            assert got[0] == want[0] and got[2] == want[2]
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[3], want[3])


# ---- 3. start values ---------------------------------------------------------------------------------------------------------------

def test_start_value_is_clamped(qa, ctx):
    """test_lmpar_gpu.test_start_value_is_clamped with lmparDevice"""
    p = problem(qa, ctx, 600, 7, 2, 0.5, 5.0)
    delta = 0.1 * p.dx0
    gnorm = np.sqrt(judge.gradient(p.t, p.diag)[1])
    _, _, _, trace = check_against_host(p, delta, par=1e30)
    assert rel(trace[1, 0], gnorm / delta) <= 1e-12
    s = judge.solve(p.t, p.diag, 0.0)[1]
    parl = (p.dx0 - delta) / (delta * s[1] / s[0])
    assert parl > 0.0
    par, x, iters, trace = check_against_host(p, delta, par=1e-300)
    assert rel(trace[1, 0], parl) <= 1e-9
    want = judge.lmpar(p.t, p.diag, delta, par=1e-300)
    assert iters == want[2] and rel(par, want[0]) <= 1e-9
    assert abs(np.linalg.norm(p.diag * x) - delta) <= 0.1 * delta
    # diag = None is D = I
    d = 0.5 * np.linalg.norm(p.x0)
    par1, x1, it1, tr1 = device_lmpar(p.qr, p.qtb, None, d)
    par2, x2, it2, tr2 = device_lmpar(p.qr, p.qtb, np.ones(p.t.n), d)
    assert par1 == par2 and par1 > 0.0 and it1 == it2
    np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(tr1, tr2)


# ---- 4. what only the device can refuse, and the host-side checks ------------------------------------------------------------------

def test_bad_values_are_refused_on_the_device(qa, ctx):
    p = problem(qa, ctx, 600, 7, 2, 0.5, 5.0)
    good = device_lmpar(p.qr, p.qtb, p.diag, 0.1 * p.dx0)
    for delta, par in ((0.0, 0.25), (-1.0, 0.25), (float("nan"), 0.25), (0.1 * p.dx0, -1.0), (0.1 * p.dx0, float("nan"))):
        pv, _, it, trace = p.qr.lmparDevice(p.qtb, p.diag, delta, par, returnTrace=True)
        assert int(it.item()) == -1
        assert pv.item() == par or (par != par and pv.item() != pv.item())       # left as it was
        assert np.all(trace.cpu().numpy()[1:] == 0.0)                           # no damped evaluation ran
        # a valid call right behind it on the same plan: the control block was reset
        again = device_lmpar(p.qr, p.qtb, p.diag, 0.1 * p.dx0)
        assert again[0] == good[0] and again[2] == good[2]
        np.testing.assert_array_equal(again[1], good[1])
        np.testing.assert_array_equal(again[3], good[3])


def test_null_arguments_on_a_real_plan(qa, ctx):
    import torch
    from qrkit_amd import _capi as capi
    p = problem(qa, ctx, 600, 7, 2, 0.5, 5.0)
    lib, qr = capi.lib(), p.qr
    n = p.t.n
    y, x = torch.ones(n, dtype=torch.float64, device=ctx.device), torch.zeros(n, dtype=torch.float64, device=ctx.device)
    s = torch.ones(2, dtype=torch.float64, device=ctx.device)
    r, pm = qr._r.data_ptr(), qr._perm.data_ptr()
    I = capi.STATUS_INVALID_ARGUMENT
    call = lambda rr, pp, yy, dl, pv, xx: lib.qrk_bd_lmpar_device(qr._plan, rr, pp, yy, None, dl, pv, xx, None, None)
    d, pv = s.data_ptr(), s.data_ptr() + 8
    assert call(None, pm, y.data_ptr(), d, pv, x.data_ptr()) == I
    assert call(r, None, y.data_ptr(), d, pv, x.data_ptr()) == I
    assert call(r, pm, None, d, pv, x.data_ptr()) == I
    assert call(r, pm, y.data_ptr(), None, pv, x.data_ptr()) == I
    assert call(r, pm, y.data_ptr(), d, None, x.data_ptr()) == I
    assert call(r, pm, y.data_ptr(), d, pv, None) == I
    assert b"qrk_bd_lmpar_device" in lib.qrk_last_error(ctx.handle)
    assert call(r, pm, y.data_ptr(), d, pv, x.data_ptr()) == capi.STATUS_OK      # iters and trace may be NULL
    ctx.synchronize()


def test_unsupported_plans_are_refused(qa, ctx):
    import torch
    from qrkit_amd import _capi as capi
    lib = capi.lib()
    for (B, r, c, fmt, n, nr, why) in ((2, 64, 64, 0, 128, 2 * 64 * 65 // 2, b"more than 32 columns"), (10, 7, 2, 1, 20, 30, b"FullQ")):
        qr = qa.BlockDiagonalSparseQR(context=ctx, qFormat=fmt)
        qr.analyzePattern(qa.SparseBlockDiagonal.fromTiles(np.full(B, r, np.int32), np.full(B, c, np.int32), np.zeros(B * r * c)))
        rv = torch.ones(nr, dtype=torch.float64, device=ctx.device)
        pm = torch.arange(n, dtype=torch.int32, device=ctx.device)
        y, x = torch.ones(n, dtype=torch.float64, device=ctx.device), torch.zeros(n, dtype=torch.float64, device=ctx.device)
        s = torch.ones(2, dtype=torch.float64, device=ctx.device)
        st = lib.qrk_bd_lmpar_device(qr._plan, rv.data_ptr(), pm.data_ptr(), y.data_ptr(), None, s.data_ptr(), s.data_ptr() + 8, x.data_ptr(),
                                     None, None)
        assert st == capi.STATUS_UNSUPPORTED
        assert b"qrk_bd_lmpar_device" in lib.qrk_last_error(ctx.handle) and why in lib.qrk_last_error(ctx.handle)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------

def test_two_identical_calls_give_identical_bits(qa, ctx):
    for p in (problem(qa, ctx, 600, 7, 2, 0.5, 5.0), problem(qa, ctx, 100, 16, 12, -1.0, 1.0), mixed_problem(qa, ctx)):
        for f in (0.5, 0.01):
            a = device_lmpar(p.qr, p.qtb, p.diag, f * p.dx0)
            b = device_lmpar(p.qr, p.qtb, p.diag, f * p.dx0)
            assert a[0] == b[0] and a[2] == b[2]
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[3], b[3])


# ---- 6. no synchronisation, shown by capture -------------------------------------------------------------------------------------------

def test_one_captured_call_replays_with_new_radii(qa, ctx):
    """One lmparDevice call captured into a torch.cuda.CUDAGraph (a single chain on the capture stream) and replayed with delta and
    par written into the static tensors: every replay gives the bits of the eager call for that delta."""
    import torch
    p = problem(qa, ctx, 600, 7, 2, 0.5, 5.0)
    dev = ctx.device
    qtb, diag = torch.from_numpy(np.ascontiguousarray(p.qtb[:p.t.n])).to(dev), torch.from_numpy(p.diag).to(dev)
    factors = (0.5, 0.1, 2.0)
    eager = [device_lmpar(p.qr, qtb, diag, f * p.dx0) for f in factors]          # (the first LM call allocated the plan's scratch)
    delta = torch.tensor([factors[0] * p.dx0], dtype=torch.float64, device=dev)
    out = (torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(p.t.n, dtype=torch.float64, device=dev),
           torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((11, 3), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        p.qr.lmparDevice(qtb, diag, delta, out[0], out=out, returnTrace=True)
    for f, want in zip(factors, eager):
        delta.fill_(f * p.dx0)
        out[0].zero_()
        out[1].fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        it = int(out[2].item())
        assert it == want[2] and out[0].item() == want[0]
        np.testing.assert_array_equal(out[1].cpu().numpy(), want[1])
        np.testing.assert_array_equal(out[3].cpu().numpy()[:it + 1], want[3])
        assert np.all(out[3].cpu().numpy()[it + 1:] == 0.0)


def test_a_capture_on_a_fresh_plan_is_refused(qa, ctx):
    """The plan's scratch is allocated by the first LM call; under capture that call must fail instead of allocating."""
    import torch
    from qrkit_amd._capi import QrkError
    dev = ctx.device
    B = 50
    mat = qa.SparseBlockDiagonal.fromTiles(np.full(B, 7, np.int32), np.full(B, 2, np.int32), seeded_tiles(3, 0.5, 5.0, B * 14))
    qr = qa.BlockDiagonalSparseQR(context=ctx)
    _, qtb = qr.computeAndSolve(mat, np.random.default_rng(1).uniform(-1.0, 1.0, B * 7), returnQtB=True)
    qtb = torch.from_numpy(np.ascontiguousarray(qtb[:2 * B])).to(dev)
    delta = torch.tensor([1e-3], dtype=torch.float64, device=dev)
    out = (torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(2 * B, dtype=torch.float64, device=dev),
           torch.zeros(1, dtype=torch.int32, device=dev), None)
    marker = torch.zeros(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    graph, caught = torch.cuda.CUDAGraph(), None
    with capture(graph):
        marker.add_(1.0)                                      # (the capture is not empty)
        try:
            qr.lmparDevice(qtb, None, delta, out[0], out=out)
        except QrkError as e:
            caught = e
    assert caught is not None and "outside the capture" in str(caught)
    # the same call outside a capture allocates and runs
    par, x, it = qr.lmparDevice(qtb, None, delta, 0.0)
    assert int(it.item()) >= 1 and par.item() > 0.0


# ---- 7. the trust-region fit -----------------------------------------------------------------------------------------------------------

def test_trust_region_fit_on_undamped_tiles(qa):
    """test_lmpar_gpu.test_trust_region_fit_on_undamped_tiles with lmparDevice for the step: the host reads par and dx once per trial
    step instead of the sums once per evaluation."""
    B = 500
    rng = np.random.default_rng(5)
    t = np.linspace(0.0, 1.0, 7)
    a_true, b_true = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    y = np.exp(a_true[:, None] * t) + b_true[:, None]
    qr = qa.BlockDiagonalSparseQR(context=qa.Context(0))
    rows, cols = np.full(B, 7, np.int32), np.full(B, 2, np.int32)
    a, b = np.zeros(B), np.zeros(B)

    def residual(a, b):
        return np.exp(a[:, None] * t) + b[:, None] - y          # (B, 7)

    cost = 0.5 * np.sum(residual(a, b) ** 2)
    analysed, delta, par, diag = False, None, 0.0, None
    factorizations = damped_steps = 0
    for it in range(40):
        r = residual(a, b)
        J = np.zeros((B, 2, 7))                                   # column-major 7x2 tiles
        J[:, 0, :] = t * np.exp(a[:, None] * t)                   # d/da
        J[:, 1, :] = 1.0                                          # d/db
        mat = qa.SparseBlockDiagonal.fromTiles(rows, cols, J.ravel())
        if not analysed:
            qr.analyzePattern(mat)
            analysed = True
            assert "bd_lm_thin_kernel" in qr.lmKernelName()
        qtb = qr.factorizeAndSolve(mat, (-r).ravel(), returnQtB=True, solve=False)
        factorizations += 1
        norms = qr.colNorms()
        diag = np.where(norms == 0.0, 1.0, norms) if diag is None else np.maximum(diag, norms)
        if delta is None:
            delta = 1.0                                           # a small region: the first steps are damped ones
        for inner in range(20):                                   # trial steps on the SAME factors
            par_t, dx_t, it_t = qr.lmparDevice(qtb, diag, delta, par)
            par, dx = par_t.item(), dx_t.cpu().numpy().reshape(B, 2)          # the one read-back of the trial step
            assert int(it_t.item()) >= 0
            damped_steps += par > 0.0
            pnorm = np.linalg.norm(diag * dx.ravel())
            new_cost = 0.5 * np.sum(residual(a + dx[:, 0], b + dx[:, 1]) ** 2)
            lin = r + np.einsum("bcr,bc->br", J, dx)
            predicted = cost - 0.5 * np.sum(lin ** 2)
            ratio = (cost - new_cost) / predicted if predicted > 0 else 0.0
            if ratio <= 0.25:
                delta = 0.5 * min(delta, pnorm)
            elif par == 0.0 or ratio >= 0.75:
                delta = 2.0 * pnorm
            if ratio >= 1e-4:
                a, b, cost = a + dx[:, 0], b + dx[:, 1], new_cost
                break
        if cost < 1e-24:
            break
    print(f"{factorizations} factorisations, {damped_steps} damped steps, cost {cost:.2e}")
    assert damped_steps >= 3                                      # (the numpy loop takes five before the region stops binding)
    assert np.max(np.abs(a - a_true)) < 1e-8 and np.max(np.abs(b - b_true)) < 1e-8
