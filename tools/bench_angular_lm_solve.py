#!/usr/bin/env python
"""Times one TRIAL DAMPING of a Levenberg-Marquardt step on the block-angular composition:
  (a) the parent route: BlockAngularSparseQR.computeAndSolve() on the damped matrix [J; sqrt(par) I] in block-angular form (c damping
      rows appended to every left tile, m2 damping rows below J2, b zero-padded) -- a factorisation per trial;
  (b) BlockAngularSparseQR.lmSolve(None, par) on the factors one computeAndSolve() of the undamped matrix left on the device;
  (c) the panel kernel alone (qrk_bd_lm_panel on the same kept factors), with its share of the nominal 8 TB/s of HBM3E on the
      algorithmic bytes (R and S once, the permutation, the panel in and twice out);
  (d) the dense part alone (qrk_dense_lm_stack, the un-pivoted factorisation of the right stack, Q^T on its last column, the
      triangular solve), between an event pair per step behind the panel kernel that refills the stack.
Writes the table profiles/angular_lm_solve_bench.txt keeps.

Method, as tools/bench_lm.py and tools/bench_angular_lm.py: HIP events on the current stream around windows of back-to-back calls;
the inputs of a window -- the damped tiles / J2 / b for (a), the kept factors of one solver per set for (b)-(d) -- are rotated so that
their footprint exceeds the 256 MiB Infinity Cache; warm-up of every route first; repeats with the routes interleaved, median
(min-max) reported.  A call is what the Python mirror does for it, its host-side bookkeeping and synchronisations included.

    python tools/bench_angular_lm_solve.py [--out FILE] [--commit ID] [--repeats 5] [--par 0.01]
                                           [--shapes 2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8]
"""
import argparse
import math
import os
import platform
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qrkit_amd  # noqa: E402
from qrkit_amd import _capi as capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
INFINITY_CACHE = 256 << 20


def bench_shape(B, r, c, m2, par, repeats, log):
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    rows, m1, rd = B * r, B * c, B * (r + c) + m2
    g = torch.Generator(device=dev); g.manual_seed(977 + r * 100 + c + m2)
    sq = math.sqrt(par)
    # rotating sets: enough of them that the smaller footprint (the kept factors the panel kernel reads and writes) passes the cache
    touched = 8 * 3 * m1 * (m2 + 1)
    nsets = max(2, min(12, math.ceil(2 * INFINITY_CACHE / touched)))
    brows, bcols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    drows = np.full(B, r + c, np.int32)
    kept, damped = [], []
    for s in range(nsets):
        t = torch.randn(B, c, r, generator=g, **f64)                                  # column-major r x c tiles
        J2 = torch.randn(m2 + 1, rows, generator=g, **f64).t()                         # [J2 | b], column-major
        solver = qrkit_amd.BlockAngularSparseQR()
        solver.setLmRoute("stacked")               # K11's chain, the one the committed table measures (tools/bench_angular_lm_reduced.py: K13's)
        solver.computeAndSolve(qrkit_amd.BlockMatrix1x2(qrkit_amd.SparseBlockDiagonal.fromTiles(brows, bcols, t.reshape(-1)), J2[:, :m2]),
                               J2[:, m2].contiguous())
        kept.append(solver)
        # the damped matrix of the parent route
        td = torch.zeros(B, c, r + c, **f64)
        td[:, :, :r] = t
        td[:, torch.arange(c), r + torch.arange(c)] = sq
        core = torch.zeros(m2 + 1, B, r + c, **f64)
        core[:, :, :r] = J2.t().reshape(m2 + 1, B, r)
        Jd = torch.zeros(m2 + 1, rd, **f64)
        Jd[:, :B * (r + c)] = core.reshape(m2 + 1, B * (r + c))
        del core
        Jd[torch.arange(m2), B * (r + c) + torch.arange(m2)] = sq
        Jd = Jd.t()
        damped.append((qrkit_amd.BlockMatrix1x2(qrkit_amd.SparseBlockDiagonal.fromTiles(drows, bcols, td.reshape(-1)), Jd[:, :m2]),
                       Jd[:, m2].contiguous()))
    parent = qrkit_amd.BlockAngularSparseQR()
    x_parent = parent.computeAndSolve(*damped[0])
    x_kept = kept[0].lmSolve(None, par)
    rel = float((x_kept - x_parent).norm() / x_parent.norm())
    for s in kept:                                                                     # (the kept arrays of every solver exist)
        s.lmSolve(None, par)
    lib = capi.lib()
    kernel = lib.qrk_bd_lm_panel_kernel_name(kept[0].m_leftSolver._plan, m2 + 1).decode()
    ldg = m1 + 2 * m2

    def parent_step(s):
        parent.computeAndSolve(*damped[s])

    def lm_step(s):
        kept[s].lmSolve(None, par)

    def panel_step(s):
        k = kept[s]
        lm, left = k._lm, k.m_leftSolver
        capi.check(lib.qrk_bd_lm_panel(left._plan, left._r.data_ptr(), left._perm.data_ptr(), None, par, k._W.data_ptr(), rows, m2 + 1,
                                       lm["colidx"].data_ptr(), lm["s"].data_ptr(), lm["top"].data_ptr(), m1, lm["G"].data_ptr() + 8 * m2, ldg),
                   k._ctx.handle)

    def dense_step(s):
        k = kept[s]
        lm, W, G = k._lm, k._W, k._lm["G"]
        capi.check(lib.qrk_dense_lm_stack(k._ctx.handle, W.data_ptr() + 8 * m1, rows, m2, W.data_ptr() + 8 * (m2 * rows + m1), None,
                                          k.m_rightSolver.colsPermutation().data_ptr(), par, m1, G.data_ptr(), ldg), k._ctx.handle)
        dense = lm["dense"].compute(G[:, :m2])
        dense.applyQ(G[:, m2:], transpose=True)
        dense.solveR(G[:m2, m2].clone().reshape(m2, 1))

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters       # ms per call

    def dense_window(_, iters):
        """the dense part between an event pair per step, behind the panel kernel that refills the fill rows of the stack"""
        pairs = []
        for i in range(iters):
            panel_step(i % nsets)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dense_step(i % nsets)
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) / iters

    routes = {"(a) damped computeAndSolve()": (window, parent_step), "(b) lmSolve()": (window, lm_step),
              "(c) panel kernel alone": (window, panel_step), "(d) dense part alone": (dense_window, None)}
    for name, (win, fn) in routes.items():                  # warm-up of every route on every set
        win(fn, nsets)
    torch.cuda.synchronize()
    iters = {}
    for name, (win, fn) in routes.items():                  # windows of about 0.1 s, a whole number of rotations
        t = win(fn, nsets)
        iters[name] = max(nsets, min(100 * nsets, int(math.ceil(100.0 / max(t, 1e-3) / nsets)) * nsets))
    times = {name: [] for name in routes}
    for rep in range(repeats):
        for name, (win, fn) in routes.items():
            times[name].append(win(fn, iters[name]))
    log(f"\n{B} blocks of {r}x{c} next to {m2} dense columns ({rows} rows, damped {rd}; par {par:g}; {nsets} rotating sets; x of (a) and (b) "
        f"differs by {rel:.1e}; kernel: {kernel}; right stack {ldg} x {m2})")
    log(f"  {'route':<30}{'median us':>11}{'min':>10}{'max':>10}{'spread':>8}{'calls':>7}")
    med = {}
    for name in routes:
        ts = [1e3 * t for t in times[name]]
        med[name] = statistics.median(ts)
        log(f"  {name:<30}{med[name]:>11.1f}{min(ts):>10.1f}{max(ts):>10.1f}{(max(ts) - min(ts)) / med[name]:>8.1%}{iters[name]:>7d}")
    panel_bytes = B * (2 * 8 * (c * (c + 1) // 2) + 4 * c) + 3 * 8 * m1 * (m2 + 1)
    rate = panel_bytes / (med["(c) panel kernel alone"] * 1e-6)
    log(f"  panel kernel alone: {panel_bytes / B:.0f} B per block, {rate / 1e12:.2f} TB/s = {rate / HBM_BYTES_PER_S:.2f} of 8 TB/s")
    a, b = "(a) damped computeAndSolve()", "(b) lmSolve()"
    clear = max(times[b]) < min(times[a]) or min(times[b]) > max(times[a])
    log(f"  lmSolve() against the damped computeAndSolve(): {med[a] / med[b]:.2f}x"
        f" ({'every repeat on one side of every repeat of the other route' if clear else 'the repeats of the two routes overlap'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--par", type=float, default=1e-2)
    ap.add_argument("--shapes", default="2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_angular_lm_solve.py needs the GPU: there is no CPU timing"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                              # (kept up to date: a long shape must not lose the ones before it)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import datetime
    log("One trial damping of an LM step on the block-angular composition: computeAndSolve() on the damped matrix against lmSolve() "
        "(tools/bench_angular_lm_solve.py)")
    log(f"date: {datetime.date.today().isoformat()}; box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the current stream, inputs rotated past the {INFINITY_CACHE >> 20} MiB Infinity Cache, {args.repeats} interleaved repeats")
    for spec in args.shapes.split(","):
        shape, count, m2 = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        bench_shape(int(count), r, c, int(m2), args.par, args.repeats, log)


if __name__ == "__main__":
    main()
