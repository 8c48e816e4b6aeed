#!/usr/bin/env python
"""Times one Levenberg-Marquardt step of the block-angular composition: BlockAngularSparseQR.compute() + solve() (the explicit
route: Q1 written and read back, the strip and the bottom block cut out by copies) against computeAndSolve() (the fused route over
qrk_bd_factorize_apply_qt: one device matrix W, no Q1), and the panel kernel alone.  Writes the table profiles/angular_qless_bench.txt keeps.

Method, as tools/bench_qless.py: HIP events on the current stream around a window of back-to-back steps; the inputs (tiles, J2, b) of
a window are rotated so that their footprint exceeds the 256 MiB Infinity Cache (the solver's own work matrices are reused from step
to step, as in an LM loop); warm-up of every route first; repeats with the routes interleaved (A B A B ...), median and spread
reported.  A step is what the Python mirror does for it, its host-side bookkeeping and synchronisations included.  The panel kernel
alone is qrk_bd_factorize_apply_qt on the same rotating inputs; its bytes are the algorithmic ones (tiles, R and the permutation once,
the panel in and out), the fraction is of the nominal 8 TB/s of HBM3E.  Device memory: what torch holds after a step with the solver
alive, and the peak during it (the library's plan workspaces are outside torch's count and the same for both routes).

    python tools/bench_angular_lm.py [--out FILE] [--commit ID] [--repeats 5] [--routes explicit,fused,panel]
                                        [--shapes 2x1:500000:5,9x2:1000000:8,9x2:250000:8,7x2:1024:384,7x2:20000:384]
"""
import argparse
import ctypes as C
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


def bench_shape(B, r, c, m2, repeats, log, want=("explicit", "fused", "panel")):
    dev = torch.device("cuda", 0)
    rows, m1 = B * r, B * c
    in_bytes = 8 * (B * r * c + rows * (m2 + 1))
    nsets = max(2, min(32, math.ceil(2 * INFINITY_CACHE / in_bytes)))
    g = torch.Generator(device=dev); g.manual_seed(4321 + r * 100 + c + m2)
    f64 = dict(dtype=torch.float64, device=dev)
    tiles = [torch.rand(B * r * c, generator=g, **f64) * 4.5 + 0.5 for _ in range(nsets)]
    # [J2 | b] of a set in one column-major buffer: J2 is a view of it (what both routes are handed), the whole is the kernel's panel
    panels = [(torch.rand(m2 + 1, rows, generator=g, **f64) * 4.5 + 0.5).t() for _ in range(nsets)]
    brows, bcols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    mats = [qrkit_amd.BlockMatrix1x2(qrkit_amd.SparseBlockDiagonal.fromTiles(brows, bcols, tiles[s]), panels[s][:, :m2]) for s in range(nsets)]
    rhs = [panels[s][:, m2].contiguous() for s in range(nsets)]

    def held(make_and_step):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        solver = make_and_step()
        torch.cuda.synchronize()
        return solver, torch.cuda.memory_allocated() - base, torch.cuda.max_memory_allocated() - base

    def explicit_step(solver, s):
        solver.compute(mats[s])
        return solver.solve(rhs[s])

    def fused_step(solver, s):
        return solver.computeAndSolve(mats[s], rhs[s])

    def first(step):
        def run():
            solver = qrkit_amd.BlockAngularSparseQR()
            run.x = step(solver, 0)
            return solver
        return run

    fe, ff = first(explicit_step), first(fused_step)
    explicit = fused = None
    held_e = peak_e = held_f = peak_f = 0
    note = ""
    try:
        if "explicit" in want:
            explicit, held_e, peak_e = held(fe)
        if "fused" in want:
            fused, held_f, peak_f = held(ff)
    except capi.QrkError as e:                      # (a shape the dense right solver does not take: neither route runs)
        explicit = fused = None
        note = f"; NEITHER ROUTE RUNS: {e}"
    both = explicit is not None and fused is not None
    rel = float((ff.x - fe.x).norm() / fe.x.norm()) if both else float("nan")
    same_perm = bool(np.array_equal(explicit.colsPermutation(), fused.colsPermutation())) if both else True

    # the panel kernel alone, on a left solver's plan of its own
    lib, left = capi.lib(), qrkit_amd.BlockDiagonalSparseQR(hCoeffs=False)
    left.analyzePattern(mats[0].leftBlock())
    kernel = left.panelKernelName(m2 + 1)
    out = torch.empty(m2 + 1, rows, **f64)
    rv = torch.empty(max(B * (c * (c + 1) // 2), 1), **f64)
    pm = torch.empty(m1, dtype=torch.int32, device=dev)

    def panel_step(_, s):
        capi.check(lib.qrk_bd_factorize_apply_qt(left._plan, tiles[s].data_ptr(), panels[s].data_ptr(), rows, m2 + 1, rv.data_ptr(), pm.data_ptr(),
                                                 None, out.data_ptr(), rows, capi.MEM_DEVICE), left._ctx.handle)

    panel_bytes = B * (8 * r * c + 8 * (c * (c + 1) // 2) + 4 * c) + 2 * 8 * rows * (m2 + 1)
    routes = {}
    if explicit is not None:
        routes["compute()+solve()"] = (explicit_step, explicit)
    if fused is not None:
        routes["computeAndSolve()"] = (fused_step, fused)
    if "panel" in want:
        routes["panel kernel alone"] = (panel_step, None)
    for name, (fn, solver) in routes.items():           # warm-up of every route on every set
        for s in range(nsets):
            fn(solver, s)
    torch.cuda.synchronize()

    def window(fn, solver, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(solver, i % nsets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters       # ms per step

    iters = {}
    for name, (fn, solver) in routes.items():            # windows of about 0.1 s, a whole number of rotations
        t = window(fn, solver, nsets)
        iters[name] = max(nsets, min(100 * nsets, int(math.ceil(100.0 / max(t, 1e-3) / nsets)) * nsets))
    times = {name: [] for name in routes}
    for rep in range(repeats):
        for name, (fn, solver) in routes.items():
            times[name].append(window(fn, solver, iters[name]))
    log(f"\n{B} blocks of {r}x{c} next to {m2} dense columns ({rows} rows; {nsets} rotating input sets; x of the two routes differs by {rel:.1e}, "
        f"permutations {'equal' if same_perm else 'DIFFER'}; kernel: {kernel}{note})")
    log(f"  {'route':<22}{'median us':>11}{'min':>10}{'max':>10}{'spread':>8}{'steps':>7}{'held MiB':>10}{'peak MiB':>10}")
    med = {}
    mem = {"compute()+solve()": (held_e, peak_e), "computeAndSolve()": (held_f, peak_f), "panel kernel alone": (0, 0)}
    for name in routes:
        ts = [1e3 * t for t in times[name]]
        med[name] = statistics.median(ts)
        h, p = mem[name]
        log(f"  {name:<22}{med[name]:>11.1f}{min(ts):>10.1f}{max(ts):>10.1f}{(max(ts) - min(ts)) / med[name]:>8.1%}{iters[name]:>7d}"
            f"{h / 2**20:>10.1f}{p / 2**20:>10.1f}")
    if "panel kernel alone" in med:
        rate = panel_bytes / (med["panel kernel alone"] * 1e-6)
        log(f"  panel kernel alone: {panel_bytes / B:.0f} B per block, {rate / 1e9:.0f} GB/s = {rate / HBM_BYTES_PER_S:.1%} of 8 TB/s")
    if not both:
        return
    clear = max(times["computeAndSolve()"]) < min(times["compute()+solve()"])
    log(f"  computeAndSolve() against compute()+solve(): {med['compute()+solve()'] / med['computeAndSolve()']:.2f}x"
        f" ({'every repeat faster than every repeat of the explicit route' if clear else 'NOT every repeat faster than every repeat of the explicit route'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="2x1:500000:5,9x2:1000000:8,9x2:250000:8,7x2:1024:384,7x2:20000:384")
    ap.add_argument("--routes", default="explicit,fused,panel", help="which of the three to run (a kernel trace of one route alone)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_angular_lm.py needs the GPU: there is no CPU timing"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                              # (kept up to date: a long shape must not lose the ones before it)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import datetime
    log("One LM step of the block-angular composition: compute() + solve() against computeAndSolve() (tools/bench_angular_lm.py)")
    log(f"date: {datetime.date.today().isoformat()}; box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the current stream, inputs rotated past the {INFINITY_CACHE >> 20} MiB Infinity Cache, {args.repeats} interleaved repeats")
    for spec in args.shapes.split(","):
        shape, count, m2 = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        bench_shape(int(count), r, c, int(m2), args.repeats, log, tuple(args.routes.split(",")))


if __name__ == "__main__":
    main()
