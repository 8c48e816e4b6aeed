#!/usr/bin/env python
"""Times the Levenberg-Marquardt step on the factors (qrk_bd_lm_solve with its sums at one par; a whole qrk_bd_lmpar with
delta = 0.1 ||D x0||) against what an LM caller did before for ONE trial damping: qrk_bd_factorize_rhs on the damped
(r + c) x c tiles [J_i; sqrt(par) D_i].  Writes the table that profiles/lm_bench.txt keeps.

Method (tools/bench_qless.py's): HIP events on the handle's stream around a window of back-to-back calls; the input / output
sets of a route are rotated so that the footprint of a window exceeds the 256 MiB Infinity Cache; warm-up of every route on
every set first; five repeats with the routes interleaved, median and spread reported.  Bytes per tile are the algorithmic
ones, the rate is those bytes over the measured time.  qrk_bd_lmpar synchronises the stream once per evaluation: its window is
timed like the others (events see the idle gaps), and "lmpar kernels" replays the same evaluations enqueue-only -- the
difference is the cost of the synchronisations.

    python tools/bench_lm.py [--out FILE] [--commit ID] [--shapes 7x2:1000000,8x6:250000,32x32:10000,32x32:160000]
"""
import argparse
import ctypes as C
import math
import os
import platform
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qrkit_amd  # noqa: E402
from qrkit_amd import _capi as capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
INFINITY_CACHE = 256 << 20
PAR = 1.0


def route_bytes(r, c):
    """Algorithmic bytes per tile of each route."""
    rr, perm, vec = 8 * (c * (c + 1) // 2), 4 * c, 8 * c
    return {
        "factorize_rhs damped": 8 * (r + c) * c + 8 * (r + c) + rr + perm + vec,     # tile, b, R, perm, x
        "lm_solve + sums": rr + perm + 3 * vec,                                       # R, perm, y, diag, x
    }


def make_plan(ctx, B, r, c):
    lay = capi.BDLayout()
    lay.num_blocks, lay.block_rows, lay.block_cols = B, r, c
    lay.rows = lay.cols = None
    lay.mat_rows, lay.mat_cols = B * r, B * c
    plan = C.c_void_p()
    capi.check(capi.lib().qrk_bd_plan_create(ctx.handle, C.byref(lay), capi.FULL_Q, capi.COLPIV_HOUSEHOLDER, C.byref(plan)), ctx.handle)
    return plan


def bench_shape(ctx, B, r, c, repeats, log):
    lib, dev = capi.lib(), ctx.device
    plan, dplan = make_plan(ctx, B, r, c), make_plan(ctx, B, r + c, c)
    nbytes = route_bytes(r, c)
    nsets = max(2, math.ceil(2 * INFINITY_CACHE / (B * nbytes["lm_solve + sums"])))
    g = torch.Generator(device=dev); g.manual_seed(4321 + r * 100 + c)
    f64 = dict(dtype=torch.float64, device=dev)
    lo, hi = (-1.0, 1.0) if c == 32 else (0.5, 5.0)
    nr = B * (c * (c + 1) // 2)
    rv = torch.empty(nsets, nr, **f64)
    perm = torch.empty(nsets, B * c, dtype=torch.int32, device=dev)
    y = torch.empty(nsets, B * c, **f64)
    diag = torch.empty(nsets, B * c, **f64)
    x = torch.empty(nsets, B * c, **f64)
    sums = torch.empty(nsets, 4, **f64)
    damped = torch.zeros(nsets, B, c, r + c, **f64)
    drhs = torch.zeros(nsets, B, r + c, **f64)
    drv, dperm, dx = torch.empty(nsets, nr, **f64), torch.empty(nsets, B * c, dtype=torch.int32, device=dev), torch.empty(nsets, B * c, **f64)
    k = torch.arange(c, device=dev)
    for s in range(nsets):
        # the undamped factors and Q^T f of set s (what a Jacobian evaluation leaves), the column norms as diag, then the damped tiles
        tiles = torch.rand(B, c, r, generator=g, **f64) * (hi - lo) + lo
        f = torch.rand(B, r, generator=g, **f64) * 2 - 1
        qtb = torch.empty(B * r, **f64)
        capi.check(lib.qrk_bd_factorize_rhs(plan, tiles.data_ptr(), f.data_ptr(), 1, rv[s].data_ptr(), perm[s].data_ptr(), None,
                                            qtb.data_ptr(), None, capi.MEM_DEVICE), ctx.handle)
        capi.check(lib.qrk_bd_r_col_norms(plan, rv[s].data_ptr(), perm[s].data_ptr(), diag[s].data_ptr(), capi.MEM_DEVICE), ctx.handle)
        torch.cuda.synchronize()
        y[s].copy_(qtb[:B * c])
        damped[s, :, :, :r] = tiles
        damped[s, :, k, r + k] = math.sqrt(PAR) * diag[s].view(B, c)
        drhs[s, :, :r] = f
        del tiles, f, qtb

    def refactorize(s):
        capi.check(lib.qrk_bd_factorize_rhs(dplan, damped[s].data_ptr(), drhs[s].data_ptr(), 1, drv[s].data_ptr(), dperm[s].data_ptr(), None,
                                            None, dx[s].data_ptr(), capi.MEM_DEVICE), ctx.handle)

    def lm_solve(s, par=PAR):
        capi.check(lib.qrk_bd_lm_solve(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(), par, x[s].data_ptr(),
                                       sums[s].data_ptr(), capi.MEM_DEVICE), ctx.handle)

    # same answer first
    refactorize(0); lm_solve(0)
    torch.cuda.synchronize()
    rel = float((x[0] - dx[0]).norm() / dx[0].norm())
    # the trust region of the lmpar rows: a tenth of the Gauss-Newton step of every set
    deltas, traces = [], []
    for s in range(nsets):
        lm_solve(s, 0.0)
        torch.cuda.synchronize()
        deltas.append(0.1 * math.sqrt(float(sums[s, 0])))
    par_out, iters_out, trace = C.c_double(0.0), C.c_int32(0), (C.c_double * 33)()

    def lmpar(s):
        par_out.value = 0.0
        capi.check(lib.qrk_bd_lmpar(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(), deltas[s], C.byref(par_out),
                                    x[s].data_ptr(), C.byref(iters_out), trace), ctx.handle)

    for s in range(nsets):
        lmpar(s)
        traces.append([trace[3 * e] for e in range(iters_out.value + 1)])
    passes = [len(t) - 1 for t in traces]

    def lmpar_kernels(s):
        # the evaluations of lmpar(s) again, enqueue-only: the damped solves at the traced par and the gradient
        for e, pv in enumerate(traces[s]):
            lm_solve(s, pv)
            if e == 0:
                capi.check(lib.qrk_bd_lm_gradient(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(), None,
                                                  sums[s, 3:].data_ptr(), capi.MEM_DEVICE), ctx.handle)

    routes = {"factorize_rhs damped": refactorize, "lm_solve + sums": lm_solve, "lmpar": lmpar, "lmpar kernels": lmpar_kernels}
    for name, fn in routes.items():
        for s in range(nsets):
            fn(s)
    torch.cuda.synchronize()

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters       # ms per call

    iters = {}
    for name, fn in routes.items():               # windows of about 0.2 s, a whole number of rotations
        t = window(fn, nsets)
        iters[name] = max(nsets, min(400, int(math.ceil(200.0 / max(t, 1e-3) / nsets)) * nsets))
    times = {name: [] for name in routes}
    for rep in range(repeats):
        for name, fn in routes.items():
            times[name].append(window(fn, iters[name]))
    kernel, dkernel = lib.qrk_bd_lm_kernel_name(plan).decode(), lib.qrk_bd_rhs_kernel_name(dplan, 1).decode()
    lib.qrk_bd_plan_destroy(plan); lib.qrk_bd_plan_destroy(dplan)
    log(f"\n{B} tiles of {r}x{c} (damped: {r + c}x{c}), par = {PAR:g}, diag = column norms   ({nsets} rotating sets; x of the two routes differs by "
        f"{rel:.1e})")
    log(f"  kernels: {kernel}; the damped factorisation: {dkernel}")
    log(f"  lmpar: delta = 0.1 |D x0|, {min(passes)}..{max(passes)} passes = {min(passes) + 1}..{max(passes) + 1} evaluations and synchronisations per call")
    log(f"  {'route':<22}{'median us':>11}{'min':>9}{'max':>9}{'spread':>8}{'calls':>7}{'B/tile':>8}{'GB/s':>8}{'of 8 TB/s':>10}")
    med = {}
    for name in routes:
        ts = [1e3 * t for t in times[name]]
        med[name] = statistics.median(ts)
        if name in nbytes:
            rate = B * nbytes[name] / (med[name] * 1e-6)
            tail = f"{nbytes[name]:>8d}{rate / 1e9:>8.0f}{rate / HBM_BYTES_PER_S:>10.1%}"
        else:
            tail = f"{'-':>8}{'-':>8}{'-':>10}"
        log(f"  {name:<22}{med[name]:>11.1f}{min(ts):>9.1f}{max(ts):>9.1f}{(max(ts) - min(ts)) / med[name]:>8.1%}{iters[name]:>7d}{tail}")
    clear = max(times["lm_solve + sums"]) < min(times["factorize_rhs damped"])
    log(f"  lm_solve + sums against factorize_rhs damped: {med['factorize_rhs damped'] / med['lm_solve + sums']:.2f}x"
        f" ({'every repeat faster than every repeat of the refactorisation' if clear else 'NOT clear of the run-to-run spread'})")
    evals = statistics.mean(passes) + 1
    log(f"  lmpar against {evals:.1f} refactorisations (one per evaluation): {evals * med['factorize_rhs damped'] / med['lmpar']:.2f}x")
    log(f"  lmpar's synchronisations: {med['lmpar'] - med['lmpar kernels']:.1f} us per call, "
        f"{(med['lmpar'] - med['lmpar kernels']) / evals:.1f} us per evaluation (whole call minus its kernels)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="7x2:1000000,8x6:250000,32x32:10000,32x32:160000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm.py needs the GPU: there is no CPU timing"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    ctx = qrkit_amd.Context(0)
    log("The LM step on the factors against re-factorising the damped tiles (tools/bench_lm.py)")
    log(f"box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the handle's stream, sets rotated past the {INFINITY_CACHE >> 20} MiB Infinity Cache, {args.repeats} interleaved repeats")
    for spec in args.shapes.split(","):
        shape, count = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        bench_shape(ctx, int(count), r, c, args.repeats, log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
