#!/usr/bin/env python
"""Times a whole MINPACK lmpar on the block-diagonal factors three ways, in one process on the same inputs and radii:

  lmpar (host loop)       qrk_bd_lmpar: one stream synchronisation per evaluation
  lmpar_device            qrk_bd_lmpar_device: one enqueue (a memset and 24 launches, those behind the stop return at once),
                          plus the one-element fill that puts the start value par = 0 back into device memory
  lmpar_device, replayed  the same call captured once per input set into a graph (torch.cuda.graph) and replayed

With QRK_LMPAR_CONTROL=last in the environment the device routes run the other shape of the control step (the solve's last-arriving
workgroup instead of a kernel of its own: a memset and 14 launches); run the tool once each way for DESIGN.md K10's two tables.

Writes the table that profiles/lmpar_device_bench.txt keeps.  Method (tools/bench_lm.py's): HIP events on the handle's stream around
a window of back-to-back calls; the input / output sets are rotated so that the footprint of a window exceeds the 256 MiB Infinity
Cache (at most --max-sets of them: a small batch is bound by launches, not by memory); warm-up of every route on every set first;
five repeats with the routes interleaved, median and min-max reported.  No route reads a result back inside the window.

    python tools/bench_lmpar_device.py [--out FILE] [--commit ID] [--cases 7x2:1000000:0.1,...]      (rows x cols : tiles : delta / |D x0|)
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
from bench_lm import INFINITY_CACHE, make_plan, route_bytes  # noqa: E402

DEFAULT_CASES = "7x2:1000000:0.1,8x6:250000:0.1,32x32:10000:0.1,32x32:160000:0.1,7x2:1000000:2,7x2:10000:0.1"


def bench_case(ctx, B, r, c, factor, repeats, max_sets, log):
    lib, dev = capi.lib(), ctx.device
    ctx.use_current_stream()
    plan = make_plan(ctx, B, r, c)
    nsets = min(max_sets, max(2, math.ceil(2 * INFINITY_CACHE / (B * route_bytes(r, c)["lm_solve + sums"]))))
    g = torch.Generator(device=dev); g.manual_seed(4321 + r * 100 + c)
    f64 = dict(dtype=torch.float64, device=dev)
    lo, hi = (-1.0, 1.0) if c == 32 else (0.5, 5.0)
    nr = B * (c * (c + 1) // 2)
    rv = torch.empty(nsets, nr, **f64)
    perm = torch.empty(nsets, B * c, dtype=torch.int32, device=dev)
    y, diag, x = torch.empty(nsets, B * c, **f64), torch.empty(nsets, B * c, **f64), torch.empty(nsets, B * c, **f64)
    sums = torch.empty(4, **f64)
    delta_d, par_d = torch.empty(nsets, **f64), torch.zeros(nsets, **f64)
    iters_d = torch.zeros(nsets, dtype=torch.int32, device=dev)
    deltas = []
    for s in range(nsets):
        tiles = torch.rand(B, c, r, generator=g, **f64) * (hi - lo) + lo
        f = torch.rand(B, r, generator=g, **f64) * 2 - 1
        qtb = torch.empty(B * r, **f64)
        capi.check(lib.qrk_bd_factorize_rhs(plan, tiles.data_ptr(), f.data_ptr(), 1, rv[s].data_ptr(), perm[s].data_ptr(), None,
                                            qtb.data_ptr(), None, capi.MEM_DEVICE), ctx.handle)
        capi.check(lib.qrk_bd_r_col_norms(plan, rv[s].data_ptr(), perm[s].data_ptr(), diag[s].data_ptr(), capi.MEM_DEVICE), ctx.handle)
        torch.cuda.synchronize()
        y[s].copy_(qtb[:B * c])
        capi.check(lib.qrk_bd_lm_solve(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(), 0.0, x[s].data_ptr(),
                                       sums.data_ptr(), capi.MEM_DEVICE), ctx.handle)
        torch.cuda.synchronize()
        deltas.append(factor * math.sqrt(float(sums[0])))
        del tiles, f, qtb
    delta_d.copy_(torch.tensor(deltas, dtype=torch.float64))
    par_out, iters_out = C.c_double(0.0), C.c_int32(0)

    def host_loop(s):
        par_out.value = 0.0
        capi.check(lib.qrk_bd_lmpar(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(), deltas[s], C.byref(par_out),
                                    x[s].data_ptr(), C.byref(iters_out), None), ctx.handle)

    def enqueue(s):
        capi.check(lib.qrk_bd_lmpar_device(plan, rv[s].data_ptr(), perm[s].data_ptr(), y[s].data_ptr(), diag[s].data_ptr(),
                                           delta_d[s].data_ptr(), par_d[s].data_ptr(), x[s].data_ptr(), iters_d[s].data_ptr(), None), ctx.handle)

    def device(s):
        par_d[s].zero_()
        enqueue(s)

    # the same search: pass counts and par of the two loops on every set
    passes, same = [], True
    for s in range(nsets):
        host_loop(s)
        device(s)
        torch.cuda.synchronize()
        passes.append(iters_out.value)
        same = same and int(iters_d[s]) == iters_out.value and float(par_d[s]) == par_out.value
    graphs = []
    for s in range(nsets):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ctx.use_current_stream()
            device(s)
        ctx.use_current_stream()
        graphs.append(gr)

    def replay(s):
        graphs[s].replay()

    routes = {"lmpar (host loop)": host_loop, "lmpar_device": device, "lmpar_device, replayed": replay}
    for fn in routes.values():
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
        iters[name] = max(nsets, min(2000, int(math.ceil(200.0 / max(t, 1e-3) / nsets)) * nsets))
    times = {name: [] for name in routes}
    for rep in range(repeats):
        for name, fn in routes.items():
            times[name].append(window(fn, iters[name]))
    kernel = lib.qrk_bd_lm_kernel_name(plan).decode()
    del graphs
    torch.cuda.synchronize()
    lib.qrk_bd_plan_destroy(plan)
    log(f"\n{B} tiles of {r}x{c}, delta = {factor:g} |D x0|, diag = column norms   ({nsets} rotating sets; {kernel})")
    log(f"  {min(passes)}..{max(passes)} passes = {min(passes) + 1}..{max(passes) + 1} evaluations per call; "
        f"par and iters of the two loops bit-identical on every set: {same}")
    log(f"  {'route':<26}{'median us':>11}{'min':>9}{'max':>9}{'calls':>7}{'against the host loop':>24}")
    med = {name: statistics.median(1e3 * t for t in ts) for name, ts in times.items()}
    for name in routes:
        ts = [1e3 * t for t in times[name]]
        log(f"  {name:<26}{med[name]:>11.1f}{min(ts):>9.1f}{max(ts):>9.1f}{iters[name]:>7d}{med['lmpar (host loop)'] / med[name]:>23.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-sets", type=int, default=32)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lmpar_device.py needs the GPU: there is no CPU timing"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    ctx = qrkit_amd.Context(0)
    log("MINPACK's lmpar on the factors: the host loop against the device-side loop (tools/bench_lmpar_device.py)")
    log(f"box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the handle's stream, sets rotated past the {INFINITY_CACHE >> 20} MiB Infinity Cache (at most {args.max_sets}), "
        f"{args.repeats} interleaved repeats; us per whole call")
    last = os.environ.get("QRK_LMPAR_CONTROL") == "last"
    log("control step of qrk_bd_lmpar_device: " + ("the last-arriving workgroup of the solve (QRK_LMPAR_CONTROL=last)" if last else
                                                    "a kernel of its own behind every solve (the default)"))
    for spec in args.cases.split(","):
        shape, count, factor = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        bench_case(ctx, int(count), r, c, float(factor), args.repeats, args.max_sets, log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
