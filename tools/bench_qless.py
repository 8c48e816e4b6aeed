#!/usr/bin/env python
"""Times factorise-and-solve WITHOUT Q (qrk_bd_factorize_rhs, nrhs = 1) against the two-call explicit-Q route
(qrk_bd_factorize + qrk_bd_solve) on the same box and the same inputs, and writes the table that profiles/qless_bench.txt keeps.

Method: HIP events on the handle's stream around a window of back-to-back calls; the input / output sets of a route are
rotated so that the footprint of a window exceeds the 256 MiB Infinity Cache (no call finds its data there); warm-up of
every route first; five repeats with the routes interleaved (A B C A B C ...), median and spread reported.  Bytes per tile
are the algorithmic ones (what the route must move, from the shapes), the rate is those bytes over the measured time, the
fraction is of the nominal 8 TB/s of HBM3E.

    python tools/bench_qless.py [--out FILE] [--commit ID] [--shapes 7x2:1000000,9x2:1000000,32x32:10000,32x32:160000]
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


def route_bytes(r, c):
    """Algorithmic bytes per tile and right-hand side of each route."""
    tile, q, rr, perm, b, x = 8 * r * c, 8 * r * r, 8 * (c * (c + 1) // 2), 4 * c, 8 * r, 8 * c
    return {
        "factorize+solve": (tile + q + rr + perm) + (q + rr + perm + b + x),       # Q written once and read back once
        "factorize_rhs x": tile + b + rr + perm + x,
        "factorize_rhs x+qtb": tile + b + rr + perm + x + b,
    }


def bench_shape(ctx, B, r, c, repeats, log):
    lib, dev = capi.lib(), ctx.device
    lay = capi.BDLayout()
    lay.num_blocks, lay.block_rows, lay.block_cols = B, r, c
    lay.rows = lay.cols = None
    lay.mat_rows, lay.mat_cols = B * r, B * c
    plan = C.c_void_p()
    capi.check(lib.qrk_bd_plan_create(ctx.handle, C.byref(lay), capi.FULL_Q, capi.COLPIV_HOUSEHOLDER, C.byref(plan)), ctx.handle)
    nbytes = route_bytes(r, c)
    # sets: the smallest route's window must pass the cache twice over
    nsets = max(2, math.ceil(2 * INFINITY_CACHE / (B * nbytes["factorize_rhs x"])))
    g = torch.Generator(device=dev); g.manual_seed(1234 + r * 100 + c)
    f64 = dict(dtype=torch.float64, device=dev)
    tiles = torch.rand(nsets, B * r * c, generator=g, **f64) * 4.5 + 0.5
    rhs = torch.rand(nsets, B * r, generator=g, **f64) * 2 - 1
    q = torch.empty(nsets, B * r * r, **f64)
    rv = torch.empty(nsets, B * (c * (c + 1) // 2), **f64)
    perm = torch.empty(nsets, B * c, dtype=torch.int32, device=dev)
    x = torch.empty(nsets, B * c, **f64)
    y = torch.empty(nsets, B * r, **f64)
    x_ref = torch.empty(B * c, **f64)

    def parent(s):
        capi.check(lib.qrk_bd_factorize(plan, tiles[s].data_ptr(), q[s].data_ptr(), rv[s].data_ptr(), perm[s].data_ptr(), None,
                                        capi.MEM_DEVICE), ctx.handle)
        capi.check(lib.qrk_bd_solve(plan, q[s].data_ptr(), rv[s].data_ptr(), perm[s].data_ptr(), rhs[s].data_ptr(), 1, x[s].data_ptr(),
                                    capi.MEM_DEVICE), ctx.handle)

    def fused(s, with_qtb):
        capi.check(lib.qrk_bd_factorize_rhs(plan, tiles[s].data_ptr(), rhs[s].data_ptr(), 1, rv[s].data_ptr(), perm[s].data_ptr(), None,
                                            y[s].data_ptr() if with_qtb else None, x[s].data_ptr(), capi.MEM_DEVICE), ctx.handle)

    routes = {"factorize+solve": parent, "factorize_rhs x": lambda s: fused(s, False), "factorize_rhs x+qtb": lambda s: fused(s, True)}
    # same answer first (and the warm-up of every route on every set)
    parent(0); x_ref.copy_(x[0]); perm_ref = perm[0].clone()
    fused(0, True)
    torch.cuda.synchronize()
    assert torch.equal(perm[0], perm_ref), "the routes disagree on the permutation"
    rel = float((x[0] - x_ref).norm() / x_ref.norm())
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
    kernel = lib.qrk_bd_rhs_kernel_name(plan, 1).decode()
    lib.qrk_bd_plan_destroy(plan)
    log(f"\n{B} tiles of {r}x{c}, nrhs = 1   ({nsets} rotating sets; x of the two routes differs by {rel:.1e}; kernel: {kernel})")
    log(f"  {'route':<22}{'median us':>11}{'min':>9}{'max':>9}{'spread':>8}{'calls':>7}{'B/tile':>8}{'GB/s':>8}{'of 8 TB/s':>10}")
    med = {}
    for name in routes:
        ts = [1e3 * t for t in times[name]]
        med[name] = statistics.median(ts)
        rate = B * nbytes[name] / (med[name] * 1e-6)
        log(f"  {name:<22}{med[name]:>11.1f}{min(ts):>9.1f}{max(ts):>9.1f}{(max(ts) - min(ts)) / med[name]:>8.1%}{iters[name]:>7d}"
            f"{nbytes[name]:>8d}{rate / 1e9:>8.0f}{rate / HBM_BYTES_PER_S:>10.1%}")
    for name in ("factorize_rhs x", "factorize_rhs x+qtb"):
        ts_new, ts_old = times[name], times["factorize+solve"]
        clear = max(ts_new) < min(ts_old)
        log(f"  {name} against factorize+solve: {med['factorize+solve'] / med[name]:.2f}x"
            f" ({'every repeat faster than every repeat of the two-call route' if clear else 'NOT clear of the run-to-run spread'})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="7x2:1000000,9x2:1000000,32x32:10000,32x32:160000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qless.py needs the GPU: there is no CPU timing"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    ctx = qrkit_amd.Context(0)
    log("Q-less factorise-and-solve against the explicit-Q two-call route (tools/bench_qless.py)")
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
