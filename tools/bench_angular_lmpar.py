#!/usr/bin/env python
"""Times MINPACK's lmpar on the factors the block-angular composition keeps, on the five shapes of
tools/bench_angular_lm_solve.py:
  (a) BlockAngularSparseQR.lmSolve(None, par) alone -- on this build and, with --parent-root DIR (a checkout of the parent commit
      with its library built), on the parent's build in a child process of the same session: lmSolve()'s body moved into the
      evaluation lmpar() shares, and this shows whether it moved in time;
  (b) one evaluation of lmpar: lmSolve()'s chain and the transposed pass behind it (qrk_bd_solve_rt, qrk_dense_gemv_t,
      qrk_dense_solve_rt, the read-back of the sums);
  (c) qrk_dense_gemv_t alone on the kept top panel (m1 x m2), with its share of the nominal 8 TB/s of HBM3E on 8 rows cols bytes,
      next to torch.mv(A.t(), w) on the same arrays (the library baseline);
  (d) a whole lmpar at delta = 0.1 || x0 ||, with its number of evaluations.
Writes the table profiles/angular_lmpar_bench.txt keeps.

Method, as tools/bench_angular_lm_solve.py: HIP events on the current stream around windows of back-to-back calls; the kept factors
of one solver per set are rotated so that their footprint exceeds the 256 MiB Infinity Cache; warm-up of every route first; repeats
with the routes interleaved, median (min-max) reported.  A call is what the Python mirror does for it, its host-side bookkeeping
and synchronisations included.

    python tools/bench_angular_lmpar.py [--out FILE] [--commit ID] [--repeats 5] [--par 0.01] [--parent-root DIR]
                                        [--shapes 2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8]
"""
import argparse
import json
import math
import os
import platform
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_BYTES_PER_S = 8.0e12
INFINITY_CACHE = 256 << 20


def kept_solvers(qrkit_amd, B, r, c, m2):
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    rows, m1 = B * r, B * c
    g = torch.Generator(device=dev); g.manual_seed(977 + r * 100 + c + m2)
    touched = 8 * 3 * m1 * (m2 + 1)
    nsets = max(2, min(12, math.ceil(2 * INFINITY_CACHE / touched)))
    brows, bcols = np.full(B, r, np.int32), np.full(B, c, np.int32)
    kept = []
    for s in range(nsets):
        t = torch.randn(B, c, r, generator=g, **f64)                                  # column-major r x c tiles
        J2 = torch.randn(m2 + 1, rows, generator=g, **f64).t()                         # [J2 | b], column-major
        solver = qrkit_amd.BlockAngularSparseQR()
        if hasattr(solver, "setLmRoute"):          # (the parent build of --parent-root may be older than the routes)
            solver.setLmRoute("stacked")           # K12's chain, the one the committed table measures (tools/bench_angular_lm_reduced.py: K13's)
        solver.computeAndSolve(qrkit_amd.BlockMatrix1x2(qrkit_amd.SparseBlockDiagonal.fromTiles(brows, bcols, t.reshape(-1)), J2[:, :m2]),
                               J2[:, m2].contiguous())
        kept.append(solver)
    return kept


def window(fn, nsets, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters       # ms per call


def measure(routes, nsets, repeats):
    """{name: (list of ms per call, calls per window)}: warm-up on every set, windows of about 0.1 s, interleaved repeats"""
    for fn in routes.values():
        window(fn, nsets, nsets)
    torch.cuda.synchronize()
    iters = {}
    for name, fn in routes.items():
        t = window(fn, nsets, nsets)
        iters[name] = max(nsets, min(100 * nsets, int(math.ceil(100.0 / max(t, 1e-3) / nsets)) * nsets))
    times = {name: [] for name in routes}
    for rep in range(repeats):
        for name, fn in routes.items():
            times[name].append(window(fn, nsets, iters[name]))
    return {name: (times[name], iters[name]) for name in routes}


def lmsolve_only(root, shapes, par, repeats):
    """(a) on the package under `root`: one JSON line per shape (the child process of --parent-root, and this build's own figure)"""
    sys.path.insert(0, root)
    import qrkit_amd
    out = {}
    for spec, (B, r, c, m2) in shapes.items():
        kept = kept_solvers(qrkit_amd, B, r, c, m2)
        for s in kept:
            s.lmSolve(None, par)
        res = measure({"a": lambda s: kept[s].lmSolve(None, par)}, len(kept), repeats)
        out[spec] = [1e3 * t for t in res["a"][0]]
        del kept
        torch.cuda.empty_cache()
    return out


def bench_shape(qrkit_amd, spec, B, r, c, m2, par, repeats, parent, log):
    capi = qrkit_amd._capi
    lib = capi.lib()
    rows, m1 = B * r, B * c
    kept = kept_solvers(qrkit_amd, B, r, c, m2)
    nsets = len(kept)
    deltas = []
    for s in kept:                                                                     # (the kept arrays of every solver exist)
        deltas.append(0.1 * float(torch.linalg.vector_norm(s.lmSolve(None, 0.0))))
        s._lm_evaluate(None, par, True)
    x, pv, iters = kept[0].lmpar(None, deltas[0])
    kernel = lib.qrk_bd_solve_rt_kernel_name(kept[0].m_leftSolver._plan).decode()
    dev = torch.device("cuda", 0)
    outs = torch.empty(m2, dtype=torch.float64, device=dev)
    evals = [0, 0]                                     # evaluations, calls of route (d)

    def lm_step(s):
        kept[s].lmSolve(None, par)

    def eval_step(s):
        kept[s]._lm_evaluate(None, par, True)

    def gemv_step(s):
        k = kept[s]
        lm = k._lm
        capi.check(lib.qrk_dense_gemv_t(k._ctx.handle, lm["top"].data_ptr(), m1, m1, m2, None, lm["w1"].data_ptr(), 1.0, None, outs.data_ptr(),
                                        lm["work"].data_ptr()), k._ctx.handle)

    def mv_step(s):
        lm = kept[s]._lm
        torch.mv(lm["top"][:, :m2].t(), lm["w1"], out=outs)

    def lmpar_step(s):
        evals[0] += kept[s].lmpar(None, deltas[s])[2] + 1
        evals[1] += 1

    gemv_step(0)
    got = outs.clone()
    mv_step(0)
    rel = float((got - outs).norm() / outs.norm())
    routes = {"(a) lmSolve()": lm_step, "(b) one lmpar evaluation": eval_step, "(c) qrk_dense_gemv_t alone": gemv_step,
              "(c') torch.mv(A.t(), w)": mv_step, "(d) lmpar at 0.1 |x0|": lmpar_step}
    res = measure(routes, nsets, repeats)
    log(f"\n{B} blocks of {r}x{c} next to {m2} dense columns ({rows} rows; par {par:g}; {nsets} rotating sets; kernel of the tile pass: {kernel}; "
        f"gemv_t on {m1} x {m2}, against torch.mv {rel:.1e}; lmpar of set 0: par {pv:.3e} after {iters + 1} evaluations)")
    log(f"  {'route':<34}{'median us':>11}{'min':>10}{'max':>10}{'spread':>8}{'calls':>7}")
    med = {}
    for name, (ts, n) in res.items():
        ts = [1e3 * t for t in ts]
        med[name] = statistics.median(ts)
        log(f"  {name:<34}{med[name]:>11.1f}{min(ts):>10.1f}{max(ts):>10.1f}{(max(ts) - min(ts)) / med[name]:>8.1%}{n:>7d}")
    if parent is not None:
        ts = parent[spec]
        m = statistics.median(ts)
        mine = [1e3 * t for t in res["(a) lmSolve()"][0]]
        overlap = not (max(mine) < min(ts) or min(mine) > max(ts))
        log(f"  {'(a) lmSolve(), the parent build':<34}{m:>11.1f}{min(ts):>10.1f}{max(ts):>10.1f}{(max(ts) - min(ts)) / m:>8.1%}")
        log(f"  lmSolve() of this build against the parent's: {med['(a) lmSolve()'] / m:.3f} of its time "
            f"({'the repeats overlap' if overlap else 'the repeats do not overlap'})")
    t_gemv, t_mv = med["(c) qrk_dense_gemv_t alone"], med["(c') torch.mv(A.t(), w)"]
    rate = 8.0 * m1 * m2 / (t_gemv * 1e-6)
    log(f"  qrk_dense_gemv_t alone: {8.0 * m1 * m2 / 2**20:.1f} MiB, {rate / 1e12:.2f} TB/s = {rate / HBM_BYTES_PER_S:.2f} of 8 TB/s; "
        f"torch.mv takes {t_mv / t_gemv:.2f}x its time")
    log(f"  the transposed pass costs (b) - (a) = {med['(b) one lmpar evaluation'] - med['(a) lmSolve()']:.1f} us per evaluation; "
        f"(d) ran {evals[0] / max(1, evals[1]):.2f} evaluations per call on average")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--par", type=float, default=1e-2)
    ap.add_argument("--shapes", default="2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: (a) is timed there too")
    ap.add_argument("--lmsolve-only", default=None, help="(internal) time (a) on the package under this root and print JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_angular_lmpar.py needs the GPU: there is no CPU timing"
    shapes = {}
    for spec in args.shapes.split(","):
        shape, count, m2 = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        shapes[spec] = (int(count), r, c, int(m2))
    if args.lmsolve_only:
        print("JSON " + json.dumps(lmsolve_only(args.lmsolve_only, shapes, args.par, args.repeats)), flush=True)
        return
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                              # (kept up to date: a long shape must not lose the ones before it)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    parent = None
    if args.parent_root:                          # a fresh child process: the parent's package and library, nothing of this build
        env = dict(os.environ)
        env.pop("QRKIT_AMD_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lmsolve-only", os.path.abspath(args.parent_root), "--shapes", args.shapes,
                              "--par", str(args.par), "--repeats", str(args.repeats)], capture_output=True, text=True, env=env, check=True)
        parent = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("JSON ")][-1][5:])
    sys.path.insert(0, os.path.dirname(HERE))
    import qrkit_amd
    import datetime
    log("MINPACK's lmpar on the kept factors of the block-angular composition: lmSolve(), one evaluation, gemv_t alone, a whole lmpar "
        "(tools/bench_angular_lmpar.py)")
    log(f"date: {datetime.date.today().isoformat()}; box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the current stream, kept factors rotated past the {INFINITY_CACHE >> 20} MiB Infinity Cache, {args.repeats} interleaved repeats")
    for spec, (B, r, c, m2) in shapes.items():
        bench_shape(qrkit_amd, spec, B, r, c, m2, args.par, args.repeats, parent, log)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
