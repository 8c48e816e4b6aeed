#!/usr/bin/env python
"""Times the two routes of the damped solve on the kept block-angular factors: "stacked" factorises the
(m1 + 2 m2) x m2 right stack with the fill in it (K11), "reduced" first reduces the fill to one triangle with qrk_dense_qless_r.
  (a) BlockAngularSparseQR.lmSolve(None, par) on "stacked" and on "reduced", alternating in one process, and -- with --parent-root DIR,
      a checkout of the parent commit with its library built -- on the parent's build in a child process of the same session;
  (b) qrk_dense_qless_r alone on the kept fill (m1 x (m2 + 1)), with its share of the nominal 8 TB/s on 8 rows cols bytes;
  (c) lmSolve(None, 0.0) -- par = 0 exactly -- against lmSolve(None, par) on both routes (K12's penalty of the evaluation every
      lmpar starts with);
  (d) a whole lmpar at delta = 0.1 || x0 || on both routes, with the evaluations per call.
Shapes with m2 > 31 are not eligible for the reduced route: only "stacked" and the parent are timed there.
Writes the table profiles/angular_lm_reduced_bench.txt keeps.

Method, as tools/bench_angular_lm_solve.py and tools/bench_angular_lmpar.py (whose helpers this tool uses): HIP events on the current
stream around windows of back-to-back calls; the kept factors of one solver per set are rotated so that their footprint exceeds the
256 MiB Infinity Cache; warm-up of every route first; repeats with the routes interleaved, median (min-max) reported.

    python tools/bench_angular_lm_reduced.py [--out FILE] [--commit ID] [--repeats 5] [--par 0.01] [--parent-root DIR]
                                [--shapes 2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8,7x2:100000:31]
"""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_angular_lmpar as base  # noqa: E402

HBM_BYTES_PER_S = base.HBM_BYTES_PER_S


def bench_shape(qrkit_amd, spec, B, r, c, m2, par, repeats, parent, log):
    capi = qrkit_amd._capi
    lib = capi.lib()
    rows, m1 = B * r, B * c
    kept = base.kept_solvers(qrkit_amd, B, r, c, m2)          # (every solver on "stacked")
    nsets = len(kept)
    eligible = m2 + 1 <= 32
    names = ("stacked", "reduced") if eligible else ("stacked",)
    deltas, rel = [], 0.0
    for s in kept:                                            # the kept arrays of every solver on every route exist
        for route in names:
            s.setLmRoute(route)
            x = s.lmSolve(None, par)
            s._lm_evaluate(None, par, True)
            if route == "stacked":
                xs = x
                deltas.append(0.1 * float(torch.linalg.vector_norm(s.lmSolve(None, 0.0))))
            else:
                rel = max(rel, float((x - xs).norm() / xs.norm()))
    evals = {n: [0, 0] for n in names}

    def lm_step(route, pv):
        def step(s):
            kept[s].setLmRoute(route)
            kept[s].lmSolve(None, pv)
        return step

    def lmpar_step(route):
        def step(s):
            kept[s].setLmRoute(route)
            evals[route][0] += kept[s].lmpar(None, deltas[s])[2] + 1
            evals[route][1] += 1
        return step

    def qless_step(s):
        k = kept[s]
        lm = k._lm_routes["reduced"]
        capi.check(lib.qrk_dense_qless_r(k._ctx.handle, lm["F"].data_ptr(), max(m1, 1), m1, m2 + 1, lm["G"].data_ptr() + 8 * m2, 3 * m2 + 1,
                                         lm["qwork"].data_ptr()), k._ctx.handle)

    routes = {}
    for n in names:
        routes[f"(a) lmSolve(par), {n}"] = lm_step(n, par)
    if eligible:
        routes["(b) qrk_dense_qless_r alone"] = qless_step
    for n in names:
        routes[f"(c) lmSolve(0), {n}"] = lm_step(n, 0.0)
    for n in names:
        routes[f"(d) lmpar at 0.1 |x0|, {n}"] = lmpar_step(n)
    res = base.measure(routes, nsets, repeats)
    kernel = lib.qrk_dense_qless_r_kernel_name(m1, m2 + 1).decode() if eligible else "(not eligible: m2 + 1 > 32)"
    lr, lc = (capi.C.c_int64 * 4)(), (capi.C.c_int64 * 4)()
    nl = lib.qrk_dense_qless_r_levels(m1, m2 + 1, lr, lc, 4) if eligible else 0
    log(f"\n{B} blocks of {r}x{c} next to {m2} dense columns ({rows} rows; par {par:g}; {nsets} rotating sets; fill {m1} x {m2 + 1}; {kernel}; "
        f"levels {list(lr[:nl])} in chunks {list(lc[:nl])}; x of the two routes differs by {rel:.1e})")
    log(f"  {'route':<36}{'median us':>11}{'min':>10}{'max':>10}{'spread':>8}{'calls':>7}")
    med, us = {}, {}
    for name, (ts, n) in res.items():
        us[name] = [1e3 * t for t in ts]
        med[name] = statistics.median(us[name])
        log(f"  {name:<36}{med[name]:>11.1f}{min(us[name]):>10.1f}{max(us[name]):>10.1f}{(max(us[name]) - min(us[name])) / med[name]:>8.1%}{n:>7d}")
    a_s = "(a) lmSolve(par), stacked"
    if parent is not None:
        ts = parent[spec]
        m = statistics.median(ts)
        overlap = not (max(us[a_s]) < min(ts) or min(us[a_s]) > max(ts))
        log(f"  {'(a) lmSolve(par), the parent build':<36}{m:>11.1f}{min(ts):>10.1f}{max(ts):>10.1f}{(max(ts) - min(ts)) / m:>8.1%}")
        log(f"  stacked on this build against the parent's lmSolve(): {med[a_s] / m:.3f} of its time "
            f"({'the repeats overlap' if overlap else 'the repeats do not overlap'})")
    if eligible:
        a_r = "(a) lmSolve(par), reduced"
        clear = max(us[a_r]) < min(us[a_s])
        log(f"  reduced against stacked: {med[a_s] / med[a_r]:.2f}x ({'every repeat of reduced is faster than every repeat of stacked' if clear else 'NOT every repeat of reduced is faster than every repeat of stacked'})")
        t = med["(b) qrk_dense_qless_r alone"]
        rate = 8.0 * m1 * (m2 + 1) / (t * 1e-6)
        log(f"  qrk_dense_qless_r alone: {8.0 * m1 * (m2 + 1) / 2**20:.1f} MiB, {rate / 1e12:.3f} TB/s = {rate / HBM_BYTES_PER_S:.3f} of 8 TB/s")
    for n in names:
        log(f"  par = 0 exactly against par = {par:g}, {n}: {med[f'(c) lmSolve(0), {n}'] / med[f'(a) lmSolve(par), {n}']:.2f}x; "
            f"lmpar ran {evals[n][0] / max(1, evals[n][1]):.2f} evaluations per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--par", type=float, default=1e-2)
    ap.add_argument("--shapes", default="2x1:500000:5,7x2:250000:8,7x2:1024:384,7x2:20000:384,8x6:100000:8,7x2:100000:31")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: (a) is timed there too")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_angular_lm_reduced.py needs the GPU: there is no CPU timing"
    shapes = {}
    for spec in args.shapes.split(","):
        shape, count, m2 = spec.split(":")
        r, c = (int(v) for v in shape.split("x"))
        shapes[spec] = (int(count), r, c, int(m2))
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
        out = subprocess.run([sys.executable, os.path.join(HERE, "bench_angular_lmpar.py"), "--lmsolve-only", os.path.abspath(args.parent_root),
                              "--shapes", args.shapes, "--par", str(args.par), "--repeats", str(args.repeats)],
                             capture_output=True, text=True, env=env, check=True)
        parent = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("JSON ")][-1][5:])
    sys.path.insert(0, os.path.dirname(HERE))
    import qrkit_amd
    import datetime
    log("The damped solve on the kept block-angular factors, stacked against reduced: lmSolve(), qrk_dense_qless_r alone, par = 0, a whole lmpar "
        "(tools/bench_angular_lm_reduced.py)")
    log(f"date: {datetime.date.today().isoformat()}; box: {platform.node()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; commit: {args.commit}")
    log(f"HIP events on the current stream, kept factors rotated past the {base.INFINITY_CACHE >> 20} MiB Infinity Cache, {args.repeats} interleaved repeats")
    for spec, (B, r, c, m2) in shapes.items():
        bench_shape(qrkit_amd, spec, B, r, c, m2, args.par, args.repeats, parent, log)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
