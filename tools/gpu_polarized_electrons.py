"""Polarized variants with an electron distribution each in one render (bl_set_polarized_variants_electrons) against one fresh render
per variant, and what the per-variant electron constants cost the renders that do not use them.

    python tools/gpu_polarized_electrons.py [--res 1024] [--grid 256] [--variants 2,6] [--tiers exact,tolerant] [--reps 5]
                                            [--parent TREE] [--rounds 3] [--compare ...] [--step-timeout 600] [--append]
                                            [--out profiles/polarized_electrons.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), full Stokes and the optical-depth row, 230 GHz: bench.py's polarized1024
workload, as tools/gpu_polarized_cuts.py renders it. One invocation measures everything, step by step: every step is a child process
of its own (this file with --step, or bench.py) under a time limit of its own, and the first step that fails or runs out of time ends
the run - nothing is started on the device after it. The steps:

  gain:V:TIER          V tuples whose mixes differ - thermal, kappa_own, power, mix, kappa_low, all_kappa, over the triples of
                       tools/gpu_polarized_variants.py - in one render, against V renders, each in a context of its own with that tuple in
                       its parameter block: what a library over the electron distribution costs without the call. The two are
                       alternated `reps` times; medians are compared, and the fresh renders' own run-to-run spread - (max - min) /
                       median of their per-repetition sums - is recorded beside the ratio. Every variant's rows are compared with its
                       fresh render's bit for bit.
  thermal:6:TIER       six thermal triples with no mixes set: the thermal-only kernel, which must not pay for a table it does not read;
  kappa_block:1:TIER   one render with kappa_own in the parameter block and no variants: the all-electrons kernel outside variant mode,
                       which now chooses between its own arguments and a table;
  bench:WORKLOAD       bench.py --workload polarized1024, and the default workload.
The last three run in this tree and, with --parent TREE (a built checkout of the parent commit), in that one. A process measures
`reps` repetitions, a repetition the median of five timed renders, and the two trees alternate for `rounds` processes each: the scatter
from one process to the next is several times the scatter within one. `within_parent_spread` says whether the median of this tree's
processes exceeds the median of the parent's by no more than the min-to-max spread of the parent's processes.

Both sides of a comparison integrate their geodesics (bl_set_geodesic_reuse(0)); bl_set_grid is outside the timed region, and every
timed render follows an untimed one of the same context. Times are host wall clock between device synchronisations.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("BLACKLIGHT_AMD_TREE", HERE)   # (a --step child of the parent's measurement imports the parent's package)

MIXES = [
    ("thermal", dict(power_frac=0.0, kappa_frac=0.0)),
    ("kappa_own", dict(power_frac=0.0, kappa_frac=0.4, kappa=4.0, w=1.5)),
    ("power", dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0)),
    ("mix", dict(power_frac=0.2, p=3.0, gamma_min=3.0, gamma_max=500.0, kappa_frac=0.25, kappa=4.3, w=2.5)),
    ("kappa_low", dict(power_frac=0.0, kappa_frac=0.49, kappa=3.5, w=1.919106339654944)),
    ("all_kappa", dict(power_frac=0.0, kappa_frac=1.0, kappa=4.5, w=1.0)),
]


def triple_sweep(rho0, v):
    """(R_low, R_high, unit) x v: tools/gpu_polarized_variants.py's"""
    import numpy as np
    if v == 1:
        return [(1.0, 40.0, 2.0 * rho0)]
    highs = np.geomspace(1.0, 160.0, v)
    units = np.geomspace(0.1 * rho0, 10.0 * rho0, v)[::-1]
    return [(1.0, float(h), float(u)) for h, u in zip(highs, units)]


def run_step(args):
    """--step: one measurement in this process; prints one JSON line"""
    sys.path.insert(0, TREE)
    sys.path.insert(0, os.path.join(TREE, "tests"))
    import numpy as np
    import torch
    import bench
    import blacklight_amd as bl
    from blacklight_amd import mock

    params = dict(bench.WORKLOAD, camera_resolution=args.res, image_polarization=True, image_tau=True)
    rho0 = float(params["simulation_rho_cgs"])
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    kind, size, tier = args.step.split(":")

    def context(p):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        ctx.set_geodesic_reuse(False)
        ctx.set_arithmetic(tier)
        ctx.set_grid(grid)
        return ctx

    def timed(ctx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if kind in ("thermal", "kappa_block"):
        if kind == "thermal":
            triples = triple_sweep(rho0, int(size))
            ctx = context(params)
            ctx.set_polarized_variants([h for _, h, _ in triples], [u for _, _, u in triples], rat_low=[lo for lo, _, _ in triples])
        else:
            triples = []
            ctx = context(dict(params, plasma_kappa_frac=0.4, plasma_kappa=4.0, plasma_w=1.5))
        timed(ctx)
        reps, st = [], None
        for rep in range(args.reps):
            times = []
            for _ in range(5):
                ms, out = timed(ctx)
                times.append(ms)
            st = out["stats"]
            reps.append(float(np.median(times)))
        ctx.close()
        print(json.dumps(dict(step=args.step, tier=tier, n_variants=max(1, len(triples)), rep_ms=reps, median_ms=float(np.median(reps)),
                              spread_ms=float(max(reps) - min(reps)), launches_shade=st.launches_shade, launches_transfer=st.launches_transfer,
                              n_chunks=st.n_chunks, ms_shade=st.ms_shade, ms_transfer=st.ms_transfer, ms_geodesic=st.ms_geodesic)))
        return
    import golden_util as gu
    n = int(size)
    triples = triple_sweep(rho0, n)
    names = [MIXES[v % len(MIXES)][0] for v in range(n)]
    mixes = [MIXES[v % len(MIXES)][1] for v in range(n)]
    multi = context(params)
    multi.set_polarized_variants([h for _, h, _ in triples], [u for _, _, u in triples], rat_low=[lo for lo, _, _ in triples], electrons=mixes)
    timed(multi)   # (warm-up)
    multi_ms, fresh_sum_ms, fresh_each_ms = [], [], []
    fresh_images = [None] * n
    got = fresh_stats = None
    for rep in range(args.reps):
        timed(multi)   # (each timed render right behind one of its own, as for the fresh contexts below)
        ms, got = timed(multi)
        multi_ms.append(ms)
        each = []
        for v, (low, high, unit) in enumerate(triples):
            block = {"plasma_" + key: value for key, value in mixes[v].items()}
            one = context(dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit, **block))
            timed(one)   # (warm-up: a context's first render allocates its scratch)
            ms, out = timed(one)
            each.append(ms)
            fresh_images[v] = out["image"]
            fresh_stats = out["stats"]
            one.close()
        fresh_each_ms.append(each)
        fresh_sum_ms.append(sum(each))
    st = got["stats"]
    same = [bool(gu.same_bits(got["image_by_variant"][v], fresh_images[v]).all()) for v in range(n)]
    multi.close()
    fresh_median = float(np.median(fresh_sum_ms))
    spread = float((max(fresh_sum_ms) - min(fresh_sum_ms)) / fresh_median)
    ratio = float(np.median(multi_ms) / fresh_median)
    print(json.dumps(dict(step=args.step, tier=tier, n_variants=n, mixes=names, triples=triples, multi_ms=multi_ms, fresh_sum_ms=fresh_sum_ms,
                          fresh_each_ms=fresh_each_ms, multi_median_ms=float(np.median(multi_ms)), fresh_median_ms=fresh_median, ratio=ratio,
                          multi_spread=float((max(multi_ms) - min(multi_ms)) / np.median(multi_ms)), fresh_spread=spread,
                          ahead_by_more_than_the_spread=bool(1.0 - ratio > spread),
                          arithmetic=st.arithmetic, n_chunks=st.n_chunks, launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade,
                          launches_transfer=st.launches_transfer, ms_geodesic=st.ms_geodesic, ms_locate=st.ms_locate, ms_shade=st.ms_shade,
                          ms_transfer=st.ms_transfer, fresh_n_chunks=fresh_stats.n_chunks, fresh_ms_geodesic=fresh_stats.ms_geodesic,
                          fresh_ms_shade=fresh_stats.ms_shade, fresh_ms_transfer=fresh_stats.ms_transfer, same_bits=same, all_same_bits=all(same))))


def document(res, grid, results):
    """The profile: the gain rows as measured, and every comparison against the parent summed up over its processes"""
    doc = dict(res=res, grid=grid, results=[r for r in results if r["step"].startswith("gain")])
    rows = [r for r in results if not r["step"].startswith("gain")]
    if rows:
        doc["against_parent"] = dict(rows=rows)
        for step in sorted({r["step"] for r in rows}):
            ours = [r["median_ms"] for r in rows if r["step"] == step and r["tree"] == "this"]
            theirs = [r["median_ms"] for r in rows if r["step"] == step and r["tree"] == "parent"]
            if ours and theirs:
                over = statistics.median(ours) - statistics.median(theirs)
                doc["against_parent"][step] = dict(this_process_ms=ours, parent_process_ms=theirs, this_ms=statistics.median(ours),
                                                   parent_ms=statistics.median(theirs), this_spread_ms=max(ours) - min(ours),
                                                   parent_spread_ms=max(theirs) - min(theirs), this_minus_parent_ms=over,
                                                   within_parent_spread=bool(over <= max(theirs) - min(theirs)))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--variants", default="2,6")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the comparisons against it")
    ap.add_argument("--rounds", type=int, default=3, help="processes per tree of a comparison against the parent, alternating")
    ap.add_argument("--compare", default="thermal:6,kappa_block:1,bench:polarized1024,bench:benchmark", help="the comparisons against the parent ('' for none)")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None)
    ap.add_argument("--append", action="store_true", help="keep what --out already holds (the steps of an earlier invocation) and add to it")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "polarized_electrons.json"))
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    trees = ([("parent", args.parent)] if args.parent else []) + [("this", HERE)]
    steps = []
    for tier in args.tiers.split(","):
        steps += [(f"gain:{v}:{tier}", "this", HERE) for v in args.variants.split(",") if v]
    for case in [c for c in args.compare.split(",") if c]:
        tiers = ["-"] if case.startswith("bench:") else args.tiers.split(",")
        for tier in tiers:
            for _ in range(args.rounds if args.parent else 1):
                steps += [(case if tier == "-" else f"{case}:{tier}", name, tree) for name, tree in trees]
    results = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            held = json.load(f)
        results = held.get("results", []) + held.get("against_parent", {}).get("rows", [])

    def save():   # (after every step: a run cut short keeps what it measured)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(document(args.res, args.grid, results), f, indent=1)

    for step, name, tree in steps:
        tree = os.path.abspath(tree)
        if step.startswith("bench:"):
            workload = step.split(":")[1]
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps),
                   "--warmup", "2", "--no-cpu-baseline", "--resolution", str(args.res), "--grid", str(args.grid)] + (["--workload", workload] if workload != "benchmark" else [])
        else:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--res", str(args.res),
                   "--grid", str(args.grid), "--reps", str(args.reps)]
        run = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, BLACKLIGHT_AMD_TREE=tree), cwd=tree)
        if run.returncode != 0:   # a failed step, a time limit: nothing more is started on the device
            print(f"step {step} ({tree}) ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}", flush=True)
            sys.exit(run.returncode)
        row = json.loads(run.stdout.strip().splitlines()[-1])
        if step.startswith("bench:"):
            row = dict(step=step, median_ms=float(row["ms_per_step"]), value=row.get("value"), unit=row.get("unit"))
        row["tree"] = name
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ("triples", "fresh_each_ms", "same_bits")}), flush=True)
        save()


if __name__ == "__main__":
    main()
