#!/usr/bin/env python3
"""Three observing bands in one render (bl_set_frequencies) against a context per band, and what the axis costs a render without it.

    python tools/gpu_frequencies.py [--res 1024] [--grid 256] [--tiers tolerant,exact] [--reps 5] [--parent TREE] [--headline-reps 3]
                                    [--step-timeout 600] [--out profiles/frequencies.json]

bench.py's workload (256^3 mock, thermal electrons, plane camera) at 86, 230 and 345 GHz. One invocation measures everything, step by
step: every step is a child process of its own (this file with --step) under a time limit of its own, and the first step that fails or
runs out of time ends the run - nothing is started on the device after it. The steps:

  bands:TIER  three ways to the three bands, each timed `reps` times after an untimed round:
                one_render        one context with the three-entry list: set-up once (bl_init, bl_set_grid), one render that integrates
                                  its geodesics (bl_set_geodesic_reuse(0)) and shades three rows;
                fresh_contexts    three contexts made by bl_init with the band as image_frequency: each its set-up and one render;
                resident          one context whose one-entry list changes from band to band: the first render integrates, the next
                                  two shade the resident records (bl_stats.geodesics_reused).
              Recorded per way: the median wall clock of the whole way and of its renders alone, (max - min) / median over the reps -
              the run-to-run spread the ratios stand beside -, bl_stats' kernel times of the renders, and how far the list render's rows
              lie from the fresh contexts' (golden_util.per_pixel_relative; bits in the exact tier).
  headline    bench.py's frame with no list set, this tree against --parent TREE (a built checkout of the parent commit): whole bench.py
              processes, alternated; `within_parent_spread` says whether this tree's median time per frame exceeds the parent's by no more
              than the parent's own min-to-max spread over its processes.

Times are host wall clock between device synchronisations unless they carry bl_stats' names. Measured, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = [8.6e10, 2.3e11, 3.45e11]


def step_bands(args, tier):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    import torch
    import bench
    import blacklight_amd as bl
    import golden_util as gu
    from blacklight_amd import mock

    params = dict(bench.WORKLOAD, camera_resolution=args.res)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    def context(p, reuse):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        ctx.set_geodesic_reuse(reuse)
        ctx.set_arithmetic(tier)
        ctx.set_grid(grid)
        return ctx

    def timed(ctx):
        t0 = clock()
        out = ctx.render()
        return (clock() - t0) * 1e3, out

    def one_render():
        t0 = clock()
        with context(params, False) as ctx:
            ctx.set_frequencies(BANDS)
            ms, out = timed(ctx)
        return dict(whole=(clock() - t0) * 1e3, renders=ms, kernel=out["stats"].ms_total, geodesic=out["stats"].ms_geodesic, n_chunks=int(out["stats"].n_chunks)), [out["image"][l] for l in range(3)]

    def fresh_contexts():
        t0 = clock()
        renders = kernel = geodesic = 0.0
        rows = []
        for hz in BANDS:
            with context(dict(params, image_frequency=hz), False) as ctx:
                ms, out = timed(ctx)
            renders, kernel, geodesic = renders + ms, kernel + out["stats"].ms_total, geodesic + out["stats"].ms_geodesic
            rows.append(out["image"][0])
        return dict(whole=(clock() - t0) * 1e3, renders=renders, kernel=kernel, geodesic=geodesic), rows

    def resident():
        t0 = clock()
        renders = kernel = geodesic = 0.0
        rows, reused = [], []
        with context(params, True) as ctx:
            for hz in BANDS:
                ctx.set_frequencies([hz])
                ms, out = timed(ctx)
                renders, kernel, geodesic = renders + ms, kernel + out["stats"].ms_total, geodesic + out["stats"].ms_geodesic
                rows.append(out["image"][0])
                reused.append(int(out["stats"].geodesics_reused))
        return dict(whole=(clock() - t0) * 1e3, renders=renders, kernel=kernel, geodesic=geodesic, geodesics_reused=reused), rows

    with context(params, False) as warm:   # (the process's first context: code objects, the runtime's pools - no way's to pay)
        timed(warm)
    ways = dict(one_render=one_render, fresh_contexts=fresh_contexts, resident=resident)
    rows = {name: way()[1] for name, way in ways.items()}   # the untimed round, whose rows are compared
    measured = {name: [] for name in ways}
    for _ in range(args.reps):
        for name, way in ways.items():   # alternated: a drift of the device's clocks falls on every way alike
            measured[name].append(way()[0])

    def summary(name, key):
        values = [m[key] for m in measured[name]]
        return dict(median=float(np.median(values)), spread=float((max(values) - min(values)) / np.median(values)))

    doc = dict(step=args.step, tier=tier, res=args.res, grid=args.grid, reps=args.reps, bands_hz=BANDS)
    for name in ways:
        doc[name] = {key + "_ms": summary(name, key) for key in ("whole", "renders", "kernel", "geodesic")}
        for extra in ("n_chunks", "geodesics_reused"):
            if extra in measured[name][-1]:
                doc[name][extra] = measured[name][-1][extra]
    for name in ("one_render", "resident"):
        doc[name]["ratio_whole_to_fresh_contexts"] = doc[name]["whole_ms"]["median"] / doc["fresh_contexts"]["whole_ms"]["median"]
        doc[name]["ratio_renders_to_fresh_contexts"] = doc[name]["renders_ms"]["median"] / doc["fresh_contexts"]["renders_ms"]["median"]
        worst = max(gu.per_pixel_relative(rows[name][l], rows["fresh_contexts"][l])[0] for l in range(3))
        doc[name]["worst_per_pixel_relative_to_fresh"] = worst
        doc[name]["same_bits_as_fresh"] = bool(all(gu.same_bits(rows[name][l], rows["fresh_contexts"][l]).all() for l in range(3)))
    doc["whole_note"] = ("whole = bl_init + bl_set_grid + the renders, inside one process whose runtime is already up; a process per band pays the "
                         "runtime's start and the reading of the snapshot besides")
    print(json.dumps(doc))


def step_headline(args):
    """bench.py processes of this tree and of the parent's, alternated"""
    import numpy as np
    rows = {"this": [], "parent": []}
    for rep in range(args.headline_reps):
        for name, tree in (("parent", args.parent), ("this", HERE)):
            done = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"],
                                  capture_output=True, text=True, cwd=os.path.abspath(tree))
            if done.returncode != 0:
                sys.exit(f"bench.py in {tree}: exit status {done.returncode}\n{done.stdout[-2000:]}{done.stderr[-2000:]}")
            line = json.loads(done.stdout.strip().splitlines()[-1])
            rows[name].append(dict(ms_per_step=line["ms_per_step"], kernel_ms_per_step=line.get("kernel_ms_per_step")))
    this, parent = [r["ms_per_step"] for r in rows["this"]], [r["ms_per_step"] for r in rows["parent"]]
    over = float(np.median(this) - np.median(parent))
    print(json.dumps(dict(step=args.step, processes_each=args.headline_reps, this=rows["this"], parent=rows["parent"], this_median_ms=float(np.median(this)),
                          parent_median_ms=float(np.median(parent)), parent_spread_ms=float(max(parent) - min(parent)), this_minus_parent_ms=over,
                          within_parent_spread=bool(over <= max(parent) - min(parent)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--tiers", default="tolerant,exact")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the headline comparison")
    ap.add_argument("--headline-reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "frequencies.json"))
    args = ap.parse_args()
    if args.step:
        kind, _, rest = args.step.partition(":")
        return step_bands(args, rest) if kind == "bands" else step_headline(args)
    steps = [f"bands:{tier}" for tier in args.tiers.split(",") if tier] + (["headline"] if args.parent else [])
    doc = dict(workload="bench.py's: 256^3 mock, thermal electrons, plane camera at r = 50; the bands 86, 230 and 345 GHz", three_bands=[])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--res", str(args.res),
               "--grid", str(args.grid), "--reps", str(args.reps), "--headline-reps", str(args.headline_reps)]
        if args.parent:
            cmd += ["--parent", args.parent]
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=HERE)
        if run.returncode != 0:   # a failed step, a time limit: nothing more is started on the device
            print(f"step {step} ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}", flush=True)
            sys.exit(run.returncode)
        row = json.loads(run.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        if step.startswith("bands"):
            doc["three_bands"].append(row)
        else:
            doc["headline_no_list_set"] = row
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:   # (after every step: a run cut short keeps what it measured)
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
