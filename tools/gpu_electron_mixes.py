"""Several electron mixes of an unpolarized run in one render (bl_set_electron_mixes) against one fresh render per mix, and what the axis
costs a render that does not use it.

    python tools/gpu_electron_mixes.py [--res 1024] [--grid 256] [--mixes 2,6,16] [--tiers exact,tolerant] [--parent TREE]
                                       [--runs 3] [--step-timeout 900] [--out profiles/electron_mixes.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), 230 GHz: bench.py's default workload. One invocation measures everything, step
by step: every step is a child process of its own (this file with --step) under a time limit of its own, and the first step that fails or
runs out of time ends the run - nothing is started on the device after it. The steps:

  mixes:E:TIER   one render of E mixes (the first thermal, the others power laws of rising share and slope) against E renders, each in a
                 context of its own with that mix in its parameter block - what a library over the electron distribution costs without
                 the call. Medians of five timed renders on either side, with the min-to-max spread of each side; the per-pixel distance
                 of every mix's rows from its fresh render (gu.per_pixel_relative; the exact tier: the same bits).
  unused:NAME    a render that sets no list, in this tree and, with --parent TREE (a built checkout of the parent commit), in that one,
                 alternating: three processes per tree. NAME is `frame` (bench.py's workload), `truecolor` (bench.py --workload
                 truecolor1024x64) or `models6` (six electron models in the tolerant tier's one pass). `within_parent_spread` says whether
                 this tree's median exceeds the parent's by no more than the parent's own min-to-max spread over its processes.
  runs           one render of a list that the tolerant tier renders run by run (thermal, three power laws, a mix without a thermal part:
                 three runs, a pass per variant), in this tree and in --parent's like `unused`: --runs processes per tree, alternating, each
                 the median wall time of bl_render over five renders; geodesic reuse as a context starts with it.

Both sides of a mixes comparison integrate their geodesics (bl_set_geodesic_reuse(0)); bl_set_grid is outside the timed region, and
every timed render follows an untimed one of the same context (the first render of a context allocates its scratch). Times are host wall
clock between device synchronisations.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("BLACKLIGHT_AMD_TREE", HERE)   # (a --step child of the parent's measurement imports the parent's package)


def mix_sweep(k):
    """The first mix thermal, then power laws: the share 0.02 ... 0.5, the slope 2.2 ... 3.5, gamma_min 1 ... 10"""
    import numpy as np
    mixes = [dict(power_frac=0.0, p=2.5, gamma_min=1.0, gamma_max=1000.0)]
    for frac, p, low in zip(np.geomspace(0.02, 0.5, max(k - 1, 1)), np.linspace(2.2, 3.5, max(k - 1, 1)), np.geomspace(1.0, 10.0, max(k - 1, 1))):
        mixes.append(dict(power_frac=float(frac), p=float(p), gamma_min=float(low), gamma_max=1.0e4))
    return mixes[:k]


def run_step(args):
    """--step: one measurement in this process; prints one JSON line"""
    sys.path.insert(0, TREE)
    sys.path.insert(0, os.path.join(TREE, "tests"))
    import numpy as np
    import torch
    import bench
    import blacklight_amd as bl
    from blacklight_amd import mock

    kind, _, rest = args.step.partition(":")
    if kind == "unused" and rest in ("frame", "truecolor"):   # bench.py itself, one process: its JSON line
        cmd = [sys.executable, os.path.join(TREE, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline"]
        cmd += ["--workload", "truecolor1024x64"] if rest == "truecolor" else []
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=TREE)
        if run.returncode != 0:
            print(run.stdout[-2000:], run.stderr[-2000:])
            sys.exit(run.returncode)
        line = json.loads([text for text in run.stdout.splitlines() if text.startswith("{")][-1])
        ms = line.get("ms_per_step", line.get("step_ms", line.get("value")))
        print(json.dumps(dict(step=args.step, ms=ms, bench=line)))
        return

    params = dict(bench.WORKLOAD, camera_resolution=args.res)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)

    def context(p, tier, mixes=None, highs=None, reuse=False):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        if not reuse:
            ctx.set_geodesic_reuse(False)
        ctx.set_arithmetic(tier)
        ctx.set_grid(grid)
        if highs is not None:
            ctx.set_electron_models(highs, rat_low=1.0)
        if mixes is not None:
            ctx.set_electron_mixes(mixes)
        return ctx

    def timed(ctx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def five(ctx):
        timed(ctx)   # (warm-up: a context's first render allocates its scratch)
        times, out = [], None
        for _ in range(5):
            ms, out = timed(ctx)
            times.append(ms)
        return times, out

    if kind == "runs":   # a list with a mix without a thermal part: tests/test_gpu_electron_mixes.py's MIXES + [PURE]
        mixes = [dict(power_frac=0.0, p=2.5, gamma_min=1.0, gamma_max=1000.0), dict(power_frac=0.3, p=2.5, gamma_min=1.0, gamma_max=1000.0),
                 dict(power_frac=0.5, p=3.5, gamma_min=10.0, gamma_max=1.0e5), dict(power_frac=0.05, p=2.2, gamma_min=2.0, gamma_max=500.0),
                 dict(power_frac=1.0, p=2.8, gamma_min=5.0, gamma_max=1.0e4)]
        ctx = context(params, "tolerant", mixes, reuse=True)
        times, out = five(ctx)
        st = out["stats"]
        ctx.close()
        print(json.dumps(dict(step=args.step, ms=float(np.median(times)), times_ms=times, n_mixes=st.n_mixes, launches_geodesic=st.launches_geodesic,
                              launches_shade=st.launches_shade, n_chunks=st.n_chunks, arithmetic=st.arithmetic)))
        return
    if kind == "unused":   # models6: six electron models, the tolerant tier's one pass
        ctx = context(params, "tolerant", None, [float(x) for x in np.geomspace(1.0, 160.0, 6)])
        times, out = five(ctx)
        st = out["stats"]
        ctx.close()
        print(json.dumps(dict(step=args.step, ms=float(np.median(times)), times_ms=times, launches_shade=st.launches_shade, n_chunks=st.n_chunks,
                              ms_shade=st.ms_shade, ms_transfer=st.ms_transfer)))
        return
    import golden_util as gu
    size, tier = rest.split(":")
    mixes = mix_sweep(int(size))
    multi = context(params, tier, mixes)
    multi_ms, got = five(multi)
    st = got["stats"]
    singles_ms, agreement = [], []
    for e, mix in enumerate(mixes):
        one = context(dict(params, **{"plasma_" + key: value for key, value in mix.items()}), tier)
        times, out = five(one)
        singles_ms.append(times)
        mine = got["image_by_mix"][e]
        worst, above, used, same_support = gu.per_pixel_relative(mine, out["image"])
        agreement.append(dict(mix=mix, per_pixel_relative=worst, same_bits=bool(gu.same_bits(mine, out["image"]).all()),
                              same_nan=bool(np.array_equal(np.isnan(mine), np.isnan(out["image"]))), same_support=same_support,
                              arithmetic=out["stats"].arithmetic, launches_shade=out["stats"].launches_shade))
        one.close()
    multi.close()
    sums = [float(sum(times[r] for times in singles_ms)) for r in range(5)]   # (repetition r of every fresh context)
    print(json.dumps(dict(step=args.step, tier=tier, n_mixes=len(mixes), multi_ms=multi_ms, multi_median_ms=float(np.median(multi_ms)),
                          multi_spread_ms=float(max(multi_ms) - min(multi_ms)), singles_sum_ms=sums, singles_median_ms=float(np.median(sums)),
                          singles_spread_ms=float(max(sums) - min(sums)), ratio=float(np.median(multi_ms) / np.median(sums)),
                          arithmetic=st.arithmetic, launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade,
                          launches_transfer=st.launches_transfer, n_chunks=st.n_chunks, ms_geodesic=st.ms_geodesic, ms_shade=st.ms_shade,
                          ms_transfer=st.ms_transfer, worst_per_pixel_relative=max(a["per_pixel_relative"] for a in agreement),
                          all_same_bits=all(a["same_bits"] for a in agreement), all_same_nan=all(a["same_nan"] for a in agreement),
                          agreement=agreement)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--mixes", default="2,6,16")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--unused", default="frame,truecolor,models6")
    ap.add_argument("--processes", type=int, default=3, help="processes per tree of an `unused` comparison")
    ap.add_argument("--runs", type=int, default=3, help="processes per tree of the `runs` comparison (0: none)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the `unused` comparisons")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "electron_mixes.json"))
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    steps = [(f"mixes:{k}:{tier}", HERE) for tier in args.tiers.split(",") if tier for k in args.mixes.split(",") if k]
    for name in [n for n in args.unused.split(",") if n]:
        for _ in range(args.processes):   # (alternating: parent, this, parent, this, ...)
            steps += ([(f"unused:{name}", args.parent)] if args.parent else []) + [(f"unused:{name}", HERE)]
    for _ in range(args.runs):
        steps += ([("runs", args.parent)] if args.parent else []) + [("runs", HERE)]
    results = []

    def save():   # (after every step: a run cut short keeps what it measured)
        doc = dict(res=args.res, grid=args.grid, results=[r for r in results if r["step"].startswith("mixes")], unused={})
        for step in sorted({r["step"] for r in results if not r["step"].startswith("mixes")}):
            by_tree = {tree: [r["ms"] for r in results if r["step"] == step and r["tree"] == tree] for tree in ("this", "parent")}
            row = {tree + "_ms": values for tree, values in by_tree.items() if values}
            if by_tree["this"] and by_tree["parent"]:
                this_median, parent_median = sorted(by_tree["this"])[len(by_tree["this"]) // 2], sorted(by_tree["parent"])[len(by_tree["parent"]) // 2]
                spread = max(by_tree["parent"]) - min(by_tree["parent"])
                row.update(this_median_ms=this_median, parent_median_ms=parent_median, parent_spread_ms=spread,
                           within_parent_spread=bool(this_median - parent_median <= spread))
            if step == "runs":
                doc["runs"] = row
            else:
                doc["unused"][step.split(":")[1]] = row
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    for step, tree in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--res", str(args.res),
               "--grid", str(args.grid)]
        env = dict(os.environ, BLACKLIGHT_AMD_TREE=os.path.abspath(tree))
        run = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=os.path.abspath(tree))
        if run.returncode != 0:   # a failed step, a time limit: nothing more is started on the device
            print(f"step {step} ({tree}) ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}", flush=True)
            sys.exit(run.returncode)
        row = json.loads(run.stdout.strip().splitlines()[-1])
        row["tree"] = "this" if tree == HERE else "parent"
        print(json.dumps({k: v for k, v in row.items() if k not in ("agreement", "bench")}), flush=True)
        results.append(row)
        save()


if __name__ == "__main__":
    main()
