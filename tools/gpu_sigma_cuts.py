"""Several sigma cuts in one render (bl_set_sigma_cuts) against one fresh render per cut, and what the axis costs a render without it.

    python tools/gpu_sigma_cuts.py [--res 1024] [--grid 256] [--cuts 2,6,16] [--models-x-cuts 6x4] [--reps 3] [--parent TREE]
                                   [--step-timeout 600] [--out profiles/sigma_cuts.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), thermal electrons, 230 GHz: bench.py's default workload, tolerant tier. One
invocation measures everything, step by step: every step is a child process of its own (this file with --step) under a time limit of
its own, and the first step that fails or runs out of time ends the run - nothing is started on the device after it. The steps:

  cuts:S        one render of S thresholds (cut_sigma_max swept log-evenly over 0.03 ... 30, the last one off) against S renders, each
                in a context of its own holding that threshold - what a library over the cut costs without the call;
  models_x_cuts the same for M electron models (R_high over 1 ... 160) times S thresholds against M * S fresh renders;
  no_cuts       the M-model one-pass render with no cuts set - the path that must not pay for an axis it does not use - in this tree
                and, with --parent TREE (a built checkout of the parent commit), in that one: `reps` repetitions each, a repetition
                the median of five timed renders. `within_parent_spread` says whether this tree's median exceeds the parent's by no
                more than the parent's own min-to-max spread.

Both sides of a comparison integrate their geodesics (bl_set_geodesic_reuse(0)); bl_set_grid is outside the timed region, and every
timed render follows an untimed one of the same context (the first render of a context allocates its scratch). Times are host wall
clock between device synchronisations. The per-pixel agreement of every variant's image with its fresh render is recorded
(gu.per_pixel_relative).
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("BLACKLIGHT_AMD_TREE", HERE)   # (a --step child of the parent's measurement imports the parent's package)


def cut_sweep(k):
    import numpy as np
    return [float(x) for x in np.geomspace(0.03, 30.0, k - 1)] + [-1.0] if k > 1 else [1.0]


def model_sweep(k):
    import numpy as np
    return [float(x) for x in np.geomspace(1.0, 160.0, k)] if k > 1 else [10.0]


def run_step(args):
    """--step: one measurement in this process; prints one JSON line"""
    sys.path.insert(0, TREE)
    sys.path.insert(0, os.path.join(TREE, "tests"))
    import numpy as np
    import torch
    import bench
    import blacklight_amd as bl
    from blacklight_amd import mock

    params = dict(bench.WORKLOAD, camera_resolution=args.res)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)

    def context(p, cuts=None, highs=None):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        ctx.set_geodesic_reuse(False)
        ctx.set_arithmetic("tolerant")
        ctx.set_grid(grid)
        if highs is not None:
            ctx.set_electron_models(highs, rat_low=1.0)
        if cuts is not None:
            ctx.set_sigma_cuts(cuts)
        return ctx

    def timed(ctx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    kind, _, size = args.step.partition(":")
    if kind == "no_cuts":
        highs = model_sweep(int(size))
        ctx = context(params, None, highs)
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
        print(json.dumps(dict(step=args.step, tree=os.path.basename(os.path.normpath(TREE)) if TREE != HERE else "this", n_models=len(highs),
                              rep_ms=reps, median_ms=float(np.median(reps)), spread_ms=float(max(reps) - min(reps)),
                              launches_shade=st.launches_shade, launches_transfer=st.launches_transfer, n_chunks=st.n_chunks,
                              ms_shade=st.ms_shade, ms_transfer=st.ms_transfer, ms_geodesic=st.ms_geodesic)))
        return
    import golden_util as gu
    if kind == "cuts":
        highs, cuts = None, cut_sweep(int(size))
    else:
        m, s = (int(x) for x in size.split("x"))
        highs, cuts = model_sweep(m), cut_sweep(s)
    multi = context(params, cuts, highs)
    timed(multi)   # (warm-up)
    variants = [(h, c) for h in (highs or [None]) for c in cuts]
    multi_ms, single_ms = [], []
    single_images = [None] * len(variants)
    got = None
    for rep in range(args.reps):
        timed(multi)   # (each timed render right behind one of its own, as for the fresh contexts below)
        ms, got = timed(multi)
        multi_ms.append(ms)
        total = 0.0
        for v, (high, cut) in enumerate(variants):
            over = dict(cut_sigma_max=cut)
            if high is not None:
                over.update(plasma_rat_low=1.0, plasma_rat_high=high)
            one = context(dict(params, **over))
            timed(one)   # (warm-up: a context's first render allocates its scratch)
            ms, out = timed(one)
            total += ms
            single_images[v] = out["image"]
            one.close()
        single_ms.append(total)
    st = got["stats"]
    n_s = len(cuts)
    agreement = []
    for v, (high, cut) in enumerate(variants):
        mine = got["image_by_cut"][v // n_s, 0, v % n_s]
        worst, above, used, same_support = gu.per_pixel_relative(mine, single_images[v])
        agreement.append(dict(rat_high=high, sigma_max=cut, per_pixel_relative=worst, same_nan=bool(np.array_equal(np.isnan(mine), np.isnan(single_images[v]))),
                              same_support=same_support))
    differing = [int((~gu.same_bits(got["image_by_cut"][0, 0, s], got["image_by_cut"][0, 0, s + 1])).sum()) for s in range(n_s - 1)]
    multi.close()
    print(json.dumps(dict(step=args.step, n_cuts=n_s, n_models=len(highs) if highs else 0, sigma_max=cuts, rat_high=highs, multi_ms=multi_ms,
                          singles_ms=single_ms, ratio=float(np.median(multi_ms) / np.median(single_ms)), arithmetic=st.arithmetic,
                          launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade, launches_transfer=st.launches_transfer,
                          n_chunks=st.n_chunks, n_deferred=st.n_deferred, ms_geodesic=st.ms_geodesic, ms_shade=st.ms_shade, ms_transfer=st.ms_transfer,
                          pixels_differing_between_neighbouring_cuts=differing,
                          worst_per_pixel_relative=max(a["per_pixel_relative"] for a in agreement),
                          all_same_nan=all(a["same_nan"] for a in agreement), agreement=agreement)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cuts", default="2,6,16")
    ap.add_argument("--models-x-cuts", default="6x4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the no_cuts comparison")
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sigma_cuts.json"))
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    m = int(args.models_x_cuts.split("x")[0])
    steps = [(f"cuts:{k}", HERE) for k in args.cuts.split(",") if k] + [(f"models_x_cuts:{args.models_x_cuts}", HERE)]
    steps += ([(f"no_cuts:{m}", args.parent)] if args.parent else []) + [(f"no_cuts:{m}", HERE)]
    results = []

    def save():   # (after every step: a run cut short keeps what it measured)
        doc = dict(res=args.res, grid=args.grid, tier="tolerant", reps=args.reps, results=[r for r in results if not r["step"].startswith("no_cuts")])
        no_cuts = {r["tree"]: r for r in results if r["step"].startswith("no_cuts")}
        if no_cuts:
            doc["no_cuts"] = dict(this=no_cuts.get("this"), parent=no_cuts.get("parent"))
            if no_cuts.get("this") and no_cuts.get("parent"):
                over = no_cuts["this"]["median_ms"] - no_cuts["parent"]["median_ms"]
                doc["no_cuts"].update(this_minus_parent_ms=over, within_parent_spread=bool(over <= no_cuts["parent"]["spread_ms"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    for step, tree in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--res", str(args.res),
               "--grid", str(args.grid), "--reps", str(args.reps)]
        env = dict(os.environ, BLACKLIGHT_AMD_TREE=os.path.abspath(tree))
        run = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=os.path.abspath(tree))
        if run.returncode != 0:   # a failed step, a time limit: nothing more is started on the device
            print(f"step {step} ({tree}) ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}", flush=True)
            sys.exit(run.returncode)
        row = json.loads(run.stdout.strip().splitlines()[-1])
        if step.startswith("no_cuts"):
            row["tree"] = "this" if tree == HERE else "parent"
        print(json.dumps({k: v for k, v in row.items() if k != "agreement"}), flush=True)
        results.append(row)
        save()


if __name__ == "__main__":
    main()
