"""Polarized variants with a sigma cut each in one render (bl_set_polarized_variants_sigma) against one fresh render per variant, and
what the cut costs a render of triples that does not use it.

    python tools/gpu_polarized_cuts.py [--res 1024] [--grid 256] [--cuts 2,4,6] [--triples-x-cuts 3x2] [--tiers exact,tolerant] [--reps 3]
                                       [--parent TREE] [--rounds 3] [--step-timeout 600] [--out profiles/polarized_cuts.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), full Stokes and the optical-depth row, 230 GHz: bench.py's polarized1024
workload, as tools/gpu_polarized_variants.py renders it. One invocation measures everything, step by step: every step is a child
process of its own (this file with --step) under a time limit of its own, and the first step that fails or runs out of time ends the
run - nothing is started on the device after it. The steps, for every tier:

  cuts:S:TIER          one triple (the workload's own) under S thresholds - cut_sigma_max swept log-evenly over 0.03 ... 30, the last one
                       off - in one render, against S renders, each in a context of its own with that threshold in its parameter block:
                       what a library over the cut costs without the call;
  triples_x_cuts:TxS:TIER   T triples (R_high over 1 ... 160, the unit over 0.1 ... 10 times the workload's) times S thresholds as T * S
                       quadruples, against T * S fresh renders;
  no_cuts:V:TIER       V triples with no cuts set - the path that must not pay for a decision it does not make - in this tree and, with
                       --parent TREE (a built checkout of the parent commit), in that one. A process measures `reps` repetitions, a
                       repetition the median of five timed renders, and the two trees alternate for `rounds` processes each: the
                       scatter from one process to the next (a context's allocations land elsewhere, clocks settle elsewhere) is
                       several times the scatter within one, and only a comparison over processes sees it. `within_parent_spread`
                       says whether the median of this tree's processes exceeds the median of the parent's by no more than the
                       min-to-max spread of the parent's processes.

Both sides of a comparison integrate their geodesics (bl_set_geodesic_reuse(0)); bl_set_grid is outside the timed region, and every
timed render follows an untimed one of the same context (a context's first render allocates its scratch). The two are alternated
`reps` times; times are host wall clock between device synchronisations, medians are compared, and the fresh renders' own run-to-run
spread - (max - min) / median of their per-repetition sums - is recorded beside the ratio. Every variant's rows are compared with its
fresh render's bit for bit.
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

    def context(p, quads=None, cuts=True):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        ctx.set_geodesic_reuse(False)
        ctx.set_arithmetic(tier)
        ctx.set_grid(grid)
        if quads is not None:
            extra = dict(sigma_max=[c for _, _, _, c in quads]) if cuts else {}
            ctx.set_polarized_variants([h for _, h, _, _ in quads], [u for _, _, u, _ in quads], rat_low=[lo for lo, _, _, _ in quads], **extra)
        return ctx

    def timed(ctx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if kind == "no_cuts":
        triples = triple_sweep(rho0, int(size))
        ctx = context(params, [t + (None,) for t in triples], cuts=False)
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
        print(json.dumps(dict(step=args.step, tier=tier, n_variants=len(triples), rep_ms=reps, median_ms=float(np.median(reps)),
                              spread_ms=float(max(reps) - min(reps)), launches_shade=st.launches_shade, launches_transfer=st.launches_transfer,
                              n_chunks=st.n_chunks, ms_shade=st.ms_shade, ms_transfer=st.ms_transfer, ms_geodesic=st.ms_geodesic)))
        return
    import golden_util as gu
    if kind == "cuts":
        own = (float(params["plasma_rat_low"]), float(params["plasma_rat_high"]), rho0)
        triples, cuts = [own], cut_sweep(int(size))
    else:
        t, s = (int(x) for x in size.split("x"))
        triples, cuts = triple_sweep(rho0, t), cut_sweep(s)
    quads = [triple + (cut,) for triple in triples for cut in cuts]
    multi = context(params, quads)
    timed(multi)   # (warm-up)
    multi_ms, fresh_sum_ms, fresh_each_ms = [], [], []
    fresh_images = [None] * len(quads)
    got = fresh_stats = None
    for rep in range(args.reps):
        timed(multi)   # (each timed render right behind one of its own, as for the fresh contexts below)
        ms, got = timed(multi)
        multi_ms.append(ms)
        each = []
        for v, (low, high, unit, cut) in enumerate(quads):
            one = context(dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit, cut_sigma_max=cut))
            timed(one)   # (warm-up: a context's first render allocates its scratch)
            ms, out = timed(one)
            each.append(ms)
            fresh_images[v] = out["image"]
            fresh_stats = out["stats"]
            one.close()
        fresh_each_ms.append(each)
        fresh_sum_ms.append(sum(each))
    st = got["stats"]
    same = [bool(gu.same_bits(got["image_by_variant"][v], fresh_images[v]).all()) for v in range(len(quads))]
    differing = [int((~gu.same_bits(got["image_by_variant"][v], got["image_by_variant"][v + 1])).sum()) for v in range(len(cuts) - 1)]
    multi.close()
    fresh_median = float(np.median(fresh_sum_ms))
    print(json.dumps(dict(step=args.step, tier=tier, n_variants=len(quads), n_triples=len(triples), n_cuts=len(cuts), quadruples=quads,
                          multi_ms=multi_ms, fresh_sum_ms=fresh_sum_ms, fresh_each_ms=fresh_each_ms,
                          multi_median_ms=float(np.median(multi_ms)), fresh_median_ms=fresh_median, ratio=float(np.median(multi_ms) / fresh_median),
                          multi_spread=float((max(multi_ms) - min(multi_ms)) / np.median(multi_ms)),
                          fresh_spread=float((max(fresh_sum_ms) - min(fresh_sum_ms)) / fresh_median),
                          arithmetic=st.arithmetic, n_chunks=st.n_chunks, launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade,
                          launches_transfer=st.launches_transfer, ms_geodesic=st.ms_geodesic, ms_locate=st.ms_locate, ms_shade=st.ms_shade,
                          ms_transfer=st.ms_transfer, fresh_n_chunks=fresh_stats.n_chunks, fresh_ms_geodesic=fresh_stats.ms_geodesic,
                          fresh_ms_shade=fresh_stats.ms_shade, fresh_ms_transfer=fresh_stats.ms_transfer,
                          values_differing_between_neighbouring_cuts=differing, same_bits=same, all_same_bits=all(same))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cuts", default="2,4,6")
    ap.add_argument("--triples-x-cuts", default="3x2")
    ap.add_argument("--no-cuts", type=int, default=6, help="triples of the render without cuts")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the no_cuts comparison")
    ap.add_argument("--rounds", type=int, default=3, help="processes per tree of the no_cuts comparison, alternating")
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "polarized_cuts.json"))
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    steps = []
    for tier in args.tiers.split(","):
        steps += [(f"cuts:{k}:{tier}", HERE) for k in args.cuts.split(",") if k]
        if args.triples_x_cuts:
            steps.append((f"triples_x_cuts:{args.triples_x_cuts}:{tier}", HERE))
        for _ in range(args.rounds if args.parent else 1):
            steps += ([(f"no_cuts:{args.no_cuts}:{tier}", args.parent)] if args.parent else []) + [(f"no_cuts:{args.no_cuts}:{tier}", HERE)]
    results = []

    import statistics

    def save():   # (after every step: a run cut short keeps what it measured)
        doc = dict(res=args.res, grid=args.grid, reps=args.reps, results=[r for r in results if not r["step"].startswith("no_cuts")])
        rows = [r for r in results if r["step"].startswith("no_cuts")]
        if rows:
            doc["no_cuts"] = dict(rows=rows)
            for tier in sorted({r["tier"] for r in rows}):
                ours = [r["median_ms"] for r in rows if r["tier"] == tier and r["tree"] == "this"]
                theirs = [r["median_ms"] for r in rows if r["tier"] == tier and r["tree"] == "parent"]
                if ours and theirs:
                    over = statistics.median(ours) - statistics.median(theirs)
                    doc["no_cuts"][tier] = dict(this_process_ms=ours, parent_process_ms=theirs, this_ms=statistics.median(ours),
                                                parent_ms=statistics.median(theirs), this_spread_ms=max(ours) - min(ours),
                                                parent_spread_ms=max(theirs) - min(theirs), this_minus_parent_ms=over,
                                                within_parent_spread=bool(over <= max(theirs) - min(theirs)))
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
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ("quadruples", "fresh_each_ms", "same_bits")}), flush=True)
        save()


if __name__ == "__main__":
    main()
