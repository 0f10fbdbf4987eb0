#!/usr/bin/env python3
"""Several cameras in one render (bl_set_cameras) against one context per camera, and what the axis costs a render without it.

    python tools/gpu_cameras.py [--sizes 128:2,128:6,128:16,256:2,256:6,256:16,1024:2] [--tiers tolerant,exact] [--grid 256] [--reps 5]
                                [--cli 6] [--parent TREE] [--headline-reps 4] [--step-timeout 600] [--out profiles/cameras.json]

bench.py's workload (256^3 mock, thermal electrons, 230 GHz) seen by C cameras: inclinations spread evenly over 17 ... 163 degrees, the
azimuth advancing by 40 degrees per camera. One invocation measures everything, step by step: every step is a child process of its own
(this file with --step) under a time limit of its own, and the first step that fails or runs out of time ends the run - nothing is
started on the device after it. The steps:

  cameras:RES:C:TIER  one render of C cameras (C res^2 rays) against C renders in C contexts made by bl_init with the camera's angles in
                      the block. Both integrate their geodesics (bl_set_geodesic_reuse(0)); every timed render follows an untimed one
                      of its context. Recorded: the median of `reps` renders and (max - min) / median on both sides, bl_stats.ms_geodesic
                      and ms_total beside the wall clock - whether filling the lanes is where the time goes -, n_chunks, and the C
                      contexts' set-up (bl_init, bl_set_grid, first render: what a process per camera pays again and again), so that the
                      comparison stands with and without it. The slices' agreement with the fresh renders is recorded
                      (golden_util.per_pixel_relative; bits in the exact tier).
  cli:C               one process of bin/blacklight_amd with C cameras in the .input file against C processes, as tools/gpu_cli_sweep.py
                      does for models: wall clock of whole processes, 1024^2, alternated `reps` times.
  headline            bench.py's frame with no cameras set, this tree against --parent TREE (a built checkout of the parent commit):
                      whole bench.py processes, alternated; `within_parent_spread` says whether this tree's median time per frame
                      exceeds the parent's by no more than the parent's own min-to-max spread over its processes.

Times are host wall clock between device synchronisations unless they carry bl_stats' names. Measured, not asserted.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(HERE, "blacklight_amd", "bin", "blacklight_amd")


def camera_list(n):
    import numpy as np
    return [(float(th), float((40.0 * c) % 360.0)) for c, th in enumerate(np.linspace(17.0, 163.0, n))]


def step_cameras(args, res, n, tier):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    import torch
    import bench
    import blacklight_amd as bl
    import golden_util as gu
    from blacklight_amd import mock

    params = dict(bench.WORKLOAD, camera_resolution=res)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    cameras = camera_list(n)

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    def context(p):
        ctx = bl.Context(bl.Params.from_dict(p), device=0)
        ctx.set_geodesic_reuse(False)
        ctx.set_arithmetic(tier)
        ctx.set_grid(grid)
        return ctx

    def timed(ctx):
        t0 = clock()
        out = ctx.render()
        return (clock() - t0) * 1e3, out

    warm = context(params)   # (the process's first context: code objects, the runtime's pools - neither side's to pay)
    timed(warm)
    warm.close()
    t0 = clock()
    multi = context(params)
    multi.set_cameras([th for th, _ in cameras], [ph for _, ph in cameras])
    timed(multi)
    multi_setup = (clock() - t0) * 1e3
    multi_ms, multi_geo, multi_total = [], [], []
    for _ in range(args.reps):
        ms, got = timed(multi)
        multi_ms.append(ms)
        multi_geo.append(got["stats"].ms_geodesic)
        multi_total.append(got["stats"].ms_total)
    st = got["stats"]
    slices = [multi.camera_slice(c) for c in range(n)]
    multi.close()
    single_ms, single_geo, single_total, single_setup = [[] for _ in range(args.reps)], [[] for _ in range(args.reps)], [[] for _ in range(args.reps)], []
    worst, same_nan, same_integers, bits = 0.0, True, True, True
    for c, (th, ph) in enumerate(cameras):
        t0 = clock()
        one = context(dict(params, camera_th=th, camera_ph=ph))
        timed(one)
        single_setup.append((clock() - t0) * 1e3)
        for rep in range(args.reps):
            ms, out = timed(one)
            single_ms[rep].append(ms)
            single_geo[rep].append(out["stats"].ms_geodesic)
            single_total[rep].append(out["stats"].ms_total)
        mine = got["image"][:, slices[c]]
        rel, _, _, _ = gu.per_pixel_relative(mine, out["image"])
        worst = max(worst, rel)
        same_nan = same_nan and bool(np.array_equal(np.isnan(mine), np.isnan(out["image"])))
        bits = bits and bool(gu.same_bits(mine, out["image"]).all())
        same_integers = same_integers and bool(np.array_equal(got["sample_num"][slices[c]], out["sample_num"])
                                               and np.array_equal(got["sample_flags"][slices[c]], out["sample_flags"]))
        one.close()

    def summary(values):
        return dict(median=float(np.median(values)), spread=float((max(values) - min(values)) / np.median(values)))

    sums = [float(sum(rep)) for rep in single_ms]
    print(json.dumps(dict(
        step=args.step, res=res, n_cameras=n, tier=tier, n_rays=int(st.n_rays), n_chunks=int(st.n_chunks), launches_geodesic=int(st.launches_geodesic),
        xcd_order=int(st.xcd_order), tail_policy=int(st.tail_policy),
        one_render_ms=summary(multi_ms), one_render_ms_geodesic=summary(multi_geo), one_render_ms_total=summary(multi_total),
        separate_renders_ms=summary(sums), separate_ms_geodesic=summary([float(sum(rep)) for rep in single_geo]),
        separate_ms_total=summary([float(sum(rep)) for rep in single_total]),
        ratio_renders_only=float(np.median(multi_ms) / np.median(sums)),
        one_context_setup_ms=multi_setup, separate_contexts_setup_ms=float(sum(single_setup)),
        ratio_with_setup=float((multi_setup + np.median(multi_ms)) / (sum(single_setup) + np.median(sums))),
        setup_note="set-up = bl_init + bl_set_grid + the context's first render, inside one process whose runtime is already up; a process per "
                   "camera pays the runtime's start besides (the cli step)",
        worst_per_pixel_relative=worst, same_nan=same_nan, same_integers=same_integers, same_bits=bits)))


def step_cli(args, n):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    import bench
    import sweep_util as su
    from blacklight_amd import mock
    from blacklight_amd.params import _format

    def write_input(path, params):
        with open(path, "w") as f:
            for key, value in params.items():
                f.write(f"{key} = {value if isinstance(value, str) else _format(value)}\n")
        return path

    def run(input_path):
        t0 = time.perf_counter()
        done = subprocess.run(["timeout", "-k", "10", "120", EXE, input_path], capture_output=True, text=True,
                              env=dict(os.environ, BLACKLIGHT_AMD_ARITHMETIC=args.cli_tier))
        if done.returncode != 0:
            sys.exit(f"{input_path}: exit status {done.returncode}\n{done.stdout[-2000:]}{done.stderr[-2000:]}")
        return time.perf_counter() - t0

    work = tempfile.mkdtemp(prefix="cli_cameras_")
    grid_path = os.path.join(work, "grid.blgrid")
    mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid).save_raw(grid_path)
    base = dict(bench.WORKLOAD, camera_resolution=args.cli_res, simulation_file=grid_path, simulation_multiple=False, output_format="npz")
    cameras = camera_list(n)
    together_out = os.path.join(work, "together.npz")
    together = write_input(os.path.join(work, "together.input"), dict(base, output_file=together_out, sweep_camera_th=su.comma(th for th, _ in cameras),
                                                                      sweep_camera_ph=su.comma(ph for _, ph in cameras)))
    singles = [write_input(os.path.join(work, f"single_{c}.input"), dict(base, output_file=os.path.join(work, f"single_{c}.npz"), camera_th=th, camera_ph=ph))
               for c, (th, ph) in enumerate(cameras)]
    run(together)   # (one untimed process of either kind first: the grid file into the page cache)
    run(singles[0])
    one, many = [], []
    for rep in range(args.reps):
        one.append(run(together))
        many.append(sum(run(path) for path in singles))
    same = [su.file_bytes(together_out.replace(".npz", f".c{c:02d}.npz")) == su.file_bytes(os.path.join(work, f"single_{c}.npz")) for c in range(n)]
    for name in os.listdir(work):
        os.remove(os.path.join(work, name))
    os.rmdir(work)
    print(json.dumps(dict(step=args.step, res=args.cli_res, n_cameras=n, tier=args.cli_tier, one_process_s=one, separate_processes_s=many,
                          one_process_median_s=float(np.median(one)), separate_median_s=float(np.median(many)),
                          ratio=float(np.median(one) / np.median(many)), one_process_spread=float((max(one) - min(one)) / np.median(one)),
                          separate_spread=float((max(many) - min(many)) / np.median(many)), files_equal_but_for_zip_time_stamps=same)))


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
    ap.add_argument("--sizes", default="128:2,128:6,128:16,256:2,256:6,256:16,1024:2")
    ap.add_argument("--tiers", default="tolerant,exact")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli", type=int, default=6)
    ap.add_argument("--cli-res", type=int, default=1024)
    ap.add_argument("--cli-tier", default="tolerant")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the headline comparison")
    ap.add_argument("--headline-reps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cameras.json"))
    args = ap.parse_args()
    if args.step:
        kind, _, rest = args.step.partition(":")
        if kind == "cameras":
            res, n, tier = rest.split(":")
            return step_cameras(args, int(res), int(n), tier)
        if kind == "cli":
            return step_cli(args, int(rest))
        return step_headline(args)
    steps = [f"cameras:{size}:{tier}" for tier in args.tiers.split(",") if tier for size in args.sizes.split(",") if size]
    steps += [f"cli:{args.cli}"] if args.cli > 0 else []
    steps += ["headline"] if args.parent else []
    doc = dict(grid=args.grid, reps=args.reps, workload="bench.py's: 256^3 mock, thermal electrons, 230 GHz, plane camera at r = 50",
               cameras="inclinations evenly over 17 ... 163 degrees, azimuth + 40 degrees per camera", one_render_against_separate_contexts=[])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--grid", str(args.grid),
               "--reps", str(args.reps), "--cli-res", str(args.cli_res), "--cli-tier", args.cli_tier, "--headline-reps", str(args.headline_reps)]
        if args.parent:
            cmd += ["--parent", args.parent]
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=HERE)
        if run.returncode != 0:   # a failed step, a time limit: nothing more is started on the device
            print(f"step {step} ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}", flush=True)
            sys.exit(run.returncode)
        row = json.loads(run.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        if step.startswith("cameras"):
            doc["one_render_against_separate_contexts"].append(row)
        else:
            doc["command_line" if step.startswith("cli") else "headline_no_cameras_set"] = row
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:   # (after every step: a run cut short keeps what it measured)
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
