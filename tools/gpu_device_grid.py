#!/usr/bin/env python3
"""What staging a snapshot from device memory costs (bl_set_grid_device) beside staging it from host memory (bl_set_grid), on the
benchmark's workload (bench.WORKLOAD: 1024^2 camera, the 256^3 mock, tolerant tier). Writes profiles/device_grid.json.

    python tools/gpu_device_grid.py [--out profiles/device_grid.json] [--parent DIR] [--grid 256] [--resolution 1024]

Every GPU step is a child process of its own under `timeout -k 10`; the first that fails ends the job (its output is shown).
  (a) staging  one process per source - host planes (pageable), device float32 [var][block], device float32 [block][var] (the mock cut
               into 8 blocks), device float64 [var][block]: the first call (tables and all), then 12 calls on the geometry in place
               (cells only): median, min, max of the wall time, and for the device sources the bytes the staging kernel moves
               ((4 or 8 B read + 4 B written) x 8 x n_cells) per second of that wall time - launch and synchronisation included, so a
               lower bound of the kernel's own rate - against the 6.29 TB/s a float4 copy reaches on this part.
  (b) series   8 snapshots resident as one device tensor: per frame set_grid_device + render into HBM, frames 2 ... 8, beside
               `bench.py --workload series8` (render alone, bl_set_grid apart) and `--workload series8_pipelined` (bl_set_grid
               beside the render) in the same session.
  (c) parent   with --parent DIR (a built tree of the parent commit): three alternating processes of either tree for bl_set_grid
               from host planes (this tool's `--step staging --source host`, run from that tree) and for bench.py's default line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12   # float4 copy, bytes per second (read + write), measured on an MI355X


def _tree(path):
    sys.path.insert(0, path)
    sys.path.insert(0, os.path.join(path, "tests"))


def step_staging(args):
    """One source in this process; prints one JSON line"""
    import dataclasses
    import numpy as np
    import torch
    _tree(args.tree)
    import bench
    import blacklight_amd as bl
    import golden_util as gu
    from blacklight_amd import mock
    params = dict(bench.WORKLOAD, camera_resolution=args.resolution)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    if args.source == "device_f32_bv":
        grid = gu.split_grid(grid, 2, 2, 2)
    n_cells = int(np.prod(grid.prim.shape[1:]))
    torch.cuda.set_device(0)
    if args.source == "host":
        def stage(ctx):
            ctx.set_grid(grid)
    else:
        tensor = torch.from_numpy(grid.prim).cuda()
        dims = "vb"
        if args.source == "device_f32_bv":
            tensor, dims = tensor.transpose(0, 1).contiguous(), "bv"
        if args.source == "device_f64_vb":
            tensor = tensor.double()
        bare = dataclasses.replace(grid, prim=None)

        def stage(ctx):
            ctx.set_grid_device(bare, tensor, stream=None, dims=dims)
    times = []
    with bl.Context(bl.Params.from_dict(params), device=0) as ctx:
        ctx.set_arithmetic("tolerant")
        for n in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage(ctx)
            torch.cuda.synchronize()
            times.append(1000.0 * (time.perf_counter() - t0))
        host_bytes = getattr(ctx, "grid_host_bytes", None)
    later = times[1:]
    line = dict(source=args.source, n_cells=n_cells, n_blocks=int(grid.prim.shape[1]), ms_first_call=times[0], ms_median=statistics.median(later),
                ms_min=min(later), ms_max=max(later), calls=len(later), host_bytes_last_call=host_bytes)
    if args.source != "host":
        moved = (8 if args.source == "device_f64_vb" else 4) * 8 * n_cells + 4 * 8 * n_cells
        line.update(kernel_bytes=moved, bytes_per_s_of_wall_median=moved / (line["ms_median"] * 1.0e-3), bytes_per_s_of_wall_min=moved / (line["ms_min"] * 1.0e-3),
                    frac_of_float4_copy_rate=moved / (line["ms_min"] * 1.0e-3) / COPY_RATE)
    print(json.dumps(line), flush=True)


def step_series(args):
    """8 resident snapshots: set_grid_device + render per frame; prints one JSON line"""
    import dataclasses
    import numpy as np
    import torch
    _tree(args.tree)
    import bench
    import blacklight_amd as bl
    from blacklight_amd import mock
    n_frames, res = 8, args.resolution
    params = dict(bench.WORKLOAD, camera_resolution=res, simulation_multiple=True, simulation_start=0, simulation_end=n_frames - 1)
    base = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    first = torch.from_numpy(base.prim).to(device)
    series = first.unsqueeze(0).repeat(n_frames, 1, 1, 1, 1, 1)
    for n in range(n_frames):   # (bench.py's series8: density and pressure of snapshot n)
        series[n, 0:2] *= np.float32(1.0 + 0.07 * n)
    bare = dataclasses.replace(base, prim=None)
    n_rays = res * res
    image = torch.zeros((1, n_rays), dtype=torch.float64, device=device)
    sample_num = torch.zeros(n_rays, dtype=torch.int32, device=device)
    flags = torch.zeros(n_rays, dtype=torch.uint8, device=device)
    with bl.Context(bl.Params.from_dict(params), device=0) as ctx:
        ctx.set_arithmetic("tolerant")
        ctx.follow_torch_stream(device)
        for rep in range(2):   # (a warm-up series first)
            frames = []
            ctx.set_geodesic_reuse(False)
            ctx.set_geodesic_reuse(True)
            for n in range(n_frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.set_grid_device(bare, series[n], stream=None)
                t1 = time.perf_counter()
                st = ctx.render_device(image.data_ptr(), n_rays, sample_num_ptr=sample_num.data_ptr(), sample_flags_ptr=flags.data_ptr())
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                frames.append(dict(ms_staging=1000.0 * (t1 - t0), ms_render=1000.0 * (t2 - t1), ms_frame=1000.0 * (t2 - t0), geodesics_reused=int(st.geodesics_reused)))
    later = frames[1:]
    print(json.dumps(dict(frames=frames, frames_2_to_8=dict(
        ms_frame_mean=statistics.mean(f["ms_frame"] for f in later), ms_frame_min=min(f["ms_frame"] for f in later), ms_frame_max=max(f["ms_frame"] for f in later),
        ms_staging_mean=statistics.mean(f["ms_staging"] for f in later), ms_render_mean=statistics.mean(f["ms_render"] for f in later),
        all_reused_geodesics=all(f["geodesics_reused"] == 1 for f in later)))), flush=True)


def child(command, limit, cwd=REPO):
    """A GPU step as a process of its own under a time limit; its last JSON line. Any failure ends the job."""
    run = subprocess.run(["timeout", "-k", "10", str(limit)] + command, cwd=cwd, capture_output=True, text=True)
    if run.returncode != 0:
        sys.stderr.write(run.stdout[-4000:] + run.stderr[-4000:])
        sys.exit(f"step failed with status {run.returncode}: {' '.join(command)}")
    lines = [line for line in run.stdout.splitlines() if line.startswith("{")]
    print("done:", " ".join(command[1:]), flush=True)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_grid.json"))
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit, for (c)")
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to measure; the others are kept as --out has them")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--step", choices=["staging", "series"], default=None, help="(internal) run one step in this process")
    ap.add_argument("--source", choices=["host", "device_f32_vb", "device_f32_bv", "device_f64_vb"], default="host")
    ap.add_argument("--tree", default=REPO, help="(internal) the tree whose package the step imports")
    args = ap.parse_args()
    if args.step == "staging":
        return step_staging(args)
    if args.step == "series":
        return step_series(args)
    me = [sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--resolution", str(args.resolution)]
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result.update(workload=f"bench.WORKLOAD, {args.resolution}^2 camera, {args.grid}^3 mock, tolerant tier", float4_copy_rate_bytes_per_s=COPY_RATE)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    bench = [sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline"]
    if "a" in args.parts:
        result["a_staging"] = {}
        for source in ("host", "device_f32_vb", "device_f32_bv", "device_f64_vb"):
            result["a_staging"][source] = child(me + ["--step", "staging", "--source", source], 240)
            save()
    if "b" in args.parts:
        result["b_series"] = dict(resident=child(me + ["--step", "series"], 300))
        save()
        for workload in ("series8", "series8_pipelined"):
            line = child(bench + ["--workload", workload, "--warmup", "1"], 420)
            result["b_series"][workload] = {k: line[k] for k in ("ms_per_step", "frames_2_to_8", "whole_series", "frame_1") if k in line}
            save()
    if "c" in args.parts and args.parent:
        parent = os.path.abspath(args.parent)
        runs = dict(parent=dict(set_grid_host=[], bench=[]), this=dict(set_grid_host=[], bench=[]))
        for rep in range(3):
            for name, tree in (("parent", parent), ("this", REPO)):
                runs[name]["set_grid_host"].append(child(me + ["--step", "staging", "--source", "host", "--tree", tree], 240, cwd=tree)["ms_median"])
                line = child(bench + ["--steps", "3", "--warmup", "1"], 420, cwd=tree)
                runs[name]["bench"].append(dict(value=line["value"], ms_per_step=line["ms_per_step"]))
                result["c_parent"] = runs
                save()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
