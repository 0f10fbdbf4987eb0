#!/usr/bin/env python3
"""What staging iharm3d-family primitives from device memory costs (bl_set_grid_device_harm: transpose and primitive conversion in
the staging kernel) beside staging converted planes (bl_set_grid_device) and beside converting on the host (bl_harm_convert_host +
bl_set_grid). Writes profiles/harm_device.json.

    python tools/gpu_harm_device.py [--out profiles/harm_device.json] [--parent DIR] [--shape 288 128 128 8]

Every GPU step is a child process of its own under `timeout -k 10`; the first that fails ends the job (its output is shown).
  (a) headline  one process, one array of n1 x n2 x n3 x n_prim float32 in device memory: the first call of each kind (tables and
                all), then five calls on the geometry in place - median, min, max of the wall time - of set_grid_device_harm,
                harm_convert_device, set_grid_device from the converted planes, and convert_host + set_grid on the host; the device
                call's bytes (n_prim x 4 B read + 32 B written per cell, the point table apart) per second of wall time against the
                6.29 TB/s a float4 copy reaches on this part.
  (b) parent    with --parent DIR (a built tree of the parent commit): three alternating processes of either tree for
                bl_set_grid_device from float32 [var][block] at 256^3 (tools/gpu_device_grid.py's staging step, which both trees
                have) and for bench.py's default line: the plain form of the staging kernel is meant to cost what it cost.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12   # float4 copy, bytes per second (read + write), measured on an MI355X


class Planes:
    """Converted planes on the host with the grid's description for them: what Context.set_grid takes"""

    def __init__(self, grid, planes):
        self.grid, self.planes = grid, planes

    def desc(self):
        from blacklight_amd import _capi
        d = _capi.GridDesc.from_buffer_copy(self.grid.desc(converted=True))
        d.prim = self.planes.ctypes.data if self.planes is not None else None   # (None: the cells are in device memory)
        return d


def step_headline(args):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    import blacklight_amd as bl
    from blacklight_amd import _capi
    from blacklight_amd.snapshot import HarmGrid
    n1, n2, n3, n_prim = args.shape
    params = dict(bench.WORKLOAD, simulation_coord="sks", simulation_a=0.0, plasma_gamma=13.0 / 9.0)
    p = bl.Params.from_dict(params)
    header = _capi.HarmHeader()
    header.n1, header.n2, header.n3, header.n_prim = n1, n2, n3, n_prim
    r_in, r_out = 1.2, 1000.0   # (an iharm3d MKS grid: log r uniform, hslope 0.3)
    header.startx[0], header.startx[1], header.startx[2] = math.log(r_in), 0.0, 0.0
    header.dx[0], header.dx[1], header.dx[2] = (math.log(r_out) - math.log(r_in)) / n1, 1.0 / n2, 2.0 * math.pi / n3
    header.a, header.hslope, header.metric = 0.0, 0.3, _capi.BL_HARM_MKS
    header.gam, header.gam_p, header.gam_e = 13.0 / 9.0, float("nan"), float("nan")
    for index, name in enumerate(("ind_rho", "ind_uu", "ind_u1", "ind_u2", "ind_u3", "ind_b1", "ind_b2", "ind_b3")):
        setattr(header, name, index)
    header.ind_kappa = -1
    t0 = time.perf_counter()
    grid = HarmGrid(p, header)
    ms_grid = 1000.0 * (time.perf_counter() - t0)
    rng = np.random.default_rng(1)
    prims = (rng.random((n1, n2, n3, n_prim), dtype=np.float32) * np.float32(0.1)) + np.float32(0.01)
    n_cells = n1 * n2 * n3
    torch.cuda.set_device(0)
    on_device = torch.from_numpy(prims).cuda()

    def timed(call, count):
        times = []
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append(1000.0 * (time.perf_counter() - t0))
        return times

    def summary(times):
        later = times[1:]
        return dict(ms_first_call=times[0], ms_median=statistics.median(later), ms_min=min(later), ms_max=max(later), calls=len(later))

    line = dict(shape=[n1, n2, n3, n_prim], n_cells=n_cells, ms_harm_grid_create=ms_grid)
    with bl.Context(p, device=0) as ctx:
        ctx.set_arithmetic("tolerant")
        line["set_grid_device_harm"] = summary(timed(lambda: ctx.set_grid_device_harm(grid, on_device, stream=None), 6))
        line["set_grid_device_harm"]["host_bytes_last_call"] = ctx.grid_host_bytes
        out = torch.empty((8, n3, n2, n1), dtype=torch.float32, device=on_device.device)
        line["harm_convert_device"] = summary(timed(lambda: ctx.harm_convert_device(grid, on_device, out=out, stream=None), 6))
        converted = Planes(grid, None)
        planes_5d = out[:, None]
        line["set_grid_device_converted"] = summary(timed(lambda: ctx.set_grid_device(converted, planes_5d, stream=None), 6))
        host_times = dict(convert=[], set_grid=[])

        def on_host():
            t0 = time.perf_counter()
            planes = grid.convert_host(prims)
            t1 = time.perf_counter()
            ctx.set_grid(Planes(grid, planes))
            host_times["convert"].append(1000.0 * (t1 - t0))
            host_times["set_grid"].append(1000.0 * (time.perf_counter() - t1))
        line["convert_host_plus_set_grid"] = summary(timed(on_host, 6))
        line["convert_host_plus_set_grid"].update(ms_convert_median=statistics.median(host_times["convert"][1:]),
                                                  ms_set_grid_median=statistics.median(host_times["set_grid"][1:]))
        same = bool(torch.equal(out.cpu(), torch.from_numpy(grid.convert_host(prims))))
        line["device_planes_equal_host_planes"] = same
    for name, read in (("set_grid_device_harm", 4 * n_prim), ("harm_convert_device", 4 * n_prim), ("set_grid_device_converted", 32)):
        moved = (read + 32) * n_cells
        line[name].update(kernel_bytes=moved, bytes_per_s_of_wall_min=moved / (line[name]["ms_min"] * 1.0e-3),
                          frac_of_float4_copy_rate=moved / (line[name]["ms_min"] * 1.0e-3) / COPY_RATE)
    print(json.dumps(line), flush=True)
    if not same:
        sys.exit("the device conversion differs from the host conversion")


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harm_device.json"))
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit, for (b)")
    ap.add_argument("--parts", default="ab", help="which of (a), (b) to measure; the other is kept as --out has it")
    ap.add_argument("--shape", type=int, nargs=4, default=[288, 128, 128, 8])
    ap.add_argument("--step", choices=["headline"], default=None, help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step == "headline":
        return step_headline(args)
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result.update(float4_copy_rate_bytes_per_s=COPY_RATE)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    if "a" in args.parts:
        result["a_headline"] = child([sys.executable, os.path.abspath(__file__), "--step", "headline", "--shape"] + [str(n) for n in args.shape], 420)
        save()
    if "b" in args.parts and args.parent:
        parent = os.path.abspath(args.parent)
        runs = dict(parent=dict(set_grid_device_256=[], bench=[]), this=dict(set_grid_device_256=[], bench=[]))
        for rep in range(3):
            for name, tree in (("parent", parent), ("this", REPO)):
                staging = child([sys.executable, os.path.join(tree, "tools", "gpu_device_grid.py"), "--step", "staging", "--source", "device_f32_vb", "--tree", tree],
                                240, cwd=tree)
                runs[name]["set_grid_device_256"].append(dict(ms_median=staging["ms_median"], ms_min=staging["ms_min"], ms_max=staging["ms_max"]))
                line = child([sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline", "--steps", "3", "--warmup", "1"], 420, cwd=tree)
                runs[name]["bench"].append(dict(value=line["value"], ms_per_step=line["ms_per_step"]))
                result["b_parent"] = runs
                save()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
