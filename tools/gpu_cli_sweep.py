#!/usr/bin/env python3
"""A sweep from the .input file against one command-line run per variant: wall clock of whole processes.

    python tools/gpu_cli_sweep.py --single-exe <bin/blacklight_amd of the commit before the sweep keys> [--res 1024] [--grid 256]
                                  [--cases 6x1,6x8,pol6] [--reps 3] [--tier tolerant] [--out profiles/cli_sweep.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock, written once as a raw grid: what bin/blacklight_amd reads without an HDF5
writer at hand - ONE snapshot per process; a raw grid cannot be a numbered series), bench.py's workload at 230 GHz. Cases: 6 electron
models x 1 density unit, 6 x 8, and 6 polarized (R_low, R_high, unit) triples with the optical-depth row. For every case one process
of this tree's binary with the sweep keys - V files - against V processes of --single-exe (default: this tree's binary), each with
one variant in its parameter block - the same V files -, alternated `reps` times. Every process is a fresh child under its own
`timeout -k 10`; the script ends at the first one that fails. Recorded per process: wall clock around the child, and the timing block
it prints (elapsed, geodesics, reading = read + stage, sampling, image, and - sweep runs - the time in the writer), so that read / stage /
render / write are separable; per case: medians, (max - min) / median of both sides, their ratio, and whether every pair of files is
byte for byte the same but for the ZIP time stamps. Measured, not asserted.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench  # noqa: E402
import sweep_util as su  # noqa: E402
from blacklight_amd import mock  # noqa: E402
from blacklight_amd.params import _format  # noqa: E402

EXE = os.path.join(REPO, "blacklight_amd", "bin", "blacklight_amd")
LINES = {"elapsed_s": "Elapsed time:", "geodesics_s": "Integrating geodesics:", "reading_s": "Reading simulation:", "sampling_s": "Sampling simulation:",
         "image_s": "Integrating image:", "writing_s": "writing outputs:"}


def run(exe, input_path, env, limit):
    t0 = time.perf_counter()
    done = subprocess.run(["timeout", "-k", "10", str(limit), exe, input_path], capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t0
    if done.returncode != 0:
        sys.exit(f"{exe} {input_path}: exit status {done.returncode}\n{done.stdout[-2000:]}{done.stderr[-2000:]}")
    row = dict(wall_s=wall)
    for key, label in LINES.items():
        found = re.search(re.escape(label) + r"\s+([0-9.e+-]+) s", done.stdout)
        if found:
            row[key] = float(found.group(1))
    return row


def write_input(path, params):
    with open(path, "w") as f:
        for key, value in params.items():
            f.write(f"{key} = {value if isinstance(value, str) else _format(value)}\n")
    return path


def cases(rho0):
    highs = [1.0, 10.0, 20.0, 40.0, 80.0, 160.0]
    units = [float(u) for u in np.geomspace(0.25 * rho0, 4.0 * rho0, 8)]
    triples = [(1.0, h, float(u)) for h, u in zip(highs, np.geomspace(4.0 * rho0, 0.25 * rho0, 6))]
    return {
        "6x1": dict(polarized=False, keys=dict(sweep_rat_low=su.comma([1.0] * 6), sweep_rat_high=su.comma(highs)),
                    variants=[(1.0, h, rho0) for h in highs], tags=[f"m{m:02d}u00" for m in range(6)]),
        "6x8": dict(polarized=False, keys=dict(sweep_rat_low=su.comma([1.0] * 6), sweep_rat_high=su.comma(highs), sweep_rho_cgs=su.comma(units)),
                    variants=[(1.0, h, u) for h in highs for u in units], tags=[f"m{m:02d}u{u:02d}" for m in range(6) for u in range(8)]),
        "pol6": dict(polarized=True, keys=dict(sweep_rat_low=su.comma(t[0] for t in triples), sweep_rat_high=su.comma(t[1] for t in triples),
                                               sweep_rho_cgs=su.comma(t[2] for t in triples)),
                     variants=triples, tags=[f"v{v:02d}" for v in range(6)]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single-exe", default=EXE)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--cases", default="6x1,6x8,pol6")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tier", default="tolerant")
    ap.add_argument("--limit", type=int, default=120, help="seconds for one process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cli_sweep.json"))
    args = ap.parse_args()
    env = dict(os.environ, BLACKLIGHT_AMD_ARITHMETIC=args.tier)
    work = tempfile.mkdtemp(prefix="cli_sweep_")
    grid_path = os.path.join(work, "grid.blgrid")
    mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid).save_raw(grid_path)
    base = dict(bench.WORKLOAD, camera_resolution=args.res, simulation_file=grid_path, simulation_multiple=False, output_format="npz")
    rho0 = float(base["simulation_rho_cgs"])
    result = dict(res=args.res, grid=args.grid, tier=args.tier, reps=args.reps, snapshots_per_process=1,
                  single_exe="this tree's binary" if os.path.abspath(args.single_exe) == EXE else "the parent commit's binary", cases={})

    def save():   # (after every case: a run cut short keeps what it measured)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    for name in args.cases.split(","):
        case = cases(rho0)[name]
        params = dict(base, image_polarization=True, image_tau=True) if case["polarized"] else dict(base)
        sweep_out = os.path.join(work, f"{name}_sweep.npz")
        sweep_input = write_input(os.path.join(work, f"{name}_sweep.input"), dict(params, output_file=sweep_out, **case["keys"]))
        single_inputs = [write_input(os.path.join(work, f"{name}_single_{v}.input"),
                                     dict(params, output_file=os.path.join(work, f"{name}_single_{v}.npz"), plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=rho))
                         for v, (low, high, rho) in enumerate(case["variants"])]
        run(EXE, sweep_input, env, args.limit)   # (one untimed process of either kind first: the grid file into the page cache)
        run(args.single_exe, single_inputs[0], env, args.limit)
        sweep_rows, single_rows = [], []
        for rep in range(args.reps):
            sweep_rows.append(run(EXE, sweep_input, env, args.limit))
            single_rows.append([run(args.single_exe, path, env, args.limit) for path in single_inputs])
            print(f"{name} repetition {rep}: sweep {sweep_rows[-1]['wall_s']:.2f} s, {len(single_inputs)} single runs {sum(r['wall_s'] for r in single_rows[-1]):.2f} s", flush=True)
        same = [su.file_bytes(sweep_out.replace(".npz", f".{tag}.npz")) == su.file_bytes(os.path.join(work, f"{name}_single_{v}.npz"))
                for v, tag in enumerate(case["tags"])]
        sweep_wall = [r["wall_s"] for r in sweep_rows]
        single_wall = [sum(r["wall_s"] for r in rows) for rows in single_rows]
        sums = {key: [sum(r.get(key, 0.0) for r in rows) for rows in single_rows] for key in LINES if key != "writing_s"}
        result["cases"][name] = dict(
            n_variants=len(case["variants"]), sweep_runs=sweep_rows, single_sum_wall_s=single_wall, single_sum_by_line_s=sums,
            single_first_rep=single_rows[0], sweep_median_s=float(np.median(sweep_wall)), single_median_s=float(np.median(single_wall)),
            ratio=float(np.median(sweep_wall) / np.median(single_wall)),
            sweep_spread=float((max(sweep_wall) - min(sweep_wall)) / np.median(sweep_wall)),
            single_spread=float((max(single_wall) - min(single_wall)) / np.median(single_wall)),
            files_equal_but_for_zip_time_stamps=same, all_files_equal=all(same),
            note="tolerant tier with composed maps: two renders agree to rounding, not bit for bit; --tier exact for equal files" if args.tier == "tolerant" else "")
        save()
        print(name, json.dumps({k: result["cases"][name][k] for k in ("n_variants", "sweep_median_s", "single_median_s", "ratio", "sweep_spread", "single_spread", "all_files_equal")}), flush=True)
    for name in os.listdir(work):
        os.remove(os.path.join(work, name))
    os.rmdir(work)


if __name__ == "__main__":
    main()
