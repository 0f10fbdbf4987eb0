"""Series of root-level frames of more than one chunk: 8 frames with geodesic reuse on against 8 with it off, in one process, for
  - a polarized 1024^2 series over the 256^3 mock (configuration 4's physics),
  - a 1024^2 x 64-frequency series (configuration 5's physics),
  - a 2048^2 unpolarized series (the benchmark's physics).
Per frame: render ms (host wall time of the call), n_chunks, geodesics_reused, the bytes of the records the stepper allocated; per
series the kept store's bytes as the library reports them (BLACKLIGHT_AMD_DEBUG_COUNTERS=1: DESIGN.md section 4a); and the
worst per-pixel distance from the reuse-off frame of the same snapshot. Writes profiles/series_chunked.json.
    python tools/gpu_series_chunked.py [--frames 8] [--series polarized1024,truecolor1024x64,plain2048] [--out profiles/series_chunked.json]"""
import argparse
import dataclasses
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch   # (before the library: see tests/test_gpu_defaults.py)

import bench
import blacklight_amd as bl
from blacklight_amd import mock

SERIES = {
    "polarized1024": dict(camera_resolution=1024, image_polarization=True, image_tau=True),
    "truecolor1024x64": dict(camera_resolution=1024, image_num_frequencies=64, image_frequency_start=1.5e11, image_frequency_end=3.3e11,
                             image_frequency_spacing="lin_wave"),
    "plain2048": dict(camera_resolution=2048),
}


def snapshots(grid, count):
    out = []
    for n in range(count):
        prim = grid.prim.copy()
        prim[0:2] *= np.float32(1.0 + 0.11 * n)
        out.append(dataclasses.replace(grid, prim=prim))
    return out


def store_records(path):
    """The kept layout's store as the library reports it with BLACKLIGHT_AMD_DEBUG_COUNTERS=1 (records; 64 bytes each)"""
    found = None
    with open(path) as f:
        for line in f:
            if line.startswith("kept layout:"):
                found = int(line.split("store ")[1].split()[0])
    return found


def run(params, snaps, reuse):
    frames = []
    with bl.Context(bl.Params.from_dict(params), device=0) as ctx:
        ctx.set_geodesic_reuse(reuse)
        for grid in snaps:
            ctx.set_grid(grid)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ctx.render()
            ms = 1000.0 * (time.perf_counter() - t0)
            st = out["stats"]
            frames.append(dict(image=out["image"], ms=ms, n_chunks=st.n_chunks, reused=st.geodesics_reused, ms_geodesic=st.ms_geodesic,
                               records=st.n_samples_emitted))
            print(f"  reuse {'on ' if reuse else 'off'} frame {len(frames)}: {ms:8.1f} ms, {st.n_chunks} chunks, reused {st.geodesics_reused}, "
                  f"geodesic {st.ms_geodesic:.1f} ms", flush=True)
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--series", default=",".join(SERIES))
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "series_chunked.json"))
    args = ap.parse_args()
    os.environ["BLACKLIGHT_AMD_DEBUG_COUNTERS"] = "1"   # (read by every new context: the kept layout's report on stderr)
    base = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    snaps = snapshots(base, args.frames)
    result = dict(frames=args.frames, grid=args.grid, device=torch.cuda.get_device_name(0), series={})
    for name in args.series.split(","):
        params = dict(bench.WORKLOAD, **SERIES[name])
        print(name, flush=True)
        # (the library's stderr to a file for the reuse-on series: its report of the store)
        log = args.out + "." + name + ".stderr"
        sys.stderr.flush()
        saved = os.dup(2)
        with open(log, "w") as f:
            os.dup2(f.fileno(), 2)
            try:
                on = run(params, snaps, True)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
        store = store_records(log)
        off = run(params, snaps, False)
        rows = []
        for a, b in zip(on, off):
            with np.errstate(invalid="ignore"):
                diff = np.abs(a["image"] - b["image"])
                scale = np.nanmax(np.abs(b["image"]))
            rows.append(dict(ms_on=round(a["ms"], 2), ms_off=round(b["ms"], 2), n_chunks_on=a["n_chunks"], n_chunks_off=b["n_chunks"],
                             geodesics_reused=a["reused"], records_allocated_bytes=64 * int(a["records"]), ms_geodesic_on=round(a["ms_geodesic"], 2), ms_geodesic_off=round(b["ms_geodesic"], 2),
                             nan_pattern_equal=bool(np.array_equal(np.isnan(a["image"]), np.isnan(b["image"]))),
                             max_abs_diff=float(np.nanmax(diff)) if diff.size else 0.0,
                             max_rel_diff=float(np.nanmax(diff) / scale) if scale > 0 else 0.0))
        kept = [r for r in rows if r["geodesics_reused"]]
        result["series"][name] = dict(params={k: v for k, v in SERIES[name].items()}, rows=rows,
                                      store_bytes=64 * store if store is not None else None,
                                      mean_ms_reused=round(float(np.mean([r["ms_on"] for r in kept])), 2) if kept else None,
                                      mean_ms_off_3_to_n=round(float(np.mean([r["ms_off"] for r in rows[2:]])), 2) if len(rows) > 2 else None)
        for n, r in enumerate(rows):
            print(f"  frame {n + 1}: on {r['ms_on']:8.1f} ms ({r['n_chunks_on']} chunks, reused {r['geodesics_reused']}) | off {r['ms_off']:8.1f} ms "
                  f"({r['n_chunks_off']} chunks) | max rel diff {r['max_rel_diff']:.3g}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
