"""Several polarized variants in one render (bl_set_polarized_variants) against one fresh render per variant.

    python tools/gpu_polarized_variants.py [--res 1024] [--grid 256] [--variants 1,2,6,16] [--tiers exact,tolerant] [--reps 5]
                                           [--only V:TIER] [--out profiles/polarized_variants.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), full Stokes and the optical-depth row, 230 GHz: bench.py's polarized1024
workload. For every V and tier: one render of V (R_low, R_high, unit) triples - R_high swept over 1 ... 160, the unit log-evenly over
0.1 ... 10 times the workload's - against V renders, each in a context of its own with that triple in its parameter block: what a
sweep costs without the call, on code the call does not touch. Both integrate their geodesics (bl_set_geodesic_reuse(0)); bl_set_grid
is outside the timed region of either, and every timed render follows an untimed one of the same context (a context's first render
allocates its scratch). The two are alternated `reps` times; times are host wall clock between device synchronisations, medians
are compared, and the fresh renders' own run-to-run spread - (max - min) / median of their per-repetition sums - is recorded beside
the ratio. Every variant's rows are compared with its fresh render's bit for bit. --only V:TIER runs that one V-variant render once
(for a profiler).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bench  # noqa: E402
import blacklight_amd as bl  # noqa: E402
import golden_util as gu  # noqa: E402
from blacklight_amd import mock  # noqa: E402


def triple_sweep(rho0, v):
    """(R_low, R_high, unit) x v"""
    if v == 1:
        return [(1.0, 40.0, 2.0 * rho0)]
    highs = np.geomspace(1.0, 160.0, v)
    units = np.geomspace(0.1 * rho0, 10.0 * rho0, v)[::-1]   # (a fit's pattern: the hotter the electrons, the smaller the unit)
    return [(1.0, float(h), float(u)) for h, u in zip(highs, units)]


def context(params, grid, tier, triples=None):
    ctx = bl.Context(bl.Params.from_dict(params), device=0)
    ctx.set_geodesic_reuse(False)
    ctx.set_arithmetic(tier)
    ctx.set_grid(grid)
    if triples is not None:
        ctx.set_polarized_variants([h for _, h, _ in triples], [u for _, _, u in triples], rat_low=[lo for lo, _, _ in triples])
    return ctx


def timed(ctx):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ctx.render()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def compare(params, grid, tier, triples, reps):
    multi = context(params, grid, tier, triples)
    timed(multi)   # (warm-up)
    multi_ms, fresh_sum_ms, fresh_each_ms = [], [], []
    fresh_images = [None] * len(triples)
    fresh_stats = None
    got = None
    for rep in range(reps):
        timed(multi)   # (each timed render right behind one of its own, as for the fresh contexts below)
        ms, got = timed(multi)
        multi_ms.append(ms)
        each = []
        for v, (low, high, unit) in enumerate(triples):
            one = context(dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit), grid, tier)
            timed(one)   # (warm-up: a context's first render allocates its scratch)
            ms, out = timed(one)
            each.append(ms)
            fresh_images[v] = out["image"]
            fresh_stats = out["stats"]
            one.close()
        fresh_each_ms.append(each)
        fresh_sum_ms.append(sum(each))
    st = got["stats"]
    same = [bool(gu.same_bits(got["image_by_variant"][v], fresh_images[v]).all()) for v in range(len(triples))]
    multi.close()
    fresh_median = float(np.median(fresh_sum_ms))
    return dict(tier=tier, n_variants=len(triples), triples=triples, multi_ms=multi_ms, fresh_sum_ms=fresh_sum_ms, fresh_each_ms=fresh_each_ms,
                multi_median_ms=float(np.median(multi_ms)), fresh_median_ms=fresh_median, ratio=float(np.median(multi_ms) / fresh_median),
                multi_spread=float((max(multi_ms) - min(multi_ms)) / np.median(multi_ms)),
                fresh_spread=float((max(fresh_sum_ms) - min(fresh_sum_ms)) / fresh_median),
                arithmetic=st.arithmetic, n_chunks=st.n_chunks, launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade,
                launches_transfer=st.launches_transfer, ms_geodesic=st.ms_geodesic, ms_locate=st.ms_locate, ms_shade=st.ms_shade,
                ms_transfer=st.ms_transfer, fresh_n_chunks=fresh_stats.n_chunks, fresh_ms_geodesic=fresh_stats.ms_geodesic,
                fresh_ms_shade=fresh_stats.ms_shade, fresh_ms_transfer=fresh_stats.ms_transfer, same_bits=same, all_same_bits=all(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--variants", default="1,2,6,16")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "polarized_variants.json"))
    args = ap.parse_args()
    params = dict(bench.WORKLOAD, camera_resolution=args.res, image_polarization=True, image_tau=True)
    rho0 = float(params["simulation_rho_cgs"])
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    if args.only:
        v, tier = args.only.split(":")
        ctx = context(params, grid, tier, triple_sweep(rho0, int(v)))
        ms, out = timed(ctx)
        print(json.dumps(dict(v=int(v), tier=tier, ms=ms, n_chunks=out["stats"].n_chunks, launches_shade=out["stats"].launches_shade)))
        ctx.close()
        return
    results = []

    def save():   # (after every row: a run cut short keeps what it measured)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(res=args.res, grid=args.grid, frequency_hz=params["image_frequency"], simulation_rho_cgs=rho0, reps=args.reps,
                           results=results), f, indent=1)

    for tier in args.tiers.split(","):
        for v in [int(x) for x in args.variants.split(",") if x]:
            row = compare(params, grid, tier, triple_sweep(rho0, v), args.reps)
            print(json.dumps({key: row[key] for key in ("tier", "n_variants", "multi_median_ms", "fresh_median_ms", "ratio", "multi_spread",
                                                        "fresh_spread", "n_chunks", "launches_shade", "ms_geodesic", "ms_shade",
                                                        "ms_transfer", "all_same_bits")}), flush=True)
            results.append(row)
            save()


if __name__ == "__main__":
    main()
