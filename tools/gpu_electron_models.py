"""Several electron-temperature models in one render (bl_set_electron_models) against one fresh render per model.

    python tools/gpu_electron_models.py [--res 1024] [--grid 256] [--models 1,6,16] [--tiers exact,tolerant] [--reps 5]
                                        [--only K:TIER] [--out profiles/electron_models.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), thermal electrons, 230 GHz: bench.py's default workload. For every K and
tier: one render of K models (R_high swept from 1 to 160, R_low = 1) against K single-model renders, each in a context of its own
holding that pair - what a library of models costs without the call. Both integrate their geodesics (bl_set_geodesic_reuse(0));
bl_set_grid is outside the timed region of either, and every timed render follows an untimed one of the same context (the
first render of a context allocates its scratch). The two are alternated `reps` times; times are host wall clock between device
synchronisations. The per-pixel agreement of every model's image with its single-model render is
recorded (gu.per_pixel_relative; bits in the exact tier). --only K:TIER runs that one K-model render once (for a profiler).
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


def sweep(k):
    return [float(x) for x in np.geomspace(1.0, 160.0, k)] if k > 1 else [10.0]


def context(params, grid, tier, highs=None):
    ctx = bl.Context(bl.Params.from_dict(params), device=0)
    ctx.set_geodesic_reuse(False)
    ctx.set_arithmetic(tier)
    ctx.set_grid(grid)
    if highs is not None:
        ctx.set_electron_models(highs, rat_low=1.0)
    return ctx


def timed(ctx):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ctx.render()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--models", default="1,6,16")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "electron_models.json"))
    args = ap.parse_args()
    params = dict(bench.WORKLOAD, camera_resolution=args.res)
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    if args.only:
        k, tier = args.only.split(":")
        ctx = context(params, grid, tier, sweep(int(k)))
        ms, out = timed(ctx)
        print(json.dumps(dict(k=int(k), tier=tier, ms=ms, launches_shade=out["stats"].launches_shade)))
        ctx.close()
        return
    results = []
    for tier in args.tiers.split(","):
        for k in [int(x) for x in args.models.split(",")]:
            highs = sweep(k)
            multi = context(params, grid, tier, highs)
            timed(multi)   # (warm-up)
            multi_ms, single_ms = [], []
            single_images = [None] * k
            got = None
            for rep in range(args.reps):
                timed(multi)   # (each timed render right behind one of its own, as for the single-model contexts below)
                ms, got = timed(multi)
                multi_ms.append(ms)
                total = 0.0
                for m, high in enumerate(highs):
                    one = context(dict(params, plasma_rat_low=1.0, plasma_rat_high=high), grid, tier)
                    timed(one)   # (warm-up: a context's first render allocates its scratch)
                    ms, out = timed(one)
                    total += ms
                    single_images[m] = out["image"]
                    one.close()
                single_ms.append(total)
            st = got["stats"]
            agreement = []
            for m in range(k):
                worst, above, used, same_support = gu.per_pixel_relative(got["image_by_model"][m], single_images[m])
                agreement.append(dict(rat_high=highs[m], per_pixel_relative=worst, same_bits=bool(gu.same_bits(got["image_by_model"][m], single_images[m]).all()),
                                      same_nan=bool(np.array_equal(np.isnan(got["image_by_model"][m]), np.isnan(single_images[m]))), same_support=same_support))
            row = dict(tier=tier, k=k, rat_high=highs, multi_ms=multi_ms, singles_ms=single_ms,
                       ratio=float(np.median(multi_ms) / np.median(single_ms)), arithmetic=st.arithmetic,
                       launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade, ms_geodesic=st.ms_geodesic,
                       ms_shade=st.ms_shade, ms_transfer=st.ms_transfer, agreement=agreement)
            print(json.dumps({key: row[key] for key in ("tier", "k", "multi_ms", "singles_ms", "ratio")}), flush=True)
            results.append(row)
            multi.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(res=args.res, grid=args.grid, frequency_hz=params["image_frequency"], results=results), f, indent=1)


if __name__ == "__main__":
    main()
