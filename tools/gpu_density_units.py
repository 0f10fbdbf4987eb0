"""Several density units in one render (bl_set_density_units) against one fresh render per unit, and a flux fit on top of them.

    python tools/gpu_density_units.py [--res 1024] [--grid 256] [--units 1,6,16] [--models-x-units 6x8] [--tiers exact,tolerant]
                                      [--reps 3] [--no-fit] [--only K:TIER] [--out profiles/density_units.json]

1024^2 camera over the 256^3 mock (blacklight_amd.mock), thermal electrons, 230 GHz: bench.py's default workload. For every K and
tier: one render of K density units (simulation_rho_cgs swept log-evenly over 0.1 ... 10 times the workload's) against K renders,
each in a context of its own holding that unit - what a flux fit costs without the call; then the same for M electron models
(R_high over 1 ... 160) times U units against M * U fresh renders. Both integrate their geodesics (bl_set_geodesic_reuse(0));
bl_set_grid is outside the timed region of either, and every timed render follows an untimed one of the same context (the first
render of a context allocates its scratch). The two are alternated `reps` times; times are host wall clock between device
synchronisations. The per-pixel agreement of every variant's image with its fresh render is recorded (gu.per_pixel_relative;
bits in the exact tier).

The fit: Context.fit_density_unit to the total flux (blacklight_amd.flux, Sgr A*'s mass and distance as in the workload) that a
fresh render at 2.7 times the workload's unit has, bracket [0.01, 100] times the unit, against the same search with one fresh context
per trial unit (warm-up and bl_set_grid untimed, the timed renders summed). --only K:TIER runs that one K-unit render once (for a
profiler).
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
from blacklight_amd import flux, mock  # noqa: E402

DISTANCE_PC = 8.1e3


def unit_sweep(rho0, k):
    return [float(x) for x in np.geomspace(0.1 * rho0, 10.0 * rho0, k)] if k > 1 else [2.0 * rho0]


def model_sweep(k):
    return [float(x) for x in np.geomspace(1.0, 160.0, k)] if k > 1 else [10.0]


def context(params, grid, tier, units=None, highs=None):
    ctx = bl.Context(bl.Params.from_dict(params), device=0)
    ctx.set_geodesic_reuse(False)
    ctx.set_arithmetic(tier)
    ctx.set_grid(grid)
    if highs is not None:
        ctx.set_electron_models(highs, rat_low=1.0)
    if units is not None:
        ctx.set_density_units(units)
    return ctx


def timed(ctx):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ctx.render()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def compare(params, grid, tier, units, highs, reps):
    """One render of every (model, unit) against one fresh render each, alternated"""
    multi = context(params, grid, tier, units, highs)
    timed(multi)   # (warm-up)
    variants = [(h, u) for h in (highs or [None]) for u in units]
    multi_ms, single_ms = [], []
    single_images = [None] * len(variants)
    got = None
    for rep in range(reps):
        timed(multi)   # (each timed render right behind one of its own, as for the fresh contexts below)
        ms, got = timed(multi)
        multi_ms.append(ms)
        total = 0.0
        for v, (high, unit) in enumerate(variants):
            over = dict(simulation_rho_cgs=unit)
            if high is not None:
                over.update(plasma_rat_low=1.0, plasma_rat_high=high)
            one = context(dict(params, **over), grid, tier)
            timed(one)   # (warm-up: a context's first render allocates its scratch)
            ms, out = timed(one)
            total += ms
            single_images[v] = out["image"]
            one.close()
        single_ms.append(total)
    st = got["stats"]
    n_u = len(units)
    agreement = []
    for v, (high, unit) in enumerate(variants):
        mine = got["image_by_unit"][v // n_u, v % n_u]
        worst, above, used, same_support = gu.per_pixel_relative(mine, single_images[v])
        agreement.append(dict(rat_high=high, rho_cgs=unit, per_pixel_relative=worst, same_bits=bool(gu.same_bits(mine, single_images[v]).all()),
                              same_nan=bool(np.array_equal(np.isnan(mine), np.isnan(single_images[v]))), same_support=same_support))
    multi.close()
    return dict(tier=tier, n_units=len(units), n_models=len(highs) if highs else 0, rho_cgs=units, rat_high=highs, multi_ms=multi_ms,
                singles_ms=single_ms, ratio=float(np.median(multi_ms) / np.median(single_ms)), arithmetic=st.arithmetic,
                launches_geodesic=st.launches_geodesic, launches_shade=st.launches_shade, launches_transfer=st.launches_transfer,
                ms_geodesic=st.ms_geodesic, ms_shade=st.ms_shade, ms_transfer=st.ms_transfer,
                worst_per_pixel_relative=max(a["per_pixel_relative"] for a in agreement),
                all_same_bits=all(a["same_bits"] for a in agreement), agreement=agreement)


def fresh_fit(params, grid, tier, target, lo, hi, rtol, per_render):
    """fit_density_unit's search, one fresh context per trial unit: (unit, flux, searches, fresh renders, summed render ms)"""
    p = bl.Params.from_dict(params)
    a, b, steps, renders, total = lo, hi, 0, 0, 0.0
    while steps < 64:
        trial = np.geomspace(a, b, per_render)
        trial[0], trial[-1] = a, b
        fluxes = []
        for unit in trial:
            one = context(dict(params, simulation_rho_cgs=float(unit)), grid, tier)
            timed(one)
            ms, out = timed(one)
            total += ms
            renders += 1
            fluxes.append(flux.total_flux_jy(out["image"], p, DISTANCE_PC))
            one.close()
        steps += 1
        fluxes = np.array(fluxes)
        best = int(np.nanargmin(np.abs(fluxes - target)))
        if abs(fluxes[best] - target) <= rtol * target:
            return float(trial[best]), float(fluxes[best]), steps, renders, total
        k = [i for i in range(per_render - 1) if (fluxes[i] - target) * (fluxes[i + 1] - target) <= 0.0][0]
        a, b = float(trial[k]), float(trial[k + 1])
    raise RuntimeError("fresh fit did not converge")


def fit(params, grid, tier, rho0, rtol=1.0e-3, per_render=16):
    p = bl.Params.from_dict(params)
    truth = 2.7 * rho0
    one = context(dict(params, simulation_rho_cgs=truth), grid, tier)
    timed(one)
    target = flux.total_flux_jy(timed(one)[1]["image"], p, DISTANCE_PC)
    one.close()
    ctx = bl.Context(p, device=0)   # (geodesic reuse on, as a fit runs it)
    ctx.set_arithmetic(tier)
    ctx.set_grid(grid)
    timed(ctx)   # (warm-up: scratch allocated, as for the fresh contexts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rho, got, renders = ctx.fit_density_unit(target, DISTANCE_PC, 0.01 * rho0, 100.0 * rho0, rtol=rtol, per_render=per_render)
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    ctx.close()
    f_rho, f_got, f_steps, f_renders, f_ms = fresh_fit(params, grid, tier, target, 0.01 * rho0, 100.0 * rho0, rtol, per_render)
    return dict(tier=tier, target_jy=target, truth_rho_cgs=truth, rtol=rtol, per_render=per_render, rho_cgs=rho, flux_jy=got,
                renders=renders, fit_ms=fit_ms, fresh_rho_cgs=f_rho, fresh_flux_jy=f_got, fresh_steps=f_steps, fresh_renders=f_renders,
                fresh_render_ms=f_ms, ratio=fit_ms / f_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--units", default="1,6,16")
    ap.add_argument("--models-x-units", default="6x8")
    ap.add_argument("--tiers", default="exact,tolerant")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "density_units.json"))
    args = ap.parse_args()
    params = dict(bench.WORKLOAD, camera_resolution=args.res)
    rho0 = float(params["simulation_rho_cgs"])
    grid = mock.generate(n_r=args.grid, n_th=args.grid, n_ph=args.grid)
    if args.only:
        k, tier = args.only.split(":")
        ctx = context(params, grid, tier, unit_sweep(rho0, int(k)))
        ms, out = timed(ctx)
        print(json.dumps(dict(k=int(k), tier=tier, ms=ms, launches_shade=out["stats"].launches_shade)))
        ctx.close()
        return
    results, fits = [], []
    m_x_u = [int(x) for x in args.models_x_units.split("x")] if args.models_x_units else None

    def save():   # (after every row: a run cut short keeps what it measured)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(res=args.res, grid=args.grid, frequency_hz=params["image_frequency"], distance_pc=DISTANCE_PC,
                           simulation_rho_cgs=rho0, reps=args.reps, results=results, fits=fits), f, indent=1)

    for tier in args.tiers.split(","):
        for k in [int(x) for x in args.units.split(",") if x]:
            row = compare(params, grid, tier, unit_sweep(rho0, k), None, args.reps)
            print(json.dumps({key: row[key] for key in ("tier", "n_units", "multi_ms", "singles_ms", "ratio", "worst_per_pixel_relative",
                                                        "all_same_bits")}), flush=True)
            results.append(row)
            save()
        if m_x_u:
            row = compare(params, grid, tier, unit_sweep(rho0, m_x_u[1]), model_sweep(m_x_u[0]), args.reps)
            print(json.dumps({key: row[key] for key in ("tier", "n_models", "n_units", "multi_ms", "singles_ms", "ratio",
                                                        "worst_per_pixel_relative", "all_same_bits")}), flush=True)
            results.append(row)
            save()
        if not args.no_fit:
            row = fit(params, grid, tier, rho0)
            print(json.dumps(row), flush=True)
            fits.append(row)
            save()


if __name__ == "__main__":
    main()
