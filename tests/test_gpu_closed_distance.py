"""GPU: the Dormand-Prince stepper with the proper distance in closed form (blacklight_amd/csrc/bl_distance_closed.h) against the same
render under BL_SWITCH_EXACT_DISTANCE, the reference's operations in every stage.

The proper distance enters nothing but the number of samples an accepted step emits, so a render in closed mode must give the switch
leg's sample_num, sample_flags, n_samples_emitted and image: bit for bit in the exact tier and in the tolerant tier under
set_reproducible, to the 1e-10 per pixel of the exact tier with composed maps. The `stepper:` line of BLACKLIGHT_AMD_DEBUG_COUNTERS says
which form a render used (distance=closed|exact|none), how many steps the closed form left undecided and whether the frame was
therefore rendered a second time. BL_SWITCH_WIDE_DISTANCE_BAND widens the band to 0.25 in the count, which leaves a step of nearly
every ray undecided: it exercises the second render, the context's memory of the camera, and what may be kept of either attempt."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu
from test_gpu_mirror_pairs import _grid as _modulated_grid, _params as _bench_params

pytestmark = pytest.mark.gpu

FALLBACK = dict(fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)
_KEPT = {}


def _line(err, head):
    lines = [line for line in err.splitlines() if line.startswith(head)]
    assert len(lines) == 1, (head, lines)
    return dict(word.split("=", 1) for word in lines[0][len(head):].split() if "=" in word)


def _render(capfd, monkeypatch, params, grid, tier="exact", reproducible=False, switches=(), tail=None, reuse=None, scratch=None, grids=None, renders=1):
    """`renders` renders in one context; per render the outputs with "stats", "stepper" and "kernels" (the debug lines, parsed)."""
    import blacklight_amd as bl
    monkeypatch.setenv("BLACKLIGHT_AMD_DEBUG_COUNTERS", "1")   # (read when the context is created)
    outs = []
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        ctx.debug_set_switches(*switches)
        if tail is not None:
            ctx.set_tail_policy(tail)
        if reuse is not None:
            ctx.set_geodesic_reuse(reuse)
        if scratch is not None:
            ctx.set_scratch_limit(scratch)
        for n in range(renders):
            if grids is not None:
                ctx.set_grid(grids[n])
            elif grid is not None and n == 0:
                ctx.set_grid(grid)
            capfd.readouterr()
            out = ctx.render()
            err = capfd.readouterr().err
            out["stats"] = ctx.stats
            out["stepper"] = _line(err, "stepper: ")
            out["kernels"] = _line(err, "kernels: ")
            outs.append(out)
    return outs


def _pair(capfd, monkeypatch, params, grid, key=None, switches=(), **how):
    """(default leg, BL_SWITCH_EXACT_DISTANCE leg) of one configuration; the switch leg of a `key` is rendered once and shared"""
    got, = _render(capfd, monkeypatch, params, grid, switches=switches, **how)
    if key is None or key not in _KEPT:
        leg, = _render(capfd, monkeypatch, params, grid, switches=tuple(switches) + ("EXACT_DISTANCE",), **how)
        assert leg["stepper"]["distance"] in ("exact", "none") and leg["stepper"]["retried"] == "0"
        if key is None:
            return got, leg
        _KEPT[key] = leg
    return got, _KEPT[key]


def _same(got, leg, bits=True):
    assert np.array_equal(got["sample_num"], leg["sample_num"])
    assert np.array_equal(got["sample_flags"], leg["sample_flags"])
    a, b = got["stats"], leg["stats"]
    assert (a.n_rays, a.n_samples, a.n_samples_emitted, a.n_flagged, a.max_sample_num) == (b.n_rays, b.n_samples, b.n_samples_emitted, b.n_flagged, b.max_sample_num)
    if bits:
        assert np.array_equal(got["image"].view(np.int64), leg["image"].view(np.int64))


def _closed(out):
    assert out["stepper"] == dict(distance="closed", undecided="0", retried="0"), out["stepper"]


# ---------------------------------------------------------------------------------------------------- the benchmark's stepper, a = 0
@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("res", [32, 64])
def test_zero_spin_simulation_frame(capfd, monkeypatch, res, pairs):
    params = dict(_bench_params(), camera_resolution=res)
    mirror = () if pairs else ("NO_MIRROR_PAIRS",)
    exact, exact_leg = _pair(capfd, monkeypatch, params, _modulated_grid(), key=("sim", res, pairs, "exact"), switches=mirror, tier="exact")
    _closed(exact)
    assert exact["kernels"]["geodesic"] == "<DP,0,1,0>" and exact["stats"].mirror_pairs == (1 if pairs else 0)
    _same(exact, exact_leg)
    tolerant, tolerant_leg = _pair(capfd, monkeypatch, params, _modulated_grid(), switches=mirror, tier="tolerant", reproducible=True)
    _closed(tolerant)
    _same(tolerant, tolerant_leg)
    composed, _ = _pair(capfd, monkeypatch, params, _modulated_grid(), key=("sim", res, pairs, "exact"), switches=mirror, tier="tolerant")
    _closed(composed)
    assert composed["stats"].composed_maps == 1
    _same(composed, exact_leg, bits=False)
    assert np.array_equal(np.isnan(composed["image"]), np.isnan(exact_leg["image"]))
    a, b = composed["image"], exact_leg["image"]
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.nanmax(np.where(b != 0.0, np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny), np.abs(a - b)))
    print("composed maps in closed mode against the exact tier under the switch: worst relative difference per pixel", worst)
    assert worst <= 1.0e-10


# ---------------------------------------------------------------------------------------------------- any spin, large s
@pytest.mark.parametrize("res", [16, 32])
def test_formula_frame_with_spin_from_r_1000(capfd, monkeypatch, res):
    fx, params, _ = gu.load_case("formula_dp")
    for tier in ("exact", "tolerant"):
        got, leg = _pair(capfd, monkeypatch, dict(params, camera_resolution=res), None, tier=tier, reproducible=True, tail="wide")
        _closed(got)
        assert got["kernels"]["geodesic"] == "<DP,0,0,0>"
        _same(got, leg)


def test_formula_frame_whose_last_rays_are_parked_stays_exact(capfd, monkeypatch):
    fx, params, _ = gu.load_case("formula_dp")
    got, leg = _pair(capfd, monkeypatch, dict(params, camera_resolution=64), None, tier="exact")
    assert got["stepper"] == dict(distance="exact", undecided="0", retried="0") and any("quad" in stage for stage in got["kernels"])
    _same(got, leg)


# ---------------------------------------------------------------------------------------------------- the stepper's other paths
@pytest.mark.parametrize("name", ["few_steps", "flat", "time", "shell"])
def test_golden_cases(capfd, monkeypatch, name):
    case, over, geodesic = {"few_steps": ("sim_few_steps", {}, None), "flat": ("formula_flat", {}, None),
                            "time": ("sim_aux_images", dict(camera_resolution=32), "<DP,1,1,0>"),
                            "shell": ("sim_dp_interp", dict(FALLBACK, camera_r=100.0), "<DP,0,1,1>")}[name]
    fx, params, mock_args = gu.load_case(case)
    grid = gu.golden_grid(mock_args) if mock_args is not None else None
    for tier in ("exact", "tolerant"):
        got, leg = _pair(capfd, monkeypatch, dict(params, **over), grid, tier=tier, reproducible=True, tail="wide")
        _closed(got)
        assert geodesic is None or got["kernels"]["geodesic"] == geodesic
        if name == "few_steps":
            assert got["stats"].n_flagged > 0   # (rays that run out of ray_max_steps)
        _same(got, leg)


@pytest.mark.parametrize("case", ["sim_rk4", "sim_rk2"])
def test_fixed_step_steppers_have_no_distance(capfd, monkeypatch, case):
    fx, params, mock_args = gu.load_case(case)
    got, leg = _pair(capfd, monkeypatch, params, gu.golden_grid(mock_args), tier="exact")
    assert got["stepper"] == dict(distance="none", undecided="0", retried="0") == leg["stepper"]
    _same(got, leg)


def test_a_render_that_writes_a_geodesic_checkpoint_stays_exact(capfd, monkeypatch, tmp_path):
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    params = dict(params, checkpoint_geodesic_save="true", checkpoint_geodesic_file=str(tmp_path / "geo.bin"))
    got, = _render(capfd, monkeypatch, params, gu.golden_grid(mock_args), tier="exact", tail="wide")
    assert got["stepper"] == dict(distance="exact", undecided="0", retried="0")


# ---------------------------------------------------------------------------------------------------- the second render
def _wide(capfd, monkeypatch, **how):
    params = _bench_params()
    return _render(capfd, monkeypatch, params, _modulated_grid(), switches=("WIDE_DISTANCE_BAND",), **how)


def _exact_leg(capfd, monkeypatch, tier, reproducible=False, **how):
    key = ("wide", tier, reproducible, tuple(sorted(how.items())))
    if key not in _KEPT:
        _KEPT[key], = _render(capfd, monkeypatch, _bench_params(), _modulated_grid(), switches=("EXACT_DISTANCE",), tier=tier, reproducible=reproducible, **how)
    return _KEPT[key]


@pytest.mark.parametrize("tier,reproducible", [("exact", False), ("tolerant", True)])
def test_an_undecided_step_renders_the_frame_again(capfd, monkeypatch, tier, reproducible):
    got, = _wide(capfd, monkeypatch, tier=tier, reproducible=reproducible)
    print("wide band:", got["stepper"])
    assert got["stepper"]["distance"] == "exact" and got["stepper"]["retried"] == "1" and int(got["stepper"]["undecided"]) > 0
    assert got["stats"].launches_geodesic == got["stats"].n_chunks == 1
    _same(got, _exact_leg(capfd, monkeypatch, tier, reproducible))


def test_the_camera_is_remembered(capfd, monkeypatch):
    first, second = _wide(capfd, monkeypatch, tier="exact", reuse=False, renders=2)
    assert first["stepper"]["retried"] == "1"
    assert second["stepper"] == dict(distance="exact", undecided="0", retried="0") and second["stats"].geodesics_reused == 0
    leg = _exact_leg(capfd, monkeypatch, "exact")
    _same(first, leg)
    _same(second, leg)


def test_a_series_reuses_the_second_render_s_records(capfd, monkeypatch):
    first = _modulated_grid()
    grids = [first]
    for factor in (1.07, 0.93):
        prim = first.prim.copy()
        prim[0:2] *= np.float32(factor)
        grids.append(dataclasses.replace(first, prim=prim))
    frames = _wide(capfd, monkeypatch, tier="exact", reuse=True, grids=grids, renders=3)
    legs = _render(capfd, monkeypatch, _bench_params(), None, switches=("EXACT_DISTANCE",), tier="exact", reuse=True, grids=grids, renders=3)
    assert frames[0]["stepper"]["retried"] == "1" and frames[0]["stats"].geodesics_reused == 0
    for got, leg in zip(frames, legs):
        _same(got, leg)
    for got in frames[1:]:
        assert got["stats"].geodesics_reused == 1 and got["stats"].launches_geodesic == 0
        assert got["stepper"] == dict(distance="none", undecided="0", retried="0")


def test_the_second_render_in_several_chunks(capfd, monkeypatch):
    cap = 2000 * 16384   # (ray_max_steps of the frame x 16 KiB: a few rays' worst case per chunk)
    got, = _wide(capfd, monkeypatch, tier="exact", scratch=cap)
    print("several chunks:", got["stats"].n_chunks, got["stepper"])
    assert got["stats"].n_chunks >= 2 and got["stats"].launches_geodesic == got["stats"].n_chunks
    assert got["stepper"]["distance"] == "exact" and got["stepper"]["retried"] == "1"
    _same(got, _exact_leg(capfd, monkeypatch, "exact", scratch=cap))
