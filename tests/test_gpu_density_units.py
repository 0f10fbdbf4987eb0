"""GPU: several density units (simulation_rho_cgs values) in one render (bl_set_density_units), and the flux fit built on them.

Every unit's image rows must be what a fresh render with that simulation_rho_cgs in the parameter block gives: the same bits in the
exact tier (and so the reference's golden for the fixture's own unit) and in the tolerant tier under bl_set_reproducible; where all
units share the tolerant tier's one pass, within the tier's tolerance of the exact tier. The geodesics and located samples are shared
by the units: one integration per render, and changing the units between renders of a series keeps the resident records."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

UNITS = [2.5e-17, 6.0e-17, 2.0e-16, 5.0e-16]   # the fixtures' own unit is 1e-16
MODELS = [(1.0, 10.0), (1.0, 80.0)]            # (R_low, R_high)


def _units(params):
    return UNITS + [float(params["simulation_rho_cgs"])]


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return fx, dict(params, **overrides), gu.golden_grid(mock_args)


def _render(params, grid, tier, units=None, pairs=None, reproducible=False, guard_band=None, switches=()):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        if switches:
            ctx.debug_set_switches(*switches)
        if guard_band is not None:
            ctx.debug_set_guard_band(guard_band)
        if pairs is not None:
            ctx.set_electron_models([h for _, h in pairs], rat_low=[lo for lo, _ in pairs])
        if units is not None:
            ctx.set_density_units(units)
        return ctx.render()


def _fresh(params, grid, tier, unit, pair=None, **kwargs):
    over = dict(simulation_rho_cgs=unit)
    if pair is not None:
        over.update(plasma_rat_low=pair[0], plasma_rat_high=pair[1])
    return _render(dict(params, **over), grid, tier, **kwargs)


def _check_units(got, params, grid, tier, units, pairs=None, **kwargs):
    n_m = len(pairs) if pairs else 1
    n_u = len(units)
    n_q = got["image"].shape[0] // (n_m * n_u)
    n_rays = got["image"].shape[1]
    assert got["image_by_unit"].shape == (n_m, n_u, n_q, n_rays)
    assert got["image_by_model"].shape == (n_m, n_u * n_q, n_rays)
    singles = []
    for m in range(n_m):
        for u, unit in enumerate(units):
            want = _fresh(params, grid, tier, unit, pairs[m] if pairs else None, **kwargs)
            assert want["image"].shape[0] == n_q
            assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
            assert gu.same_bits(got["image_by_unit"][m, u], want["image"]).all(), f"model {m} unit {u} {unit}"
            row = (m * n_u + u) * n_q
            assert gu.same_bits(got["image"][row:row + n_q], want["image"]).all()
            singles.append(want)
    return singles


@pytest.mark.parametrize("case, overrides", [
    ("sim_dp_interp", {}),
    ("sim_multifreq", {}),
    ("sim_cuts", {"cut_rho_min": 3.0e-18}),   # a density cut: each unit decides it on its own
    ("sim_aux_images", {}),
])
def test_exact_tier_equals_fresh_renders(case, overrides):
    fx, params, grid = _case(case, **overrides)
    units = _units(params)
    got = _render(params, grid, "exact", units)
    singles = _check_units(got, params, grid, "exact", units)
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic   # (one integration for all the units)
    assert got["stats"].launches_shade == len(units) * singles[0]["stats"].launches_shade
    assert not gu.same_bits(got["image_by_unit"][0, 0], got["image_by_unit"][0, 3]).all()   # (the units do differ)
    if case in ("sim_dp_interp", "sim_multifreq"):   # the fixture's own unit, last: the reference's bits
        n_pix = got["sample_num"].size
        assert gu.same_bits(got["image_by_unit"][0, -1], gu.expected_image(fx, "B", n_pix)).all()
    if "cut_rho_min" in overrides:   # (the cut does bite: without it the smallest unit renders otherwise)
        uncut = _fresh(dict(params, cut_rho_min=-1.0), grid, "exact", units[0])
        assert not gu.same_bits(uncut["image"], got["image_by_unit"][0, 0]).all()


def test_models_times_units_exact():
    fx, params, grid = _case("sim_multifreq")
    units = [4.0e-17, 1.0e-16, 3.0e-16]
    got = _render(params, grid, "exact", units, pairs=MODELS)
    singles = _check_units(got, params, grid, "exact", units, pairs=MODELS)
    assert got["stats"].launches_shade == 6 * singles[0]["stats"].launches_shade
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic


@pytest.mark.parametrize("case, overrides", [
    ("sim_aux_images", {}),
    ("sim_cuts", {"cut_rho_min": 3.0e-18}),
])
def test_tolerant_loop_equals_fresh_renders(case, overrides):
    """Where one pass does not apply: one shading pass per unit, the bits of fresh renders under bl_set_reproducible"""
    fx, params, grid = _case(case, **overrides)
    units = _units(params)
    got = _render(params, grid, "tolerant", units, reproducible=True)
    singles = _check_units(got, params, grid, "tolerant", units, reproducible=True)
    assert got["stats"].launches_shade == len(units) * singles[0]["stats"].launches_shade
    assert got["stats"].arithmetic == singles[0]["stats"].arithmetic


@pytest.mark.parametrize("case, overrides, switches", [
    ("sim_dp_interp", {}, ()),                                # one frequency, no spin
    ("sim_spin_fallback", {}, ()),                            # a spinning hole
    ("sim_multifreq", {}, ()),                                # three frequencies
    ("sim_multifreq", {"image_num_frequencies": 5}, ()),      # five
    ("sim_dp_interp", {}, ("NO_FUSED_LOCATE",)),              # a locate kernel + bl_shade_fast_kernel
])
@pytest.mark.parametrize("guard_band", [None, 1.0e-2])
@pytest.mark.parametrize("pairs", [None, MODELS], ids=["units", "models_x_units"])
def test_tolerant_one_pass(case, overrides, switches, guard_band, pairs):
    """The tolerant tier's hot path for a flux fit: one gather per sample whatever the number of units and models (launches_shade =
    n_chunks), each variant within the tier's tolerance of the exact tier's fresh render - also where a widened guard band leaves
    samples to the exact second pass"""
    fx, params, grid = _case(case, **overrides)
    units = _units(params)
    got = _render(params, grid, "tolerant", units, pairs=pairs, guard_band=guard_band, switches=switches)
    st = got["stats"]
    assert st.arithmetic == 1 and st.launches_shade == st.n_chunks and st.launches_transfer == st.n_chunks
    assert st.fused_variant == (0 if switches else 2)
    if guard_band is not None:
        assert st.n_deferred > 0
    for m, pair in enumerate(pairs or [None]):
        for u, unit in enumerate(units):
            exact = _fresh(params, grid, "exact", unit, pair)
            assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
            a, b = got["image_by_unit"][m, u], exact["image"]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            worst, _, _, same_support = gu.per_pixel_relative(a, b)
            assert worst < 1.0e-10 and same_support, (m, u, worst)


def test_one_unit_is_that_unit():
    fx, params, grid = _case("sim_dp_interp")
    for tier in ("exact", "tolerant"):
        got = _render(params, grid, tier, [3.0e-16], reproducible=True)
        want = _fresh(params, grid, tier, 3.0e-16, reproducible=True)
        assert got["image"].shape == want["image"].shape
        assert gu.same_bits(got["image"], want["image"]).all()
        assert np.array_equal(got["sample_num"], want["sample_num"])


def test_series_keeps_geodesics_when_units_change():
    import blacklight_amd as bl
    fx, params, grid = _case("sim_dp_interp")
    second = dataclasses.replace(grid, prim=grid.prim * np.float32(1.07))
    first_units, second_units = UNITS[:2], UNITS[2:]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(grid)
        ctx.set_density_units(first_units)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        ctx.set_grid(second)
        ctx.set_density_units(second_units)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        ctx.set_density_units([])   # back to the parameter block's unit: still the same records
        c = ctx.render()
        assert c["stats"].geodesics_reused == 1 and c["image"].shape[0] == b["image"].shape[0] // 2
    _check_units(a, params, grid, "exact", first_units)
    _check_units(b, params, second, "exact", second_units)
    assert gu.same_bits(c["image"], _render(params, second, "exact")["image"]).all()


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_fit_reaches_a_flux_the_frame_has(tier):
    import blacklight_amd as bl
    from blacklight_amd import flux
    fx, params, grid = _case("sim_dp_interp")
    p = bl.Params.from_dict(params)
    distance_pc = 8.1e3
    truth = 2.7e-16
    target = flux.total_flux_jy(_fresh(params, grid, tier, truth)["image"], p, distance_pc)
    assert target > 0.0
    with bl.Context(p) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        rho, got, renders = ctx.fit_density_unit(target, distance_pc, 1.0e-18, 1.0e-14, rtol=1.0e-4)
        assert ctx.density_units == [] and ctx.num_density_units == 0
        assert ctx.stats.geodesics_reused == 1   # (every render after the first shades resident geodesics)
    assert abs(got - target) <= 1.0e-4 * target and 1 <= renders <= 10
    again = flux.total_flux_jy(_fresh(params, grid, tier, rho)["image"], p, distance_pc)
    assert abs(again - target) <= 1.0e-4 * target
