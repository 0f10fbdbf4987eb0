"""GPU: several sigma cuts (cut_sigma_max values) in one render (bl_set_sigma_cuts).

Every cut's image rows must be what a fresh render with that cut_sigma_max in the parameter block gives: the same bits in the exact tier
(and so the reference's golden for the fixtures' own value, 1.0) and in the tolerant tier under bl_set_reproducible; where all cuts share
the tolerant tier's one pass - the coefficient kernels run with the sigma upper cut off and leave sigma in the sample's row, a transfer
lane per (ray, model, unit, cut, frequency) compares it - within the tier's tolerance of the exact tier. Geodesics and located samples are
shared by the cuts: one integration per render, and changing the cuts between renders of a series keeps the resident records.

Fresh renders are made once per (fixture, tier, values) and shared by the tests of this module."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

CUTS = [0.01, 0.1, 1.0, 10.0, -1.0]            # the fixtures' own value is 1.0; -1: the cut off
EDGES = [0.0, 1.0000001]                       # everything with a field cut; a value next to another
MODELS = [(1.0, 10.0), (1.0, 80.0)]            # (R_low, R_high)
UNITS = [6.0e-17, 2.0e-16]

_CASES, _FRESH = {}, {}


def _case(name, **overrides):
    key = (name, tuple(sorted(overrides.items())))
    if key not in _CASES:
        fx, params, mock_args = gu.load_case(name)
        _CASES[key] = (fx, dict(params, **overrides), gu.golden_grid(mock_args))
    return _CASES[key]


def _render(params, grid, tier, cuts=None, pairs=None, units=None, reproducible=False, guard_band=None, switches=()):
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
        if cuts is not None:
            ctx.set_sigma_cuts(cuts)
        return ctx.render()


def _fresh(case_key, params, grid, tier, cut, pair=None, unit=None, reproducible=False):
    """A render of its own with the values in the parameter block (made once, left unchanged)."""
    key = (case_key, tier, cut, pair, unit, reproducible)
    if key not in _FRESH:
        over = dict(cut_sigma_max=cut)
        if pair is not None:
            over.update(plasma_rat_low=pair[0], plasma_rat_high=pair[1])
        if unit is not None:
            over.update(simulation_rho_cgs=unit)
        got = _render(dict(params, **over), grid, tier, reproducible=reproducible)
        for name in ("image", "sample_num", "sample_flags"):
            got[name].setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def _check_cuts(got, case_key, params, grid, tier, cuts, pairs=None, units=None, reproducible=False):
    """Row ((m U + u) S + s) n_q + q is row q of a fresh render of model m at unit u under cut s: the same bits."""
    n_m, n_u, n_s = len(pairs) if pairs else 1, len(units) if units else 1, len(cuts)
    n_q = got["image"].shape[0] // (n_m * n_u * n_s)
    n_rays = got["image"].shape[1]
    assert got["image_by_cut"].shape == (n_m, n_u, n_s, n_q, n_rays)
    assert got["image_by_unit"].shape == (n_m, n_u, n_s * n_q, n_rays) and got["image_by_model"].shape == (n_m, n_u * n_s * n_q, n_rays)
    singles = []
    for m in range(n_m):
        for u in range(n_u):
            for s, cut in enumerate(cuts):
                want = _fresh(case_key, params, grid, tier, cut, pairs[m] if pairs else None, units[u] if units else None, reproducible)
                assert want["image"].shape[0] == n_q
                assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
                assert gu.same_bits(got["image_by_cut"][m, u, s], want["image"]).all(), f"model {m} unit {u} cut {s} ({cut})"
                row = ((m * n_u + u) * n_s + s) * n_q
                assert gu.same_bits(got["image"][row:row + n_q], want["image"]).all()
                singles.append(want)
    return singles


@pytest.mark.parametrize("case, overrides", [
    ("sim_dp_interp", {}),
    ("sim_multifreq", {}),
    ("sim_aux_images", {}),
    ("sim_cuts", {}),                               # cuts on rho, B and 1 / beta and the geometric ones beside the sigma cut
    ("sim_dp_interp", {"cut_b_max": 30.0}),         # ... and a field-strength cut that bites beside thresholds that all bite
])
def test_exact_tier_equals_fresh_renders(case, overrides):
    fx, params, grid = _case(case, **overrides)
    key = (case, tuple(sorted(overrides.items())))
    cuts = CUTS + EDGES
    got = _render(params, grid, "exact", cuts)
    singles = _check_cuts(got, key, params, grid, "exact", cuts)
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic == 1   # (one integration for all the cuts)
    assert got["stats"].launches_shade == len(cuts) * singles[0]["stats"].launches_shade
    by_cut = got["image_by_cut"][0, 0]
    if case == "sim_cuts":
        # (its geometric cuts leave no cell with sigma > 0.01 - the CPU oracle says so: thresholds from 0.01 up render one image; that
        # the sigma cut decides anything here shows at 0, which cuts every cell with a field)
        assert not gu.same_bits(by_cut[cuts.index(0.0)], by_cut[cuts.index(-1.0)]).all()
    else:
        for s in range(len(CUTS) - 1):   # images of neighbouring thresholds differ
            assert not gu.same_bits(by_cut[s], by_cut[s + 1]).all(), (CUTS[s], CUTS[s + 1])
        assert not gu.same_bits(by_cut[cuts.index(0.0)], by_cut[0]).all()
    if not overrides and case in ("sim_dp_interp", "sim_multifreq"):   # the fixture's own cut: the reference's bits
        n_pix = got["sample_num"].size
        assert gu.same_bits(by_cut[cuts.index(1.0)], gu.expected_image(fx, "B", n_pix)).all()


def test_models_times_units_times_cuts_exact():
    fx, params, grid = _case("sim_multifreq")
    cuts = [0.1, 1.0, -1.0]
    got = _render(params, grid, "exact", cuts, pairs=MODELS, units=UNITS)
    singles = _check_cuts(got, ("sim_multifreq", ()), params, grid, "exact", cuts, pairs=MODELS, units=UNITS)
    assert got["stats"].launches_shade == 12 * singles[0]["stats"].launches_shade
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic


def test_tolerant_loop_equals_fresh_renders():
    """Where one pass does not apply (auxiliary rows): one shading pass per cut, the bits of fresh renders under bl_set_reproducible"""
    fx, params, grid = _case("sim_aux_images")
    got = _render(params, grid, "tolerant", CUTS, reproducible=True)
    singles = _check_cuts(got, ("sim_aux_images", ()), params, grid, "tolerant", CUTS, reproducible=True)
    assert got["stats"].launches_shade == len(CUTS) * singles[0]["stats"].launches_shade
    assert got["stats"].arithmetic == singles[0]["stats"].arithmetic


@pytest.mark.parametrize("case, overrides, switches", [
    ("sim_dp_interp", {}, ()),                                # one frequency, no spin
    ("sim_spin_fallback", {}, ()),                            # a spinning hole
    ("sim_multifreq", {}, ()),                                # three frequencies
    ("sim_multifreq", {"image_num_frequencies": 5}, ()),      # five
    ("sim_dp_interp", {}, ("NO_FUSED_LOCATE",)),              # a locate kernel + bl_shade_fast_kernel
])
@pytest.mark.parametrize("guard_band", [None, 1.0e-2])
@pytest.mark.parametrize("product", [False, True], ids=["cuts", "models_x_units_x_cuts"])
def test_tolerant_one_pass(case, overrides, switches, guard_band, product):
    """The tolerant tier's hot path: one gather per sample whatever the number of cuts, units and models (launches_shade = n_chunks),
    each variant within the tier's tolerance of the exact tier's fresh render - also where a widened guard band leaves the samples
    near any of the thresholds to the exact second pass, whose rows carry the exact tier's sigma"""
    fx, params, grid = _case(case, **overrides)
    key = (case, tuple(sorted(overrides.items())))
    pairs, units = (MODELS, UNITS) if product else (None, None)
    got = _render(params, grid, "tolerant", CUTS, pairs=pairs, units=units, guard_band=guard_band, switches=switches)
    st = got["stats"]
    assert st.arithmetic == 1 and st.launches_shade == st.n_chunks and st.launches_transfer == st.n_chunks
    assert st.fused_variant == (0 if switches else 2)
    if guard_band is not None:
        assert st.n_deferred > 0
    for m, pair in enumerate(pairs or [None]):
        for u, unit in enumerate(units or [None]):
            for s, cut in enumerate(CUTS):
                exact = _fresh(key, params, grid, "exact", cut, pair, unit)
                assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
                a, b = got["image_by_cut"][m, u, s], exact["image"]
                assert np.array_equal(np.isnan(a), np.isnan(b))
                worst, _, _, same_support = gu.per_pixel_relative(a, b)
                assert worst < 1.0e-10 and same_support, (m, u, s, cut, worst)


def test_one_cut_is_that_cut():
    fx, params, grid = _case("sim_dp_interp")
    for tier in ("exact", "tolerant"):
        for cut in (0.1, -1.0):
            got = _render(params, grid, tier, [cut], reproducible=True)
            want = _fresh(("sim_dp_interp", ()), params, grid, tier, cut, reproducible=True)
            assert got["image"].shape == want["image"].shape
            assert gu.same_bits(got["image"], want["image"]).all(), (tier, cut)
            assert np.array_equal(got["sample_num"], want["sample_num"])
            assert got["stats"].launches_shade == want["stats"].launches_shade


def test_series_keeps_geodesics_when_cuts_change():
    import blacklight_amd as bl
    fx, params, grid = _case("sim_dp_interp")
    second = dataclasses.replace(grid, prim=grid.prim * np.float32(1.07))
    first_cuts, second_cuts = CUTS[:2], CUTS[2:4]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(grid)
        ctx.set_sigma_cuts(first_cuts)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        ctx.set_grid(second)
        ctx.set_sigma_cuts(second_cuts)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        ctx.set_sigma_cuts([])   # back to the parameter block's cut, the single image: still the same records
        c = ctx.render()
        assert c["stats"].geodesics_reused == 1 and c["image"].shape[0] == b["image"].shape[0] // 2
        assert ctx.sigma_cuts == [] and ctx.num_sigma_cuts == 0
    _check_cuts(a, ("sim_dp_interp", ()), params, grid, "exact", first_cuts)
    _check_cuts(b, ("sim_dp_interp", "second grid"), params, second, "exact", second_cuts)
    assert gu.same_bits(c["image"], _render(params, second, "exact")["image"]).all()
