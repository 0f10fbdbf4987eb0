"""GPU: several electron-temperature models in one render (bl_set_electron_models).

Every model's image rows must be what a fresh render with that (R_low, R_high) pair in the parameter block gives: the same bits in
the exact tier (and so the reference's golden for the fixture's own pair) and in the tolerant tier under bl_set_reproducible; the
tolerant tier within its stated tolerance of the exact tier. The geodesics and located samples are shared by the models: one
integration per render, and changing the models between renders of a series keeps the resident records."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

MODELS = [(1.0, 1.0), (1.0, 10.0), (1.0, 40.0), (1.0, 160.0)]   # (R_low, R_high); the fixtures' own pair is (1, 10)


def _pairs(params):
    return MODELS + [(float(params["plasma_rat_low"]), float(params["plasma_rat_high"]))]


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return fx, dict(params, **overrides), gu.golden_grid(mock_args)


def _render(params, grid, tier, pairs=None, reproducible=False, guard_band=None):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        if guard_band is not None:
            ctx.debug_set_guard_band(guard_band)
        if pairs is not None:
            ctx.set_electron_models([h for _, h in pairs], rat_low=[lo for lo, _ in pairs])
        return ctx.render()


def _fresh(params, grid, tier, pair, **kwargs):
    return _render(dict(params, plasma_rat_low=pair[0], plasma_rat_high=pair[1]), grid, tier, **kwargs)


def _check_models(got, params, grid, tier, pairs, **kwargs):
    n_q = got["image"].shape[0] // len(pairs)
    assert got["image_by_model"].shape == (len(pairs), n_q, got["image"].shape[1])
    singles = []
    for m, pair in enumerate(pairs):
        want = _fresh(params, grid, tier, pair, **kwargs)
        assert want["image"].shape[0] == n_q
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        assert gu.same_bits(got["image_by_model"][m], want["image"]).all(), f"model {m} {pair}"
        assert gu.same_bits(got["image"][m * n_q:(m + 1) * n_q], want["image"]).all()
        singles.append(want)
    return singles


@pytest.mark.parametrize("case", ["sim_dp_interp", "sim_multifreq", "sim_pole", "sim_cuts", "sim_aux_images"])
def test_exact_tier_equals_fresh_renders(case):
    fx, params, grid = _case(case)
    pairs = _pairs(params)
    got = _render(params, grid, "exact", pairs)
    singles = _check_models(got, params, grid, "exact", pairs)
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic   # (one integration for all the models)
    assert got["stats"].launches_shade == len(pairs) * singles[0]["stats"].launches_shade
    assert not gu.same_bits(got["image_by_model"][0], got["image_by_model"][3]).all()   # (the models do differ)
    if case in ("sim_dp_interp", "sim_multifreq"):   # the fixture's own pair, last: the reference's bits
        n_pix = got["sample_num"].size
        assert gu.same_bits(got["image_by_model"][-1], gu.expected_image(fx, "B", n_pix)).all()


@pytest.mark.parametrize("case, overrides", [
    ("sim_cuts", {"cut_theta_e_min": 2.0}),   # a Theta_e cut: each model decides it on its own
    ("sim_aux_images", {}),
])
def test_tolerant_loop_equals_fresh_renders(case, overrides):
    """Where one pass does not apply: one shading pass per model, the bits of fresh renders under bl_set_reproducible"""
    fx, params, grid = _case(case, **overrides)
    pairs = _pairs(params)
    got = _render(params, grid, "tolerant", pairs, reproducible=True)
    singles = _check_models(got, params, grid, "tolerant", pairs, reproducible=True)
    one = _render(params, grid, "tolerant", pairs[:1], reproducible=True)
    assert got["stats"].launches_shade == len(pairs) * one["stats"].launches_shade
    assert got["stats"].arithmetic == singles[0]["stats"].arithmetic


def test_renderings_come_out_once():
    """A rendering no model enters (density, sigma, 1 / beta): the one a fresh render gives, beside every model's image"""
    fx, params, grid = _case("sim_render")
    pairs = _pairs(params)
    got = _render(params, grid, "exact", pairs)
    singles = _check_models(got, params, grid, "exact", pairs)
    assert gu.same_bits(got["rendering"], singles[0]["rendering"]).all()


@pytest.mark.parametrize("case, overrides, switches", [
    ("sim_dp_interp", {}, ()),                                # one frequency, no spin: bl_shade_fused2_kernel<true, ...>
    ("sim_spin_fallback", {}, ()),                            # a spinning hole: bl_shade_fused2_kernel<false, ...>
    ("sim_multifreq", {}, ()),                                # three frequencies
    ("sim_multifreq", {"image_num_frequencies": 5}, ()),      # five: the tier's factor path as it was
    ("sim_dp_interp", {}, ("NO_FUSED_LOCATE",)),              # a locate kernel + bl_shade_fast_kernel
])
@pytest.mark.parametrize("guard_band", [None, 1.0e-2])
def test_tolerant_one_pass(case, overrides, switches, guard_band):
    """The tolerant tier's hot path for a library of models: one gather per sample whatever the number of models (launches_shade
    as with one model), each model's image within the tier's tolerance of the exact tier's - also where a widened guard band leaves
    samples to the exact second pass, which stores the same model-free rows"""
    import blacklight_amd as bl
    fx, params, grid = _case(case, **overrides)
    pairs = _pairs(params)
    exact = _render(params, grid, "exact", pairs)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic("tolerant")
        if switches:
            ctx.debug_set_switches(*switches)
        if guard_band is not None:
            ctx.debug_set_guard_band(guard_band)
        ctx.set_electron_models([h for _, h in pairs], rat_low=[lo for lo, _ in pairs])
        got = ctx.render()
        ctx.set_electron_models(pairs[0][1], rat_low=pairs[0][0])
        one = ctx.render()
    st = got["stats"]
    assert st.arithmetic == 1 and st.launches_shade == one["stats"].launches_shade == st.n_chunks
    assert st.fused_variant == (0 if switches else 2)
    if guard_band is not None:
        assert st.n_deferred > 0
    assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
    for m in range(len(pairs)):
        a, b = got["image_by_model"][m], exact["image_by_model"][m]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        worst, _, _, same_support = gu.per_pixel_relative(a, b)
        assert worst < 1.0e-10 and same_support, (m, worst)
    worst, _, _, _ = gu.per_pixel_relative(got["image_by_model"][0], one["image"])
    assert worst < 1.0e-12


def test_one_model_is_that_pair():
    fx, params, grid = _case("sim_dp_interp")
    for tier in ("exact", "tolerant"):
        got = _render(params, grid, tier, [(2.0, 40.0)], reproducible=True)
        want = _fresh(params, grid, tier, (2.0, 40.0), reproducible=True)
        assert got["image"].shape == want["image"].shape
        assert gu.same_bits(got["image"], want["image"]).all()
        assert np.array_equal(got["sample_num"], want["sample_num"])


def test_series_keeps_geodesics_when_models_change():
    import blacklight_amd as bl
    fx, params, grid = _case("sim_dp_interp")
    second = dataclasses.replace(grid, prim=grid.prim * np.float32(1.07))
    first_pairs, second_pairs = MODELS[:2], MODELS[2:]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(grid)
        ctx.set_electron_models([h for _, h in first_pairs], rat_low=[lo for lo, _ in first_pairs])
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        ctx.set_grid(second)
        ctx.set_electron_models([h for _, h in second_pairs], rat_low=[lo for lo, _ in second_pairs])
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        ctx.set_electron_models([])   # back to the parameter block's pair: still the same records
        c = ctx.render()
        assert c["stats"].geodesics_reused == 1 and c["image"].shape[0] == b["image"].shape[0] // 2
    _check_models(a, params, grid, "exact", first_pairs)
    _check_models(b, params, second, "exact", second_pairs)
    assert gu.same_bits(c["image"], _render(params, second, "exact")["image"]).all()
