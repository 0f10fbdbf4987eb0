"""GPU: several electron mixes (thermal plus power-law electrons) of an unpolarized run in one render (bl_set_electron_mixes).

Every mix's image rows must be what a fresh render with that mix's four plasma_* values in the parameter block gives: the same bits in
the exact tier (and so the reference's golden for sim_powerlaw's own mix) and, where a pass per variant runs, in the tolerant tier under
bl_set_reproducible; where all mixes share the tolerant tier's one pass - the coefficient kernels write the mix-free row with a thermal
fraction of 1, a transfer workgroup per (256 rays, mix, model, unit, cut, frequency) applies its mix - within the tier's tolerance of the
exact tier. Geodesics and located samples are shared by the mixes: one integration per render, and changing the list between renders of a
series keeps the resident records.

Fresh renders are made once per (fixture, tier, values) and shared by the tests of this module."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

THERMAL = dict(power_frac=0.0, p=2.5, gamma_min=1.0, gamma_max=1000.0)
OWN = dict(power_frac=0.3, p=2.5, gamma_min=1.0, gamma_max=1000.0)            # sim_powerlaw's own mix
MIXES = [THERMAL, OWN, dict(power_frac=0.5, p=3.5, gamma_min=10.0, gamma_max=1.0e5), dict(power_frac=0.05, p=2.2, gamma_min=2.0, gamma_max=500.0)]
PURE = dict(power_frac=1.0, p=2.8, gamma_min=5.0, gamma_max=1.0e4)            # no thermal part
MODELS = [(1.0, 10.0), (1.0, 80.0)]            # (R_low, R_high)
UNITS = [6.0e-17, 2.0e-16]
CUTS = [1.0, -1.0]

_CASES, _FRESH = {}, {}


def _case(name, **overrides):
    key = (name, tuple(sorted(overrides.items())))
    if key not in _CASES:
        fx, params, mock_args = gu.load_case(name)
        _CASES[key] = (fx, dict(params, **overrides), gu.golden_grid(mock_args))
    return _CASES[key]


def _block(mix):
    return {"plasma_" + key: value for key, value in mix.items()}


def _mix_key(mix):
    return None if mix is None else tuple(sorted(mix.items()))


def _render(params, grid, tier, mixes=None, pairs=None, units=None, cuts=None, reproducible=False, guard_band=None, switches=(), cameras=None):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        if switches:
            ctx.debug_set_switches(*switches)
        if guard_band is not None:
            ctx.debug_set_guard_band(guard_band)
        if cameras is not None:
            ctx.set_cameras([th for th, _ in cameras], [ph for _, ph in cameras])
        if pairs is not None:
            ctx.set_electron_models([h for _, h in pairs], rat_low=[lo for lo, _ in pairs])
        if units is not None:
            ctx.set_density_units(units)
        if cuts is not None:
            ctx.set_sigma_cuts(cuts)
        if mixes is not None:
            ctx.set_electron_mixes(mixes)
        return ctx.render()


def _fresh(case_key, params, grid, tier, mix, pair=None, unit=None, cut=None, reproducible=False):
    """A render of its own with the values in the parameter block and no list set (made once, left unchanged)."""
    key = (case_key, tier, _mix_key(mix), pair, unit, cut, reproducible)
    if key not in _FRESH:
        over = _block(mix) if mix is not None else {}
        if pair is not None:
            over.update(plasma_rat_low=pair[0], plasma_rat_high=pair[1])
        if unit is not None:
            over.update(simulation_rho_cgs=unit)
        if cut is not None:
            over.update(cut_sigma_max=cut)
        got = _render(dict(params, **over), grid, tier, reproducible=reproducible)
        for name in ("image", "sample_num", "sample_flags"):
            got[name].setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def _variants(mixes, pairs, units, cuts):
    return [(e, m, u, s) for e in range(len(mixes)) for m in range(len(pairs) if pairs else 1) for u in range(len(units) if units else 1)
            for s in range(len(cuts) if cuts else 1)]


def _check_bits(got, case_key, params, grid, tier, mixes, pairs=None, units=None, cuts=None, reproducible=False):
    """Row (((e M + m) U + u) S + s) n_q + q is row q of a fresh render of mix e, model m, unit u and cut s: the same bits."""
    n_e, n_m, n_u, n_s = len(mixes), len(pairs) if pairs else 1, len(units) if units else 1, len(cuts) if cuts else 1
    n_q, n_rays = got["image"].shape[0] // (n_e * n_m * n_u * n_s), got["image"].shape[1]
    assert got["image_by_mix"].shape == (n_e, n_m * n_u * n_s * n_q, n_rays)
    assert got["image_by_cut"].shape == (n_e, n_m, n_u, n_s, n_q, n_rays)
    assert got["image_by_unit"].shape == (n_e, n_m, n_u, n_s * n_q, n_rays) and got["image_by_model"].shape == (n_e, n_m, n_u * n_s * n_q, n_rays)
    assert got["stats"].n_mixes == n_e
    singles = []
    for e, m, u, s in _variants(mixes, pairs, units, cuts):
        want = _fresh(case_key, params, grid, tier, mixes[e], pairs[m] if pairs else None, units[u] if units else None, cuts[s] if cuts else None, reproducible)
        assert want["image"].shape[0] == n_q
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        assert gu.same_bits(got["image_by_cut"][e, m, u, s], want["image"]).all(), f"mix {e} model {m} unit {u} cut {s}"
        row = (((e * n_m + m) * n_u + u) * n_s + s) * n_q
        assert gu.same_bits(got["image"][row:row + n_q], want["image"]).all()
        singles.append(want)
    return singles


def _check_tolerance(got, case_key, params, grid, mixes, pairs=None, units=None, cuts=None):
    """Every variant within the tolerant tier's contract of the exact tier's fresh render; the worst distance."""
    worst_of_all = 0.0
    for e, m, u, s in _variants(mixes, pairs, units, cuts):
        exact = _fresh(case_key, params, grid, "exact", mixes[e], pairs[m] if pairs else None, units[u] if units else None, cuts[s] if cuts else None)
        assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
        a, b = got["image_by_cut"][e, m, u, s], exact["image"]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        worst, _, _, same_support = gu.per_pixel_relative(a, b)
        print(f"electron mixes, {case_key}: mix {e} model {m} unit {u} cut {s}: worst per-pixel distance {worst:.3e}")
        assert worst < 1.0e-10 and same_support, (e, m, u, s, worst)
        worst_of_all = max(worst_of_all, worst)
    return worst_of_all


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the exact tier
@pytest.mark.parametrize("case", ["sim_powerlaw", "sim_dp_interp", "sim_multifreq"])
def test_exact_tier_equals_fresh_renders(case):
    fx, params, grid = _case(case)
    got = _render(params, grid, "exact", MIXES)
    singles = _check_bits(got, (case, ()), params, grid, "exact", MIXES)
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic == 1   # (one integration for all the mixes)
    assert got["stats"].launches_shade == len(MIXES) * singles[0]["stats"].launches_shade
    by_mix = got["image_by_mix"]
    for e in range(len(MIXES) - 1):   # images of neighbouring mixes differ
        assert not gu.same_bits(by_mix[e], by_mix[e + 1]).all(), e
    if case == "sim_powerlaw":        # the fixture's own mix: the reference's bits
        assert gu.same_bits(by_mix[MIXES.index(OWN)], gu.expected_image(fx, "B", got["sample_num"].size)).all()


def test_the_product_exact():
    fx, params, grid = _case("sim_multifreq")
    mixes = [MIXES[0], MIXES[2]]
    got = _render(params, grid, "exact", mixes, pairs=MODELS, units=UNITS, cuts=CUTS)
    singles = _check_bits(got, ("sim_multifreq", ()), params, grid, "exact", mixes, pairs=MODELS, units=UNITS, cuts=CUTS)
    assert got["stats"].launches_shade == 16 * singles[0]["stats"].launches_shade
    assert got["stats"].launches_geodesic == singles[0]["stats"].launches_geodesic


# ---------------------------------------------------------------------------------------------------------------- 3: passes, tolerant
def test_tolerant_passes_equal_fresh_renders():
    """A variant without a thermal part forces a pass per variant: under bl_set_reproducible the bits of fresh tolerant renders"""
    fx, params, grid = _case("sim_powerlaw")
    mixes = MIXES + [PURE]
    got = _render(params, grid, "tolerant", mixes, reproducible=True)
    singles = _check_bits(got, ("sim_powerlaw", ()), params, grid, "tolerant", mixes, reproducible=True)
    assert got["stats"].launches_shade == len(mixes) * singles[0]["stats"].launches_shade


def test_tolerant_runs_times_the_product():
    """Two runs of different kinds - the second starts at row offset 8 n_q - over models x units x cuts: every row the bits of its
    fresh render (a wrong row offset of a run, or a wrong (unit, cut) block of cut thresholds in a run's passes, shows here), and the
    context holds after the render what was set before it.
    (Before the runs became ranges the plan receives, the thermal run of this list still took the one pass over models x units x
    cuts: launches_shade 9, its eight images within 1.0e-14 per pixel of their fresh renders and not their bits - DESIGN.md 4h.)"""
    import blacklight_amd as bl
    fx, params, grid = _case("sim_powerlaw")
    mixes = [THERMAL, PURE]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic("tolerant")
        ctx.set_reproducible(True)
        n_q = ctx.num_quantities
        ctx.set_electron_models([h for _, h in MODELS], rat_low=[lo for lo, _ in MODELS])
        ctx.set_density_units(UNITS)
        ctx.set_sigma_cuts(CUTS)
        ctx.set_electron_mixes(mixes)
        before = (ctx.num_electron_mixes, ctx.electron_mixes, ctx.num_variants, ctx.num_quantities, ctx._variants())
        assert before[0] == 2 and before[2:4] == (16, 16 * n_q)
        assert [{key: mix[key] for key in THERMAL} for mix in before[1]] == mixes
        got = ctx.render()
        assert (ctx.num_electron_mixes, ctx.electron_mixes, ctx.num_variants, ctx.num_quantities, ctx._variants()) == before
    singles = _check_bits(got, ("sim_powerlaw", ()), params, grid, "tolerant", mixes, pairs=MODELS, units=UNITS, cuts=CUTS, reproducible=True)
    st = got["stats"]
    assert st.n_mixes == 2
    assert st.launches_shade == 16 * singles[0]["stats"].launches_shade
    assert 1 <= st.launches_geodesic <= 2


# ---------------------------------------------------------------------------------------------------------------- 4, 5: one pass
@pytest.mark.parametrize("case, overrides, switches", [
    ("sim_dp_interp", {}, ()),                                # one frequency, no spin
    ("sim_spin_fallback", {}, ()),                            # a spinning hole
    ("sim_multifreq", {}, ()),                                # three frequencies
    ("sim_multifreq", {"image_num_frequencies": 5}, ()),      # five
    ("sim_dp_interp", {}, ("NO_FUSED_LOCATE",)),              # a locate kernel + bl_shade_fast_kernel
])
@pytest.mark.parametrize("guard_band", [None, 1.0e-2])
@pytest.mark.parametrize("product", [False, True], ids=["mixes", "mixes_x_models_x_units_x_cuts"])
def test_tolerant_one_pass(case, overrides, switches, guard_band, product):
    """The tolerant tier's hot path: one gather per sample whatever the number of mixes, models, units and cuts (launches_shade =
    n_chunks), each variant within the tier's tolerance of the exact tier's fresh render - also where a widened guard band leaves
    samples to the exact second pass, which writes the same mix-free row.
    Worst per-pixel distances measured on one MI355X: sim_dp_interp 5.4e-14, sim_spin_fallback 9.1e-14,
    sim_multifreq 5.3e-14 at three and at five frequencies."""
    fx, params, grid = _case(case, **overrides)
    key = (case, tuple(sorted(overrides.items())))
    mixes, pairs, units, cuts = ([MIXES[0], MIXES[2]], MODELS, UNITS, CUTS) if product else (MIXES, None, None, None)
    got = _render(params, grid, "tolerant", mixes, pairs=pairs, units=units, cuts=cuts, guard_band=guard_band, switches=switches)
    st = got["stats"]
    assert st.arithmetic == 1 and st.launches_shade == st.n_chunks and st.launches_transfer == st.n_chunks
    assert st.fused_variant == (0 if switches else 2) and st.n_mixes == len(mixes)
    if guard_band is not None:
        assert st.n_deferred > 0
    _check_tolerance(got, key, params, grid, mixes, pairs, units, cuts)
    if not product:   # the thermal entry against a context with no list set, in this tier: the same bound
        plain = _fresh(key, params, grid, "tolerant", THERMAL)
        worst, _, _, same_support = gu.per_pixel_relative(got["image_by_mix"][0], plain["image"])
        assert worst < 1.0e-10 and same_support, worst
        assert np.array_equal(np.isnan(got["image_by_mix"][0]), np.isnan(plain["image"]))


def test_a_frame_that_is_no_multiple_of_a_wave():
    """100 rays x 3 frequencies x 4 mixes: every workgroup of the transfer kernel is ragged, its last wave too"""
    fx, params, grid = _case("sim_multifreq", camera_resolution=10)
    got = _render(params, grid, "tolerant", MIXES)
    st = got["stats"]
    assert got["sample_num"].size == 100 and st.arithmetic == 1 and st.launches_shade == st.n_chunks and st.launches_transfer == st.n_chunks
    assert st.fused_variant == 2
    _check_tolerance(got, ("sim_multifreq", (("camera_resolution", 10),)), params, grid, MIXES)


# ---------------------------------------------------------------------------------------------------------------- 6: one mix, no mix
def test_one_mix_is_that_mix():
    fx, params, grid = _case("sim_dp_interp")
    for tier in ("exact", "tolerant"):
        for mix in (MIXES[2], THERMAL):
            got = _render(params, grid, tier, [mix], reproducible=True)
            want = _fresh(("sim_dp_interp", ()), params, grid, tier, mix, reproducible=True)
            assert got["image"].shape == want["image"].shape
            assert gu.same_bits(got["image"], want["image"]).all(), (tier, mix)
            assert np.array_equal(got["sample_num"], want["sample_num"])
            assert got["stats"].launches_shade == want["stats"].launches_shade
            assert got["stats"].arithmetic == want["stats"].arithmetic and got["stats"].fused_variant == want["stats"].fused_variant


def _plan_lines(capfd, monkeypatch, params, grid, tier, clear_list):
    """Two renders in contexts of their own - one that set and cleared a list, one that never had one - with the `kernels:` line of each"""
    import blacklight_amd as bl
    monkeypatch.setenv("BLACKLIGHT_AMD_DEBUG_COUNTERS", "1")   # (read when the context is created)
    out = []
    for touched in (clear_list, False):
        with bl.Context(bl.Params.from_dict(params)) as ctx:
            ctx.set_arithmetic(tier)
            ctx.set_grid(grid)
            if touched:
                ctx.set_electron_mixes(MIXES)
                ctx.set_electron_mixes([])
            capfd.readouterr()
            got = ctx.render()
            lines = [line for line in capfd.readouterr().err.splitlines() if line.startswith("kernels: ")]
            assert len(lines) == 1, lines
            out.append((got, lines[0]))
    return out


@pytest.mark.parametrize("name", ["tolerant", "exact", "tolerant_four_frequencies", "power_law"])
def test_no_list_renders_what_it_rendered(name, capfd, monkeypatch):
    """With no list set: the bits of a second context, and the kernel plan tests/test_gpu_kernel_plan.py reads for the configuration"""
    import test_gpu_kernel_plan as plan
    case, tier, over, mesh, setup, expected = plan.CASES[name]
    assert not mesh and not setup
    fx, params, grid = _case(case, **over)
    (a, line_a), (b, line_b) = _plan_lines(capfd, monkeypatch, params, grid, tier, clear_list=True)
    assert line_a == line_b and plan._stages(line_a[len("kernels: "):]) == plan._stages(expected)
    assert np.array_equal(a["sample_num"], b["sample_num"])
    if a["stats"].composed_maps:   # (composed maps: equal to rounding from run to run, not bit for bit - include/blacklight_amd.h)
        worst, _, _, same_support = gu.per_pixel_relative(a["image"], b["image"])
        assert worst < 1.0e-10 and same_support
    else:
        assert gu.same_bits(a["image"], b["image"]).all()
    assert a["stats"].n_mixes == b["stats"].n_mixes == 1
    assert a["image_by_model"].shape == (1,) + a["image"].shape and a["image_by_cut"].shape == (1, 1, 1) + a["image"].shape


# ---------------------------------------------------------------------------------------------------------------- 7: cameras
def test_cameras_times_mixes():
    fx, params, grid = _case("sim_dp_interp", camera_resolution=16)
    cameras = [(60.0, 0.0), (30.0, 45.0)]
    n_pix = 16 * 16
    # (the last input: a mix without a thermal part beside one with - the tolerant tier renders that list as two runs)
    for tier, reproducible, mixes in (("exact", False, [MIXES[0], MIXES[1]]), ("tolerant", True, [MIXES[0], MIXES[1]]), ("tolerant", True, [OWN, PURE])):
        runs = PURE in mixes
        got = _render(params, grid, tier, mixes, cameras=cameras, reproducible=reproducible)
        assert got["image"].shape[1] == 2 * n_pix and got["stats"].n_cameras == 2 and got["stats"].n_mixes == 2
        assert (1 <= got["stats"].launches_geodesic <= 2) if runs else got["stats"].launches_geodesic == 1
        for c, (th, ph) in enumerate(cameras):
            one = _render(dict(params, camera_th=th, camera_ph=ph), grid, tier, mixes, reproducible=reproducible)
            view = slice(c * n_pix, (c + 1) * n_pix)
            assert np.array_equal(got["sample_num"][view], one["sample_num"])
            if tier == "exact":
                assert gu.same_bits(got["image_by_mix"][:, :, view], one["image_by_mix"]).all(), (tier, c)
            else:   # (the one pass, per-sample records under bl_set_reproducible: a ray's lane does what it does in the one-camera render)
                assert np.array_equal(np.isnan(got["image_by_mix"][:, :, view]), np.isnan(one["image_by_mix"]))
                assert gu.same_bits(got["image_by_mix"][:, :, view], one["image_by_mix"]).all(), (tier, c)
            if runs:   # ... and every mix's slice against a context of one camera with that mix in its block
                key = ("sim_dp_interp", (("camera", c), ("camera_resolution", 16)))
                for e, mix in enumerate(mixes):
                    fresh = _fresh(key, dict(params, camera_th=th, camera_ph=ph), grid, tier, mix, reproducible=reproducible)
                    assert np.array_equal(got["sample_num"][view], fresh["sample_num"])
                    assert gu.same_bits(got["image_by_mix"][e][:, view], fresh["image"]).all(), (tier, c, e)


# ---------------------------------------------------------------------------------------------------------------- 8: a series
def test_series_keeps_geodesics_when_mixes_change():
    import blacklight_amd as bl
    fx, params, grid = _case("sim_dp_interp")
    second = dataclasses.replace(grid, prim=grid.prim * np.float32(1.07))
    first_mixes, second_mixes = MIXES[:2], MIXES[2:4]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(grid)
        ctx.set_electron_mixes(first_mixes)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        ctx.set_grid(second)
        ctx.set_electron_mixes(second_mixes)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        ctx.set_electron_mixes([])   # back to the parameter block's mix, the single image (thermal: other kernels, whose record layout
        c = ctx.render()             # is part of what the resident records depend on - reuse is not asserted here)
        assert c["image"].shape[0] == b["image"].shape[0] // 2
        assert ctx.electron_mixes == [] and ctx.num_electron_mixes == 0
    _check_bits(a, ("sim_dp_interp", ()), params, grid, "exact", first_mixes)
    _check_bits(b, ("sim_dp_interp", "second grid"), params, second, "exact", second_mixes)
    assert gu.same_bits(c["image"], _render(params, second, "exact")["image"]).all()
