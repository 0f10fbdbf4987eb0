"""GPU: polarized variants with an electron distribution each - (R_low, R_high, simulation_rho_cgs, cut_sigma_max, mix) tuples - in one
render (bl_set_polarized_variants_electrons, Context.set_polarized_variants(electrons=...)).

Every variant's image rows must be the bits of a fresh render with that tuple - its seven plasma_* values included - in the parameter
block, in the exact tier (and so the reference's golden for the fixture's own tuple) and in the tolerant tier. A mix enters no decision
of a render - sample counts, flags, cells and cuts do not depend on it - except that Theta_e exists only where the thermal fraction is
non-zero: where the triples render in one pass the tuples do too, every wave of bl_polarized_coefficients_kernel reading its variant's
electron constants from a device table; with a Theta_e cut and mixes that differ, and wherever the triples take a pass per variant,
each pass binds its own variant's mix. The mixes are no part of what the resident geodesics depend on.

The CPU oracle's images of the seven mixes below differ pairwise in every value, on sim_polarized_kappa (16^2, all 1280 values) and on
sim_polarized (24^2, all 2880): a mix that is ignored, or taken from another variant, cannot pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

# (R_low, R_high, unit) as tests/test_gpu_polarized_variants.py has them; the fixtures' own triple is (1, 10, 1e-16)
OFF_FIXTURE = [(1.0, 1.0, 1.0e-17), (1.0, 40.0, 3.0e-17), (2.0, 160.0, 3.0e-16), (0.5, 20.0, 1.0e-15)]
DISTINCT = [0.01, 0.1, 1.0, 10.0, -1.0, 0.0]   # (tests/test_gpu_polarized_cuts.py)
# A missing key is the parameter block's value: the shape values of a distribution whose fraction is zero are not read
MIXES = {
    "kappa_own": dict(power_frac=0.0, kappa_frac=0.4, kappa=4.0, w=1.5),
    "thermal": dict(power_frac=0.0, kappa_frac=0.0),
    "power": dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0),
    "mix": dict(power_frac=0.2, p=3.0, gamma_min=3.0, gamma_max=500.0, kappa_frac=0.25, kappa=4.3, w=2.5),
    "kappa_low": dict(power_frac=0.0, kappa_frac=0.49, kappa=3.5, w=1.919106339654944),
    "all_power": dict(power_frac=1.0, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0),
    "all_kappa": dict(power_frac=0.0, kappa_frac=1.0, kappa=4.5, w=1.0),
}
NAMES = list(MIXES)
STATS = ("n_chunks", "launches_geodesic", "launches_locate", "launches_shade", "launches_transfer", "n_samples", "n_gathers", "arithmetic")


@functools.lru_cache(maxsize=None)
def _load(name):
    fx, params, mock_args = gu.load_case(name)
    return fx, params, gu.golden_grid(mock_args)


def _case(name, **overrides):
    fx, params, grid = _load(name)
    return fx, dict(params, image_polarization=True, **overrides), grid


def _own(params):
    """The fixture's own tuple: its mix is the parameter block's (None)"""
    return (float(params["plasma_rat_low"]), float(params["plasma_rat_high"]), float(params["simulation_rho_cgs"]), float(params["cut_sigma_max"]), None)


def _tuples(params, names=NAMES, cuts=None):
    """The mixes over the off-fixture triples in turn (under the fixture's cut, or `cuts` in turn), and the fixture's own tuple last"""
    own_cut = float(params["cut_sigma_max"])
    return [OFF_FIXTURE[k % len(OFF_FIXTURE)] + (cuts[k % len(cuts)] if cuts else own_cut, name) for k, name in enumerate(names)] + [_own(params)]


def _context(params, grid, tier, reproducible=False, scratch=None):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_grid(grid)
    ctx.set_arithmetic(tier)
    ctx.set_reproducible(reproducible)
    if scratch is not None:
        ctx.set_scratch_limit(scratch)
    return ctx


def _set(ctx, tuples):
    ctx.set_polarized_variants([t[1] for t in tuples], [t[2] for t in tuples], rat_low=[t[0] for t in tuples], sigma_max=[t[3] for t in tuples],
                               electrons=[MIXES[t[4]] if t[4] is not None else {} for t in tuples])


def _render(params, grid, tier, tuples=None, **kwargs):
    with _context(params, grid, tier, **kwargs) as ctx:
        if tuples is not None:
            _set(ctx, tuples)
        return ctx.render()


def _block(params, tup):
    low, high, unit, cut, name = tup
    mix = {"plasma_" + key: value for key, value in (MIXES[name] if name is not None else {}).items()}
    return dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit, cut_sigma_max=cut, **mix)


_FRESH = {}


def _fresh(params, grid, tier, tup, reproducible=True):
    """A fresh render with the tuple in the parameter block: computed once per (parameters, tier, tuple), never changed"""
    block = _block(params, tup)
    key = (tuple(sorted((k, str(v)) for k, v in block.items())), id(grid), tier, reproducible)
    if key not in _FRESH:
        got = _render(block, grid, tier, reproducible=reproducible)
        for name in ("image", "sample_num", "sample_flags"):
            got[name].setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def _check_variants(got, params, grid, tier, tuples, reproducible=True):
    n_v = len(tuples)
    n_q, n_rays = got["image"].shape[0] // n_v, got["image"].shape[1]
    assert got["image_by_variant"].shape == (n_v, n_q, n_rays)
    for v, tup in enumerate(tuples):
        want = _fresh(params, grid, tier, tup, reproducible)
        assert want["image"].shape[0] == n_q
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        differing = int((~gu.same_bits(got["image_by_variant"][v], want["image"])).sum())
        print(f"variant {v} {tup}: {differing} of {want['image'].size} values differ from the fresh render's bits")
        assert differing == 0, f"variant {v} {tup}"
        assert gu.same_bits(got["image"][v * n_q:(v + 1) * n_q], want["image"]).all()


def _one_pass(st):
    return st.launches_geodesic == st.n_chunks and st.launches_shade == st.n_chunks


@pytest.mark.parametrize("case", ["sim_polarized_kappa", "sim_polarized"])
def test_one_pass_exact_tier_equals_fresh_renders_and_the_golden(case):
    """... and, over sim_polarized, its `thermal` variant at the own triple: the all-electrons kernel with zero fractions gives the
    thermal kernel's bits, which are the reference's"""
    fx, params, grid = _case(case)
    tuples = _tuples(params)
    if case == "sim_polarized":
        tuples.insert(3, _own(params)[:4] + ("thermal",))
    got = _render(params, grid, "exact", tuples)
    st = got["stats"]
    assert st.arithmetic == 0 and _one_pass(st)
    _check_variants(got, params, grid, "exact", tuples, reproducible=False)
    golden = gu.expected_image(fx, "B", got["sample_num"].size)
    assert gu.same_bits(got["image_by_variant"][-1], golden).all()
    if case == "sim_polarized":
        assert gu.same_bits(got["image_by_variant"][3], golden).all()


@pytest.mark.parametrize("case", ["sim_polarized_kappa", "sim_polarized"])
def test_one_pass_tolerant_tier_reproducible_equals_fresh_renders(case):
    fx, params, grid = _case(case)
    tuples = _tuples(params)
    got = _render(params, grid, "tolerant", tuples, reproducible=True)
    st = got["stats"]
    assert st.arithmetic == 1 and _one_pass(st)
    _check_variants(got, params, grid, "tolerant", tuples)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_only_the_mixes_differ(tier):
    """One triple and cut under the seven mixes, in one pass: a mix that is ignored, or read as another variant's, fails here"""
    fx, params, grid = _case("sim_polarized_kappa")
    tuples = [_own(params)[:4] + (name,) for name in NAMES]
    fresh = [_fresh(params, grid, tier, tup)["image"] for tup in tuples]
    for i in range(len(NAMES)):   # the precondition, which holds for the reference: no two mixes render the same image
        assert np.isfinite(fresh[i]).any()
        for j in range(i + 1, len(NAMES)):
            assert not gu.same_bits(fresh[i], fresh[j]).all(), (NAMES[i], NAMES[j])
    got = _render(params, grid, tier, tuples, reproducible=True)
    assert _one_pass(got["stats"])
    _check_variants(got, params, grid, tier, tuples)


PASS_MIXES = ["thermal", "power", "kappa_own"]


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_passes_bind_their_own_variants_mix(tier):
    """sim_polarized_kappa_mix: image_emission makes it an auxiliary run (two frequencies, rotation split, a = 0.9) - one shading pass per
    variant, each with its own electron constants and BlShadeCold"""
    fx, params, grid = _case("sim_polarized_kappa_mix")
    tuples = [_own(params)] + [OFF_FIXTURE[k] + (float(params["cut_sigma_max"]), name) for k, name in enumerate(PASS_MIXES)]
    got = _render(params, grid, tier, tuples, reproducible=True)
    st = got["stats"]
    assert st.launches_shade == st.n_chunks * len(tuples) and st.launches_geodesic == st.n_chunks
    _check_variants(got, params, grid, tier, tuples)
    if tier == "exact":
        assert gu.same_bits(got["image_by_variant"][0], gu.expected_image(fx, "B", got["sample_num"].size)).all()


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_a_theta_e_cut_with_mixes_that_differ_plans_passes(tier):
    """Theta_e exists only where the thermal fraction is non-zero (all_power and all_kappa have none, and no cell of theirs is cut): the
    one decision a mix enters. Equal triples, so that without the mixes this would be one pass."""
    fx, params, grid = _case("sim_polarized_kappa", cut_theta_e_max=20.0)
    tuples = [_own(params)[:4] + (name,) for name in ("kappa_own", "all_power", "thermal", "all_kappa")]
    got = _render(params, grid, tier, tuples, reproducible=True)
    st = got["stats"]
    assert st.launches_shade == st.n_chunks * len(tuples) and st.launches_geodesic == st.n_chunks
    _check_variants(got, params, grid, tier, tuples)
    same = [_own(params)[:3] + (cut, "mix") for cut in (0.1, 10.0)]   # ... and with equal mixes it is one pass again
    got = _render(params, grid, tier, same, reproducible=True)
    assert _one_pass(got["stats"])
    _check_variants(got, params, grid, tier, same)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_every_member_of_the_tuple_differs(tier):
    fx, params, grid = _case("sim_polarized_kappa")
    tuples = _tuples(params, cuts=DISTINCT)
    got = _render(params, grid, tier, tuples, reproducible=True)
    assert _one_pass(got["stats"])
    _check_variants(got, params, grid, tier, tuples)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_one_tuple_is_a_fresh_render(tier):
    fx, params, grid = _case("sim_polarized_kappa")
    for name in ("mix", "thermal"):   # (non-thermal in a kappa block, and thermal in it: each plans as the block with that mix does)
        tup = OFF_FIXTURE[2] + (0.1, name)
        got = _render(params, grid, tier, [tup], reproducible=True)
        want = _fresh(params, grid, tier, tup)
        assert gu.same_bits(got["image"], want["image"]).all()
        assert not gu.same_bits(got["image"], _fresh(params, grid, tier, OFF_FIXTURE[2] + (0.1, None))["image"]).all()   # (not the block's mix)
        for stat in STATS:
            assert getattr(got["stats"], stat) == getattr(want["stats"], stat), (name, stat)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
@pytest.mark.parametrize("n", [3, 16])
def test_three_and_sixteen_variants(n, tier):
    fx, params, grid = _case("sim_polarized_kappa")
    tuples = [OFF_FIXTURE[k % 4] + (DISTINCT[k % 6], NAMES[k % 7]) for k in range(n)]
    got = _render(params, grid, tier, tuples, reproducible=True)
    assert _one_pass(got["stats"])
    _check_variants(got, params, grid, tier, tuples)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_chunked_render_equals_the_unchunked_bits(tier):
    fx, params, grid = _case("sim_polarized")
    tuples = _tuples(params, ["power", "kappa_low", "thermal"])
    whole = _render(params, grid, tier, tuples, reproducible=True)
    assert whole["stats"].n_chunks == 1
    # (the series of scratch limits tests/test_gpu_polarized_cuts.py walks down for this fixture: the first that takes two chunks)
    for limit in [int((1 << 30) * 0.8 ** k) for k in range(24)]:
        got = _render(params, grid, tier, tuples, reproducible=True, scratch=limit)
        if got["stats"].n_chunks >= 2:
            break
    assert got["stats"].n_chunks >= 2
    assert got["stats"].launches_shade == got["stats"].n_chunks
    assert gu.same_bits(got["image"], whole["image"]).all()
    assert np.array_equal(got["sample_num"], whole["sample_num"]) and np.array_equal(got["sample_flags"], whole["sample_flags"])
    _check_variants(whole, params, grid, tier, tuples)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_series_keeps_the_geodesics(tier):
    fx, params, grid = _case("sim_polarized_kappa")
    triple = OFF_FIXTURE[1] + (float(params["cut_sigma_max"]),)
    first = [triple + ("power",), triple + ("kappa_low",)]
    second = [triple + ("all_kappa",), triple + ("thermal",)]   # only the mixes change
    third = [triple + (name,) for name in ("mix", "kappa_own", "all_power", "thermal", "power")]   # ... and more of them than before
    with _context(params, grid, tier, reproducible=True) as ctx:
        _set(ctx, first)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        _set(ctx, second)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        _set(ctx, third)
        c = ctx.render()
        assert c["stats"].geodesics_reused == 1 and c["stats"].launches_geodesic == 0
        # the C entry point of the quadruples behind it: the mixes are gone, the parameter block's render again
        low, high, unit, cut = (np.ascontiguousarray([t[k] for t in second], dtype=np.float64) for k in range(4))
        assert ctx._lib.bl_set_polarized_variants_sigma(ctx._ctx, len(second), *(x.ctypes.data_as(ctypes.c_void_p) for x in (low, high, unit, cut))) == 0
        d = ctx.render()
        assert d["stats"].geodesics_reused == 1
    _check_variants(a, params, grid, tier, first)
    _check_variants(b, params, grid, tier, second)
    _check_variants(c, params, grid, tier, third)
    _check_variants(d, params, grid, tier, [triple + (None,)] * 2)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_two_cameras_times_three_mixes(tier):
    fx, params, grid = _case("sim_polarized_kappa")
    angles = [(60.0, 0.0), (35.0, 80.0)]
    tuples = _tuples(params, ["power", "mix"])   # (with the fixture's own: three)
    with _context(params, grid, tier, reproducible=True) as ctx:
        ctx.set_cameras([th for th, _ in angles], [ph for _, ph in angles])
        _set(ctx, tuples)
        got = ctx.render()
        slices = [ctx.camera_slice(c) for c in range(2)]
    assert _one_pass(got["stats"])
    for c, (th, ph) in enumerate(angles):
        for v, tup in enumerate(tuples):
            with _context(_block(params, tup), grid, tier, reproducible=True) as ctx:
                ctx.set_cameras([th], [ph])
                want = ctx.render()
            assert np.array_equal(got["sample_num"][slices[c]], want["sample_num"]) and np.array_equal(got["sample_flags"][slices[c]], want["sample_flags"])
            assert gu.same_bits(got["image_by_variant"][v][:, slices[c]], want["image"]).all(), (c, tup)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_all_thermal_mixes_are_the_quadruples(tier):
    """... bit for bit, and planned as they are: the thermal-only kernel, no table of mixes"""
    fx, params, grid = _case("sim_polarized")
    tuples = [OFF_FIXTURE[k] + (DISTINCT[k], "thermal") for k in range(4)]
    got = _render(params, grid, tier, tuples, reproducible=True)
    with _context(params, grid, tier, reproducible=True) as ctx:
        ctx.set_polarized_variants([t[1] for t in tuples], [t[2] for t in tuples], rat_low=[t[0] for t in tuples], sigma_max=[t[3] for t in tuples])
        want = ctx.render()
    assert gu.same_bits(got["image"], want["image"]).all()
    assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
    for stat in STATS:
        assert getattr(got["stats"], stat) == getattr(want["stats"], stat), stat
