"""GPU: polarized variants with a sigma cut each - (R_low, R_high, simulation_rho_cgs, cut_sigma_max) quadruples - in one render
(bl_set_polarized_variants_sigma, Context.set_polarized_variants(sigma_max=...)).

Every variant's image rows must be the bits of a fresh render with that quadruple in the parameter block, in the exact tier (and so
the reference's golden for the fixture's own quadruple) and in the tolerant tier. Where the triples render in one pass the quadruples
do too: the frame-and-inputs kernel runs with the sigma upper cut off and bl_polarized_coefficients_kernel decides each variant's cut
from the cell's rho and b.b in the sample's row - the quotient sample_finish_simulation() forms of the same operands. A sample that one
variant cuts and another keeps has one shared frame (BlPolSample), which a fresh render takes from bl_polarized_frame_kernel where the
cell is cut and from the coefficient kernel proper where it is not: these tests hold that the two write the same bits. Where the
render takes one shading pass per variant, each pass compares its own variant's cut. The cuts are no part of what the resident
geodesics depend on."""
import ctypes
import functools

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

# (R_low, R_high, unit) as tests/test_gpu_polarized_variants.py has them; the fixtures' own triple is (1, 10, 1e-16)
OFF_FIXTURE = [(1.0, 1.0, 1.0e-17), (1.0, 40.0, 3.0e-17), (2.0, 160.0, 3.0e-16), (0.5, 20.0, 1.0e-15)]
# The fixtures' own cut is 1.0; 0.0 cuts every cell with a field; 1.0000001 lies next to another cut. The CPU oracle's images of
# sim_polarized under 0.01, 0.1, 1.0, 10.0, -1.0 and 0.0 differ pairwise (in 80 to 2880 of the 2880 values; 1.0000001 gives the
# image of 1.0): the sigma of the fixture's cells spans all of these thresholds.
CUTS = [0.01, 0.1, 1.0, 10.0, -1.0, 0.0, 1.0000001]
DISTINCT = [0.01, 0.1, 1.0, 10.0, -1.0, 0.0]
AUX_OFF = dict(image_time=False, image_length=False, image_lambda=False, image_emission=False, image_lambda_ave=False,
               image_emission_ave=False, image_tau_int=False, image_crossings=False)


@functools.lru_cache(maxsize=None)
def _load(name):
    fx, params, mock_args = gu.load_case(name)
    return fx, params, gu.golden_grid(mock_args)


def _case(name, **overrides):
    fx, params, grid = _load(name)
    return fx, dict(params, image_polarization=True, **overrides), grid


def _own(params):
    return (float(params["plasma_rat_low"]), float(params["plasma_rat_high"]), float(params["simulation_rho_cgs"]), float(params["cut_sigma_max"]))


def _quads(params, cuts=CUTS):
    """The cuts over the off-fixture triples, one after another, and the fixture's own quadruple last"""
    return [OFF_FIXTURE[k % len(OFF_FIXTURE)] + (cut,) for k, cut in enumerate(cuts)] + [_own(params)]


def _context(params, grid, tier, reproducible=False, scratch=None, guard_band=None):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_grid(grid)
    ctx.set_arithmetic(tier)
    ctx.set_reproducible(reproducible)
    if scratch is not None:
        ctx.set_scratch_limit(scratch)
    if guard_band is not None:
        ctx.debug_set_guard_band(guard_band)
    return ctx


def _set(ctx, quads):
    ctx.set_polarized_variants([h for _, h, _, _ in quads], [u for _, _, u, _ in quads], rat_low=[lo for lo, _, _, _ in quads],
                               sigma_max=[c for _, _, _, c in quads])


def _render(params, grid, tier, quads=None, **kwargs):
    with _context(params, grid, tier, **kwargs) as ctx:
        if quads is not None:
            _set(ctx, quads)
        return ctx.render()


_FRESH = {}


def _fresh(params, grid, tier, quad, reproducible=True):
    """A fresh render with the quadruple in the parameter block: computed once per (parameters, tier, quadruple), never changed"""
    low, high, unit, cut = quad
    block = dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit, cut_sigma_max=cut)
    key = (tuple(sorted((k, str(v)) for k, v in block.items())), id(grid), tier, reproducible)
    if key not in _FRESH:
        got = _render(block, grid, tier, reproducible=reproducible)
        for name in ("image", "sample_num", "sample_flags"):
            got[name].setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def _check_variants(got, params, grid, tier, quads, reproducible=True):
    n_v = len(quads)
    n_q, n_rays = got["image"].shape[0] // n_v, got["image"].shape[1]
    assert got["image_by_variant"].shape == (n_v, n_q, n_rays)
    for v, quad in enumerate(quads):
        want = _fresh(params, grid, tier, quad, reproducible)
        assert want["image"].shape[0] == n_q
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        differing = int((~gu.same_bits(got["image_by_variant"][v], want["image"])).sum())
        print(f"variant {v} {quad}: {differing} of {want['image'].size} values differ from the fresh render's bits")
        assert differing == 0, f"variant {v} {quad}"
        assert gu.same_bits(got["image"][v * n_q:(v + 1) * n_q], want["image"]).all()


ONE_PASS = ["sim_polarized", "sim_polarized_cks", "sim_polarized_split", "sim_refined"]


@pytest.mark.parametrize("case", ONE_PASS)
def test_exact_tier_equals_fresh_renders_and_the_golden(case):
    fx, params, grid = _case(case)
    quads = _quads(params)
    got = _render(params, grid, "exact", quads)
    st = got["stats"]
    assert st.arithmetic == 0
    assert st.launches_geodesic == st.n_chunks and st.launches_shade == st.n_chunks
    _check_variants(got, params, grid, "exact", quads, reproducible=False)
    if case != "sim_refined":   # (its golden is the unpolarized run's)
        assert gu.same_bits(got["image_by_variant"][-1], gu.expected_image(fx, "B", got["sample_num"].size)).all()


@pytest.mark.parametrize("case", ONE_PASS)
def test_tolerant_tier_reproducible_equals_fresh_renders(case):
    fx, params, grid = _case(case)
    quads = _quads(params)
    got = _render(params, grid, "tolerant", quads, reproducible=True)
    st = got["stats"]
    assert st.arithmetic == 1
    assert st.launches_geodesic == st.n_chunks and st.launches_shade == st.n_chunks
    _check_variants(got, params, grid, "tolerant", quads)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_only_the_cuts_differ(tier):
    """One triple under all seven cuts, in one pass: a cut that is ignored, or decided as another variant's, fails here"""
    fx, params, grid = _case("sim_polarized")
    quads = [_own(params)[:3] + (cut,) for cut in CUTS]   # (the triple the oracle's images above were made with)
    got = _render(params, grid, tier, quads, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks and got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, quads)
    rows = {cut: got["image_by_variant"][v] for v, cut in enumerate(CUTS)}
    for i, a in enumerate(DISTINCT):   # (the thresholds whose images the CPU oracle shows to differ pairwise)
        assert np.isfinite(rows[a]).any()
        for b in DISTINCT[i + 1:]:
            assert not gu.same_bits(rows[a], rows[b]).all(), (a, b)
    assert not np.nansum(np.abs(rows[0.0][:4])) > 0.0   # (every cell with a field is cut: no Stokes intensity)


PASSES = [("sim_polarized_powerlaw", {}), ("sim_polarized_kappa_mix", {}), ("sim_code_kappa", {}), ("sim_polarized", {"cut_theta_e_max": 20.0})]
SHORT = [0.1, -1.0, 10.0]   # (three cuts and the fixture's own: a pass each)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
@pytest.mark.parametrize("case, overrides", PASSES)
def test_passes_compare_their_own_variants_cut(case, overrides, tier):
    """Auxiliary rows, Theta_e from the grid's entropy, a Theta_e cut that the pairs decide differently: one shading pass per variant,
    each with its own BlShadeCold and cut-mask bit"""
    fx, params, grid = _case(case, **overrides)
    quads = _quads(params, SHORT)
    got = _render(params, grid, tier, quads, reproducible=True)
    st = got["stats"]
    assert st.launches_shade == st.n_chunks * len(quads) and st.launches_geodesic == st.n_chunks
    _check_variants(got, params, grid, tier, quads)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
@pytest.mark.parametrize("case, overrides", [
    ("sim_polarized_powerlaw", AUX_OFF),        # power-law electrons, spin 0.9, nearest-cell sampling; the optical-depth row stays
    ("sim_polarized_kappa_mix", AUX_OFF),       # thermal + power-law + kappa electrons, two frequencies, rotation split
    ("sim_blockinterp", {}),                    # inter-block interpolation: a locate kernel in front of bl_shade_kernel
    ("sim_multiblock", {}),
])
def test_one_pass_with_every_electron_population_and_locate_path(case, overrides, tier):
    fx, params, grid = _case(case, **overrides)
    quads = _quads(params, SHORT)
    got = _render(params, grid, tier, quads, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks and got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, quads)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_equal_units_share_one_pass_under_a_density_cut(tier):
    fx, params, grid = _case("sim_polarized", cut_rho_max=3.0e-18)
    quads = [(1.0, 1.0, 1.0e-16, 0.1), (1.0, 40.0, 1.0e-16, 10.0), (2.0, 160.0, 1.0e-16, -1.0), (1.0, 40.0, 1.0e-16, 0.1)]
    got = _render(params, grid, tier, quads, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, quads)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_three_frequencies(tier):
    fx, params, grid = _case("sim_polarized", image_num_frequencies=3, image_frequency_start=8.6e10, image_frequency_end=6.9e11,
                             image_frequency_spacing="log")
    quads = _quads(params, SHORT)
    got = _render(params, grid, tier, quads, reproducible=True)
    assert got["image_by_variant"].shape[1] == 12 + 3   # (Stokes rows of three frequencies, and the fixture's optical-depth rows)
    assert got["stats"].launches_shade == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, quads)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_chunked_render_equals_the_unchunked_bits(tier):
    fx, params, grid = _case("sim_polarized")
    quads = _quads(params, SHORT)
    whole = _render(params, grid, tier, quads, reproducible=True)
    assert whole["stats"].n_chunks == 1
    # (the largest of a descending series of scratch limits that no longer takes the frame in one chunk; a grid of persistent waves
    # reserves ray_max_steps records per lane, so the limits start far above what the frame's samples alone would need)
    for limit in [int((1 << 30) * 0.8 ** k) for k in range(24)]:
        got = _render(params, grid, tier, quads, reproducible=True, scratch=limit)
        print(f"scratch limit {limit >> 20} MiB: {got['stats'].n_chunks} chunks")
        if got["stats"].n_chunks >= 2:
            break
    assert got["stats"].n_chunks >= 2
    assert got["stats"].launches_shade == got["stats"].n_chunks
    assert gu.same_bits(got["image"], whole["image"]).all()
    assert np.array_equal(got["sample_num"], whole["sample_num"]) and np.array_equal(got["sample_flags"], whole["sample_flags"])


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_one_quadruple_is_a_fresh_render(tier):
    fx, params, grid = _case("sim_polarized")
    quad = OFF_FIXTURE[2] + (0.1,)
    got = _render(params, grid, tier, [quad], reproducible=True)
    want = _fresh(params, grid, tier, quad)
    assert gu.same_bits(got["image"], want["image"]).all()
    assert not gu.same_bits(got["image"], _fresh(params, grid, tier, OFF_FIXTURE[2] + (1.0,))["image"]).all()   # (not the block's cut)
    a, b = got["stats"], want["stats"]
    for name in ("n_chunks", "launches_geodesic", "launches_locate", "launches_shade", "launches_transfer", "n_samples", "n_gathers", "arithmetic"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_series_keeps_the_geodesics(tier):
    fx, params, grid = _case("sim_polarized")
    first = [OFF_FIXTURE[0] + (0.1,), OFF_FIXTURE[1] + (10.0,)]
    second = [OFF_FIXTURE[0] + (-1.0,), OFF_FIXTURE[1] + (0.01,)]   # only the cuts change
    with _context(params, grid, tier, reproducible=True) as ctx:
        _set(ctx, first)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        _set(ctx, second)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        low, high, unit = (np.ascontiguousarray([quad[k] for quad in second], dtype=np.float64) for k in range(3))
        assert ctx._lib.bl_set_polarized_variants(ctx._ctx, len(second), *(a.ctypes.data_as(ctypes.c_void_p) for a in (low, high, unit))) == 0
        c = ctx.render()   # (the C entry point bl_set_polarized_variants itself: the triples under the parameter block's cut again)
        assert c["stats"].geodesics_reused == 1
        ctx.set_polarized_variants([], [])
        d = ctx.render()
        assert d["stats"].geodesics_reused == 1
    _check_variants(a, params, grid, tier, first)
    _check_variants(b, params, grid, tier, second)
    _check_variants(c, params, grid, tier, [quad[:3] + (float(params["cut_sigma_max"]),) for quad in second])
    assert gu.same_bits(d["image"], _fresh(params, grid, tier, _own(params))["image"]).all()


def test_tolerant_tier_with_the_guard_band_widened():
    """The polarized frame-and-inputs kernels are the exact tier's in both tiers: the row's rho and b.b are the exact tier's bits, and
    no sample near a threshold is decided otherwise than a fresh tolerant render decides it, whatever the band"""
    fx, params, grid = _case("sim_polarized")
    quads = _quads(params)
    got = _render(params, grid, "tolerant", quads, reproducible=True, guard_band=1.0e-2)
    assert got["stats"].arithmetic == 1 and got["stats"].launches_shade == got["stats"].n_chunks
    _check_variants(got, params, grid, "tolerant", quads)


def _distance(a, b):   # (tests/test_gpu_tolerant.py)
    scale = np.nanmax(np.abs(b), axis=-1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / scale
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def test_tolerant_tier_as_a_context_starts():
    """Without bl_set_reproducible: the polarized tolerant path has no cross-lane reduction, so equal bits are expected; only if two
    fresh frames differ from each other may a variant row differ from the fresh frame, by no more than they do."""
    fx, params, grid = _case("sim_polarized")
    quads = _quads(params, SHORT)
    got = _render(params, grid, "tolerant", quads)
    for v, quad in enumerate(quads):
        low, high, unit, cut = quad
        block = dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit, cut_sigma_max=cut)
        one, two = _render(block, grid, "tolerant"), _render(block, grid, "tolerant")
        spread = _distance(two["image"], one["image"])
        rows = got["image_by_variant"][v]
        print(f"variant {v} {quad}: fresh frames differ by {spread:.3e}, variant row from fresh frame by {_distance(rows, one['image']):.3e}")
        if gu.same_bits(one["image"], two["image"]).all():
            assert gu.same_bits(rows, one["image"]).all(), f"variant {v} {quad}"
        else:
            assert _distance(rows, one["image"]) <= spread
