"""GPU: several (R_low, R_high, simulation_rho_cgs) triples of a polarized run in one render (bl_set_polarized_variants), and the
polarized flux fit built on them.

Every variant's image rows must be what a fresh render with that triple in the parameter block gives - the same bits, in the exact
tier (and so the reference's golden for the fixture's own triple) and in the tolerant tier: a variant's scalars are formed by the
same device functions on the same operands as a fresh render's, and a transfer lane does for its (ray, variant) what it does for a
ray. The gather, the fluid frame, the geodesics and the transport matrices are shared: one integration and one coefficient-kernel
launch per chunk, and changing the variants between renders keeps the resident records."""
import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

# (R_low, R_high, unit): R_high 1 ... 160, two decades of unit; the fixtures' own triple is (1, 10, 1e-16) and comes last
OFF_FIXTURE = [(1.0, 1.0, 1.0e-17), (1.0, 40.0, 3.0e-17), (2.0, 160.0, 3.0e-16), (0.5, 20.0, 1.0e-15)]
CASES = ["sim_polarized", "sim_polarized_cks", "sim_polarized_powerlaw", "sim_polarized_kappa_mix", "sim_polarized_split", "sim_refined"]
# (auxiliary rows beside the Stokes and optical-depth rows - image_emission, image_time, ... - are written by a kernel that knows one
# variant: these fixtures take one shading pass per variant over the shared samples, the others one pass)
PASSES = ["sim_polarized_powerlaw", "sim_polarized_kappa_mix"]


def _expected_shade_launches(case, stats, n_variants):
    return stats.n_chunks * (n_variants if case in PASSES else 1)


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return fx, dict(params, image_polarization=True, **overrides), gu.golden_grid(mock_args)


def _triples(params):
    return OFF_FIXTURE + [(float(params["plasma_rat_low"]), float(params["plasma_rat_high"]), float(params["simulation_rho_cgs"]))]


def _context(params, grid, tier, reproducible=False, scratch=None):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_grid(grid)
    ctx.set_arithmetic(tier)
    ctx.set_reproducible(reproducible)
    if scratch is not None:
        ctx.set_scratch_limit(scratch)
    return ctx


def _set(ctx, triples):
    ctx.set_polarized_variants([h for _, h, _ in triples], [u for _, _, u in triples], rat_low=[lo for lo, _, _ in triples])


def _render(params, grid, tier, triples=None, **kwargs):
    with _context(params, grid, tier, **kwargs) as ctx:
        if triples is not None:
            _set(ctx, triples)
        return ctx.render()


def _fresh(params, grid, tier, triple, **kwargs):
    low, high, unit = triple
    return _render(dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit), grid, tier, **kwargs)


def _check_variants(got, params, grid, tier, triples, **kwargs):
    n_v = len(triples)
    n_q, n_rays = got["image"].shape[0] // n_v, got["image"].shape[1]
    assert got["image_by_variant"].shape == (n_v, n_q, n_rays)
    singles = []
    for v, triple in enumerate(triples):
        want = _fresh(params, grid, tier, triple, **kwargs)
        assert want["image"].shape[0] == n_q
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        assert gu.same_bits(got["image_by_variant"][v], want["image"]).all(), f"variant {v} {triple}"
        assert gu.same_bits(got["image"][v * n_q:(v + 1) * n_q], want["image"]).all()
        singles.append(want)
    assert np.isfinite(singles[-1]["image"]).any() and not gu.same_bits(singles[0]["image"], singles[-1]["image"]).all()   # (the variants do differ)
    return singles


@pytest.mark.parametrize("case", CASES)
def test_exact_tier_equals_fresh_renders_and_the_golden(case):
    fx, params, grid = _case(case)
    triples = _triples(params)
    got = _render(params, grid, "exact", triples)
    assert got["stats"].arithmetic == 0
    assert got["stats"].launches_shade == _expected_shade_launches(case, got["stats"], len(triples))
    assert got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, "exact", triples)
    if case != "sim_refined":   # (its golden is the unpolarized run's)
        assert gu.same_bits(got["image_by_variant"][-1], gu.expected_image(fx, "B", got["sample_num"].size)).all()


@pytest.mark.parametrize("case", CASES)
def test_tolerant_tier_reproducible_equals_fresh_renders(case):
    fx, params, grid = _case(case)
    triples = _triples(params)
    got = _render(params, grid, "tolerant", triples, reproducible=True)
    assert got["stats"].arithmetic == 1
    assert got["stats"].launches_shade == _expected_shade_launches(case, got["stats"], len(triples))
    assert got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, "tolerant", triples, reproducible=True)


AUX_OFF = dict(image_time=False, image_length=False, image_lambda=False, image_emission=False, image_lambda_ave=False,
               image_emission_ave=False, image_tau_int=False, image_crossings=False)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
@pytest.mark.parametrize("case, overrides", [
    ("sim_polarized_powerlaw", AUX_OFF),        # power-law electrons, spin 0.9, nearest-cell sampling; the optical-depth row stays
    ("sim_polarized_kappa_mix", AUX_OFF),       # thermal + power-law + kappa electrons, two frequencies, rotation split
    ("sim_blockinterp", {}),                    # inter-block interpolation: a locate kernel in front of bl_shade_kernel
    ("sim_multiblock", {}),
])
def test_one_pass_with_every_electron_population_and_locate_path(case, overrides, tier):
    """The fixtures above without their auxiliary rows: the one pass through the coefficient kernel's instantiation that knows
    power-law and kappa electrons, and behind a locate kernel."""
    fx, params, grid = _case(case, **overrides)
    triples = _triples(params)
    got = _render(params, grid, tier, triples, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks and got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, triples, reproducible=True)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_code_kappa_takes_passes(tier):
    """plasma_model = code_kappa: Theta_e comes from the grid's electron entropy, the units still enter n_e and B - one pass per variant"""
    fx, params, grid = _case("sim_code_kappa")
    triples = _triples(params)
    got = _render(params, grid, tier, triples, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks * len(triples)
    n_q = got["image"].shape[0] // len(triples)
    for v, triple in enumerate(triples):
        want = _fresh(params, grid, tier, triple, reproducible=True)
        assert gu.same_bits(got["image"][v * n_q:(v + 1) * n_q], want["image"]).all(), f"variant {v} {triple}"
    # (the pairs are unused: two variants that differ in their pair only are the same image)
    same = _render(params, grid, tier, [(1.0, 10.0, 1.0e-16), (3.0, 90.0, 1.0e-16)], reproducible=True)
    assert gu.same_bits(same["image"][:n_q], same["image"][n_q:]).all() and np.isfinite(same["image"]).any()


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_three_frequencies(tier):
    fx, params, grid = _case("sim_polarized", image_num_frequencies=3, image_frequency_start=8.6e10, image_frequency_end=6.9e11,
                             image_frequency_spacing="log")
    triples = _triples(params)
    got = _render(params, grid, tier, triples, reproducible=True)
    assert got["image_by_variant"].shape[1] == 12 + 3   # (Stokes rows of three frequencies, and the fixture's optical-depth rows)
    _check_variants(got, params, grid, tier, triples, reproducible=True)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_chunked_render_equals_the_unchunked_bits(tier):
    fx, params, grid = _case("sim_polarized")
    triples = _triples(params)
    whole = _render(params, grid, tier, triples, reproducible=True)
    assert whole["stats"].n_chunks == 1
    # (the largest of a descending series of scratch limits that no longer takes the frame in one chunk; a grid of persistent waves
    # reserves ray_max_steps records per lane, so the limits start far above what the frame's samples alone would need)
    for limit in [int((1 << 30) * 0.8 ** k) for k in range(24)]:
        got = _render(params, grid, tier, triples, reproducible=True, scratch=limit)
        print(f"scratch limit {limit >> 20} MiB: {got['stats'].n_chunks} chunks")
        if got["stats"].n_chunks >= 2:
            break
    assert got["stats"].n_chunks >= 2
    assert got["stats"].launches_shade == got["stats"].n_chunks
    assert gu.same_bits(got["image"], whole["image"]).all()
    assert np.array_equal(got["sample_num"], whole["sample_num"]) and np.array_equal(got["sample_flags"], whole["sample_flags"])


def test_one_pass_launch_counts():
    fx, params, grid = _case("sim_polarized")
    triples = _triples(params)
    single = _render(params, grid, "exact")
    got = _render(params, grid, "exact", triples)
    assert got["stats"].launches_geodesic == single["stats"].launches_geodesic == single["stats"].n_chunks
    assert got["stats"].launches_shade == got["stats"].n_chunks
    assert got["stats"].n_samples == single["stats"].n_samples


@pytest.mark.parametrize("cut", [{"cut_rho_max": 3.0e-18}, {"cut_theta_e_max": 20.0}])
@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_a_cut_that_variants_decide_differently_takes_passes(cut, tier):
    fx, params, grid = _case("sim_polarized", **cut)
    triples = _triples(params)
    got = _render(params, grid, tier, triples, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks * len(triples)
    assert got["stats"].launches_geodesic == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, triples, reproducible=True)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_equal_units_share_one_pass_under_a_density_cut(tier):
    fx, params, grid = _case("sim_polarized", cut_rho_max=3.0e-18)
    triples = [(1.0, 1.0, 1.0e-16), (1.0, 40.0, 1.0e-16), (2.0, 160.0, 1.0e-16)]
    got = _render(params, grid, tier, triples, reproducible=True)
    assert got["stats"].launches_shade == got["stats"].n_chunks
    _check_variants(got, params, grid, tier, triples, reproducible=True)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_one_variant_is_a_fresh_render(tier):
    fx, params, grid = _case("sim_polarized")
    triple = OFF_FIXTURE[2]
    got = _render(params, grid, tier, [triple], reproducible=True)
    want = _fresh(params, grid, tier, triple, reproducible=True)
    assert gu.same_bits(got["image"], want["image"]).all()
    a, b = got["stats"], want["stats"]
    for name in ("n_chunks", "launches_geodesic", "launches_locate", "launches_shade", "launches_transfer", "n_samples", "n_gathers", "arithmetic"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_series_keeps_the_geodesics(tier):
    fx, params, grid = _case("sim_polarized")
    first, second = _triples(params)[:2], _triples(params)[1:]
    with _context(params, grid, tier, reproducible=True) as ctx:
        _set(ctx, first)
        a = ctx.render()
        assert a["stats"].geodesics_reused == 0
        _set(ctx, second)
        b = ctx.render()
        assert b["stats"].geodesics_reused == 1 and b["stats"].launches_geodesic == 0
        ctx.set_polarized_variants([], [])
        c = ctx.render()
        assert c["stats"].geodesics_reused == 1
    _check_variants(a, params, grid, tier, first, reproducible=True)
    _check_variants(b, params, grid, tier, second, reproducible=True)
    assert gu.same_bits(c["image"], _render(params, grid, tier, reproducible=True)["image"]).all()


def test_polarized_fit_reaches_its_target():
    from blacklight_amd import flux
    fx, params, grid = _case("sim_polarized", camera_resolution=32)
    pairs = [(10.0, 1.0), (80.0, 1.0)]
    lo, hi, distance = 1.0e-17, 1.0e-15, 8.1e3
    with _context(params, grid, "exact") as ctx:
        _set(ctx, [(l, h, u) for h, l in pairs for u in (lo, hi)])
        ends = [flux.stokes_flux_jy(rows, ctx.params, distance)[0] for rows in ctx.render()["image_by_variant"]]
        ctx.set_polarized_variants([], [])
        # a target inside both pairs' brackets (the fluxes rise with the unit)
        low_end, high_end = max(ends[0], ends[2]), min(ends[1], ends[3])
        assert 0.0 < low_end < high_end
        target = float(np.sqrt(low_end * high_end))
        found, renders = ctx.fit_density_units_polarized(pairs, target, distance, lo, hi, rtol=1.0e-3)
        assert ctx.num_polarized_variants == 0 and 2 <= renders <= 40
        p = ctx.params
    for (high, low), (rho, flux_jy, m_net, v_net) in zip(pairs, found):
        assert lo <= rho <= hi and abs(flux_jy - target) <= 1.0e-3 * target
        fresh = _fresh(params, grid, "exact", (low, high, rho))
        stokes = flux.stokes_flux_jy(fresh["image"], p, distance)
        assert stokes[0] == flux_jy
        assert flux.net_polarization(stokes)[:2] == (m_net, v_net)
        assert 0.0 <= m_net <= 1.0 and abs(v_net) <= 1.0


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
    triples = _triples(params)
    got = _render(params, grid, "tolerant", triples)
    n_q = got["image"].shape[0] // len(triples)
    for v, triple in enumerate(triples):
        one, two = _fresh(params, grid, "tolerant", triple), _fresh(params, grid, "tolerant", triple)
        spread = _distance(two["image"], one["image"])
        rows = got["image_by_variant"][v]
        print(f"variant {v} {triple}: fresh frames differ by {spread:.3e}, variant row from fresh frame by {_distance(rows, one['image']):.3e}")
        if gu.same_bits(one["image"], two["image"]).all():
            assert gu.same_bits(rows, one["image"]).all(), f"variant {v} {triple}"
        else:
            assert _distance(rows, one["image"]) <= spread
    exact = _render(params, grid, "exact")
    assert _distance(got["image_by_variant"][-1], exact["image"]) < 1e-9
