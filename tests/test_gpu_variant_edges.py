"""GPU: electron models and density units at the physical edges of the transfer step.

test_gpu_electron_models.py and test_gpu_density_units.py hold variants near the fixture's own unit (1e-16 g/cm^3) and pair at
1e11-4e11 Hz, where every step is optically thin and h nu << k T_e. Here the units span 1e-21 to 1e-12 (BL_MAX_DENSITY_UNITS of
them), R_high reaches 1e4, the frequencies 1e15 Hz, and two grids derived from the fixture's in this module add what the plain one
lacks: cells without a field and cells without pressure (the degenerate grid), and a stronger field at the same plasma (the scaled
grid, where cold electrons still emit at 1e15 Hz). Each case proves from the CPU oracle's per-sample dump (blo_render_dump: k T_e,
j_nu, alpha_nu and delta tau at frequency 0) that it enters the branches of bl_transfer_freq_kernel it claims:

  planck     a sample with j > 0 and h nu / k T_e >= 2^-10 (the Planck factor's expm1 branch)
  moderate   a sample with 2^-10 <= delta tau <= 100 (the expm1(-delta tau) branch)
  thick      a sample with delta tau > 100 (the thick step that replaces the intensity behind it)
  underflow  a ray that mixes samples whose j_nu underflows to 0 with samples of j_nu > 0

and what it asserts, per tier:

  exact      every variant row is the CPU oracle's bits with that unit and pair in the parameter block, and a fresh GPU render's;
             sample_num and sample_flags as the oracle's
  tolerant   (one pass: launches_shade = n_chunks) sample_num, sample_flags and the NaN mask of the exact tier's fresh render,
             and per pixel |I - I_exact| <= max(1e-10 |I_exact|, 2^-1022 nu^3): the tier's relative 1e-10, and at the underflow edge
             one DBL_MIN of the accumulator I / nu^3 (see _within_tier); the same positive support wherever either accumulator
             is normal; two renders of one context are bit-identical
  tolerant   (a pass per variant: image_tau, a density cut) the bits of fresh tolerant renders under bl_set_reproducible"""
import dataclasses
import functools

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

gpu = pytest.mark.gpu   # (the regime proofs need only the CPU oracle)

UNITS = [float(u) for u in np.geomspace(1.0e-21, 1.0e-12, 16)]            # BL_MAX_DENSITY_UNITS; the parameter block keeps 1e-16
PAIRS = [(lo, hi) for hi in (1.0, 10.0, 1.0e3, 1.0e4) for lo in (1.0, 0.1, 5.0)]   # (R_low, R_high)
SEVEN = dict(image_num_frequencies=7, image_frequency_start=1.0e10, image_frequency_end=1.0e15, image_frequency_spacing="log")
DUMP_RAYS = (528, 404, 652, 330, 726)   # near the middle of a 32^2 or 33^2 camera: long rays through the disk
SUBNORMAL = 2.0 ** -1022
FALLBACK = dict(fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)   # (the values the fixtures use)
H_CGS, C_CGS = 6.62607015e-27, 2.99792458e10

# name: (grid, parameter overrides, units, pairs, regimes the case must reach)
CASES = {
    "units_230ghz": ("plain", dict(image_frequency=2.3e11), UNITS, None, {"moderate", "thick"}),
    "units_1e13": ("plain", dict(image_frequency=1.0e13), UNITS, None, {"moderate", "thick", "underflow"}),
    "units_1e15": ("plain", dict(image_frequency=1.0e15), UNITS, None, {"underflow"}),
    "units_7freq": ("plain", SEVEN, UNITS, None, {"moderate", "thick"}),
    "models_230ghz": ("plain", dict(image_frequency=2.3e11), None, PAIRS, {"moderate", "underflow"}),
    "models_1e15": ("scaled", dict(image_frequency=1.0e15), None, PAIRS, {"planck", "underflow"}),
    "lanes_105": ("plain", dict(SEVEN, camera_resolution=33), [1.0e-20, 1.0e-18, 1.0e-16, 1.0e-14, 1.0e-12],
                  [(1.0, 1.0), (1.0, 10.0), (0.1, 1.0e3)], {"moderate", "thick", "underflow"}),
    "lanes_256": ("plain", dict(image_frequency=1.0e13), UNITS,
                  [(lo, float(hi)) for lo, hi in zip((1.0, 0.1, 5.0) * 6, np.geomspace(1.0, 1.0e4, 16))],
                  {"moderate", "thick", "underflow"}),
    "degenerate_units_nan": ("degenerate", dict(fallback_nan="true"), UNITS, None, {"moderate", "thick"}),
    "degenerate_units": ("degenerate", dict(FALLBACK), UNITS, None, {"moderate", "thick"}),
    "degenerate_models_nan": ("degenerate", dict(fallback_nan="true"), None, PAIRS, {"moderate", "underflow"}),
    "degenerate_models": ("degenerate", dict(FALLBACK, image_frequency=1.0e13), None, PAIRS, {"underflow"}),
}
# one pass does not apply: image_tau, a density cut
LOOP_CASES = {
    "units_230ghz_tau": ("plain", dict(image_frequency=2.3e11, image_tau="true"), UNITS, None, {"moderate", "thick"}),
    "degenerate_cut_1e13": ("degenerate", dict(image_frequency=1.0e13, cut_rho_min=3.0e-18), UNITS, [(1.0, 10.0), (0.1, 1.0e3)],
                            {"moderate", "thick"}),
}


@functools.lru_cache(maxsize=None)
def _grid(kind):
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    grid = gu.golden_grid(mock_args)
    if kind == "plain":
        return grid
    prim = grid.prim.copy()
    if kind == "scaled":   # rho and p / 100 at a unit of 1e-10 (_params): the plasma the fixture has at 1e-12, in a field ten times stronger
        prim[0:2] *= np.float32(1.0e-2)
    else:                  # degenerate: no field in the azimuthal quarter [0, pi/2), no pressure in [pi, 3 pi/2)
        for b in range(prim.shape[1]):
            phi = grid.x3v[b]
            prim[5:8, b, (phi >= 0.0) & (phi < 0.5 * np.pi)] = 0.0
            prim[1, b, (phi >= np.pi) & (phi < 1.5 * np.pi)] = 0.0
    return dataclasses.replace(grid, prim=np.ascontiguousarray(prim))


def _params(kind, overrides):
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    params = dict(params, **overrides)
    if kind != "plain":
        params["cut_sigma_max"] = -1.0   # (the sigma cut would hide what these grids change)
    if kind == "scaled":
        params["simulation_rho_cgs"] = 1.0e-10
    return params


def _variants(units, pairs):
    return [(m, u, unit, pair) for m, pair in enumerate(pairs or [None]) for u, unit in enumerate(units or [None])]


def _block(params, unit, pair):
    over = {}
    if unit is not None:
        over["simulation_rho_cgs"] = unit
    if pair is not None:
        over.update(plasma_rat_low=pair[0], plasma_rat_high=pair[1])
    return dict(params, **over)


def _render(params, grid, tier, units=None, pairs=None, reproducible=False, twice=False):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        if pairs is not None:
            ctx.set_electron_models([h for _, h in pairs], rat_low=[lo for lo, _ in pairs])
        if units is not None:
            ctx.set_density_units(units)
        got = ctx.render()
        if twice:
            return got, ctx.render()
        return got


def _oracle(params, grid, dump_ray=-1):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    p = bl.Params.from_dict(params)
    return oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=int(params["camera_resolution"]) ** 2,
                             num_threads=16, dump_ray=dump_ray, max_steps=int(params["ray_max_steps"]),
                             n_freq=int(params["image_num_frequencies"]))


@functools.lru_cache(maxsize=None)
def _fresh_exact(name, unit, pair):
    """The exact tier's fresh render of one variant of a case (shared by the tests of both tiers)"""
    kind, overrides, units, pairs, _ = {**CASES, **LOOP_CASES}[name]
    return _render(_block(_params(kind, overrides), unit, pair), _grid(kind), "exact")


def _regimes(params, grid):
    """Which of the transfer step's branches the oracle's samples of DUMP_RAYS enter at frequency 0"""
    found = set()
    for ray in DUMP_RAYS:
        d = _oracle(params, grid, dump_ray=ray)["dump"]
        kte, j, alpha, dtau = d["kte"], d["j"], d["alpha"], d["dtau"]
        assert len(kte) > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            # alpha = j expm1(h nu / k T_e) c^2 / (2 h) in the fluid frame (simulation_coefficients.cpp:505-510): the branch's x
            x_planck = np.log1p(alpha / j * (2.0 * H_CGS / C_CGS ** 2))
        emitting = j > 0.0
        if np.any(emitting & (alpha > 0.0) & (x_planck >= 2.0 ** -10) & np.isfinite(kte) & (kte > 0.0)):
            found.add("planck")
        if np.any((alpha > 0.0) & (dtau >= 2.0 ** -10) & (dtau <= 100.0)):
            found.add("moderate")
        if np.any(dtau > 100.0):
            found.add("thick")
        if np.any(np.isfinite(kte) & (kte > 0.0) & (j == 0.0)) and np.any(emitting):   # (kte: the sample has coefficients)
            found.add("underflow")
    return found


@pytest.mark.parametrize("name", sorted(CASES) + sorted(LOOP_CASES))
def test_case_reaches_its_regimes(name):
    """A case that never enters a branch is no coverage of it: the oracle's dumped samples, over the case's variants"""
    kind, overrides, units, pairs, want = {**CASES, **LOOP_CASES}[name]
    params, grid = _params(kind, overrides), _grid(kind)
    found = set()
    for _, _, unit, pair in _variants(units, pairs):
        found |= _regimes(_block(params, unit, pair), grid)
        if found >= want:
            break
    assert found >= want, (name, sorted(found))
    if kind == "degenerate":   # the field-free and pressure-free cells do reach the images: NaN and zero pixels the plain grid lacks
        image = _oracle(params, grid)["image"][0]
        plain = _oracle(_params("plain", overrides), _grid("plain"))["image"][0]
        assert np.isnan(image).any() and (image == 0.0).any()
        assert np.isnan(image).sum() + (image == 0.0).sum() > np.isnan(plain).sum() + (plain == 0.0).sum()


@gpu
def test_thick_steps_in_the_exact_tau_image():
    """The thick reset at 230 GHz, from the exact tier itself: a ray whose mean delta tau per sample exceeds kDeltaTauMax"""
    kind, overrides, units, pairs, _ = LOOP_CASES["units_230ghz_tau"]
    params, grid = _params(kind, overrides), _grid(kind)
    got = _render(params, grid, "exact", units, pairs)
    tau = got["image_by_unit"][0, -1, 1]
    assert np.nanmax(tau / np.maximum(got["sample_num"], 1)) > 100.0


@gpu
@pytest.mark.parametrize("name", sorted(CASES) + sorted(LOOP_CASES))
def test_exact_tier_is_the_oracle(name):
    kind, overrides, units, pairs, _ = {**CASES, **LOOP_CASES}[name]
    params, grid = _params(kind, overrides), _grid(kind)
    got = _render(params, grid, "exact", units, pairs)
    n_m, n_u = len(pairs or [None]), len(units or [None])
    n_q = got["image"].shape[0] // (n_m * n_u)
    by_unit = got["image"].reshape(n_m, n_u, n_q, -1)
    for m, u, unit, pair in _variants(units, pairs):
        block = _block(params, unit, pair)
        want = _oracle(block, grid)
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        assert gu.same_bits(by_unit[m, u], want["image"]).all(), (name, m, u, unit, pair)
        fresh = _fresh_exact(name, unit, pair)
        assert gu.same_bits(by_unit[m, u], fresh["image"]).all(), (name, m, u, unit, pair)
        assert np.array_equal(got["sample_num"], fresh["sample_num"]) and np.array_equal(got["sample_flags"], fresh["sample_flags"])


def _within_tier(a, b, frequencies):
    """Tolerant row a against exact row b (n_q = frequencies): the same NaN mask, and per pixel |a - b| <= max(1e-10 |b|, 2^-1022 nu^3):
    the tier's 1e-10 wherever the accumulator I / nu^3 lies well inside the normal range, and one DBL_MIN of the accumulator at and
    below its edge. There each sample whose j_nu went through a subnormal exp(-x^(1/3)) carries that factor's unit 2^-1074 in both
    tiers, scaled by the sample's coefficient and length, so the exact tier is itself no closer (sample_num 2^-1074 nu^3 does not hold:
    differences of up to 5e6 times that were seen at 1e10 Hz). The positive support is the same wherever either accumulator is
    normal. Returns the number of pixels held by the absolute bound alone."""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    nu3 = np.asarray(frequencies, dtype=np.float64)[:, None] ** 3
    finite = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    with np.errstate(invalid="ignore"):
        err = np.abs(a - b)
        tol = np.maximum(1.0e-10 * np.abs(b), SUBNORMAL * nu3)
        edge = np.maximum(np.abs(a), np.abs(b)) / nu3 < SUBNORMAL
    assert np.all(err[finite] <= tol[finite]), float(np.max((err / tol)[finite]))
    assert np.array_equal(((a > 0.0) & finite)[~edge], ((b > 0.0) & finite)[~edge])
    return int((finite & (err > 1.0e-10 * np.abs(b))).sum())


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_tolerant_one_pass(name):
    kind, overrides, units, pairs, _ = CASES[name]
    params, grid = _params(kind, overrides), _grid(kind)
    got, again = _render(params, grid, "tolerant", units, pairs, twice=True)
    st = got["stats"]
    assert st.arithmetic == 1 and st.launches_shade == st.n_chunks and st.launches_transfer == st.n_chunks
    assert gu.same_bits(got["image"], again["image"]).all()   # (two renders of one context)
    n_m, n_u = len(pairs or [None]), len(units or [None])
    n_q = got["image"].shape[0] // (n_m * n_u)
    by_unit = got["image"].reshape(n_m, n_u, n_q, -1)
    frequencies = _oracle(params, grid)["frequencies"][:n_q]
    for m, u, unit, pair in _variants(units, pairs):
        exact = _fresh_exact(name, unit, pair)
        assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
        _within_tier(by_unit[m, u], exact["image"], frequencies)


@gpu
@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_tolerant_loop_equals_fresh_renders(name):
    """Where one pass does not apply: one shading pass per variant, the bits of fresh renders under bl_set_reproducible"""
    kind, overrides, units, pairs, _ = LOOP_CASES[name]
    params, grid = _params(kind, overrides), _grid(kind)
    got = _render(params, grid, "tolerant", units, pairs, reproducible=True)
    n_m, n_u = len(pairs or [None]), len(units or [None])
    one = _render(_block(params, units[0] if units else None, pairs[0] if pairs else None), grid, "tolerant", reproducible=True)
    assert got["stats"].launches_shade == n_m * n_u * one["stats"].launches_shade
    n_q = got["image"].shape[0] // (n_m * n_u)
    by_unit = got["image"].reshape(n_m, n_u, n_q, -1)
    for m, u, unit, pair in _variants(units, pairs):
        want = _render(_block(params, unit, pair), grid, "tolerant", reproducible=True)
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
        assert gu.same_bits(by_unit[m, u], want["image"]).all(), (name, m, u, unit, pair)
