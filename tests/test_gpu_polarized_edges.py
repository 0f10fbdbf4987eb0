"""GPU: polarized renders at the edges of the coupling step (couple_sample, bl_polarized.hip), in both tiers.

test_gpu_parity.py, test_gpu_polarized_variants.py, _cuts.py and _electrons.py render the sim_polarized* fixtures and draws around
them: a unit of 1e-16 g/cm^3 at 86-690 GHz, where every sample has coefficients, is optically thin and takes the joint solution.
Here the fixture sim_polarized (its own 24^2 camera) is rendered with units from 1e-20 to 1e-10, frequencies from 1e10 to 1e15 Hz,
R_high up to 1e4, the other fixtures' electrons, the rotation split, flat rays, and on the degenerate grid of
test_gpu_variant_edges.py (no field in one azimuthal quarter, no pressure in another). Each case proves from the CPU oracle's
per-sample dump (blo_render_dump_polarized: k T_e, j_I, alpha_I, delta tau, j_Q, j_V, alpha_Q, alpha_V, rho_Q, rho_V and
delta lambda at frequency 0, of the rays DUMP_RAYS) that it enters the branches it claims. With rho_p = hypot(rho_Q, rho_V):

  none                no coefficients (k T_e NaN): all eight values zero
  thin                alpha_I > 0, rho_p > 0, delta tau <= 100 (the joint solution with its exponentials)
  thick               alpha_I > 0, rho_p > 0, delta tau > 100 (the joint solution's limit)
  rotate_only         coefficients, alpha_I == 0, rho_p > 0 (rotate + j dl)
  alpha_zeroed        rotate_only with j_I > 0 and alpha_Q == alpha_V == 0 (the "1 / alpha^2 overflows" rule, bl_coefficients.inc)
  emission_underflow  coefficients, j_I == 0, on a ray that also has j_I > 0
  cold                Theta_e = k T_e / m_e c^2 < 0.01, rho_Q == 0, rho_V != 0 (factor_q = 0, factor_v = 1)
  cold_absorbing      cold with alpha_I > 0
  faraday_thick       rho_p delta lambda > 1e3: sin / cos arguments that need the real range reduction
  theta_e_edge        Theta_e == 0.01 to the bit, beside colder and hotter samples: the last sample that takes the Bessel functions
  split_*             the first seven under image_rotation_split (absorb / rotate / absorb). The step's branch is chosen by the whole
                      delta tau (> 100), and absorb is handed delta tau / 2: split_thick asks for delta tau > 200, where each half is
                      thick by itself, split_thin for delta tau <= 100

Regimes that no parameter setting reaches, and so no case claims:

  rho_p == 0 beside alpha_I > 0 (couple_sample's `rho_p == 0` arm of absorb with alpha_p != 0), and alpha_p == 0 beside alpha_I > 0
  (absorb's `alpha_p == 0` arms): rho_p and alpha_p are square roots of sums of two squares, which vanish only when both coefficients
  lie below 2^-537 ~ 1e-162, while alpha_I > 0 survives the "1 / alpha^2 overflows" rule only above ~1e-154; the coefficients of one
  sample are the same n_e, B and Theta_e times factors of order 1e-3 ... 1e3 (rho_V / alpha_I grows with 1 / nu^2, but with it
  delta tau does not shrink), so no sample has one of them eight orders below the other. Samples in a field-free cell have no
  coefficients at all (`none`), in both grids.

What is asserted, per case:

  CPU only   test_case_reaches_its_regimes (above); test_reference_spread_keeps_half_the_rows_well_conditioned
  exact      every row is the bits of the oracle's blmath build; sample_num and sample_flags are the oracle's; the render went through
             bl_shade_polarized2_kernel (fused_variant 4) or, with flat rays, through the locate kernel
  exact      three edge settings as set_polarized_variants triples in one render: each variant's rows are its fresh render's bits
  tolerant   stats.arithmetic == 1; sample_num, sample_flags and the NaN mask are the exact tier's; two renders of one context are
             bit-identical; per row, with d_AB = distance(oracle libm build, oracle blmath build) (the row-maximum distance of
             test_gpu_tolerant.py): distance(tolerant, exact) < 1e-9 where d_AB < 1e-10 (well conditioned: the project's polarized
             bound), and <= max(1e-9, 100 d_AB) elsewhere - the two reference builds differ in the last place of about fifteen
             elementary functions, the tolerant tier also reassociates the transport products, and the coupling amplifies both alike;
             two decimal orders over the reference's own spread, not tuned to the kernel (DESIGN.md holds the measured table)."""
import functools

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import frequency_util as fu
import golden_util as gu
from test_gpu_tolerant import _distance
from test_gpu_variant_edges import _grid

gpu = pytest.mark.gpu   # (the regime proofs and the reference's spread need only the CPU oracle)

FIXTURE = "sim_polarized"
DUMP_RAYS = (300, 297, 276, 303, 228)   # the middle of the 24^2 camera and its surroundings: long rays through the disk
M_E_C2 = 9.1093837015e-28 * 2.99792458e10 * 2.99792458e10   # (multiplied in the coefficients' order: k T_e / M_E_C2 is their Theta_e to the bit)
FALLBACK = dict(fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)   # (the values the fixtures use)
POWERLAW = dict(plasma_power_frac=0.3, plasma_p=2.5, plasma_gamma_min=2.0, plasma_gamma_max=1000.0)               # sim_polarized_powerlaw's electrons
KAPPA_MIX = dict(plasma_power_frac=0.2, plasma_p=3.0, plasma_gamma_min=3.0, plasma_gamma_max=500.0,              # sim_polarized_kappa_mix's
                 plasma_kappa_frac=0.25, plasma_kappa=4.3, plasma_w=2.5)
SPLIT = dict(image_rotation_split="true")
THREE = (1.0e10, 2.3e11, 1.0e15)   # through set_frequencies: bl_polarized_coefficients_kernel instead of the coefficients inside the shading kernel

# name: (grid, parameter overrides, frequency list or None, regimes the case must reach)
CASES = {
    "fixture": ("plain", {}, None, {"none", "thin"}),
    "unit_1e-12": ("plain", dict(simulation_rho_cgs=1.0e-12), None, {"none", "thin", "thick", "faraday_thick"}),
    "unit_1e-14": ("plain", dict(simulation_rho_cgs=1.0e-14), None, {"none", "thin"}),
    "unit_1e-20": ("plain", dict(simulation_rho_cgs=1.0e-20), None, {"none", "thin"}),
    "1e15hz": ("plain", dict(image_frequency=1.0e15), None, {"none", "thin", "rotate_only", "alpha_zeroed", "emission_underflow"}),
    "1e13hz_rhigh_1e4": ("plain", dict(image_frequency=1.0e13, plasma_rat_high=1.0e4), None, {"none", "rotate_only", "cold"}),
    "230ghz_rhigh_1e4": ("plain", dict(plasma_rat_high=1.0e4), None, {"none", "rotate_only", "cold"}),
    # (cold_absorbing: the unit raised from the fixture's 1e-16 to 1e-12, at the fixture's 230 GHz)
    "230ghz_rhigh_1e4_unit_1e-12": ("plain", dict(plasma_rat_high=1.0e4, simulation_rho_cgs=1.0e-12), None,
                                    {"none", "thin", "rotate_only", "alpha_zeroed", "emission_underflow", "cold", "cold_absorbing", "faraday_thick"}),
    "3e13hz_unit_1e-20": ("plain", dict(image_frequency=3.0e13, simulation_rho_cgs=1.0e-20), None, {"none", "thin", "rotate_only", "alpha_zeroed", "emission_underflow"}),
    "1e10hz_unit_1e-14": ("plain", dict(image_frequency=1.0e10, simulation_rho_cgs=1.0e-14), None, {"none", "thin", "thick", "faraday_thick"}),
    # (R_high found by bisection on the oracle: sample 1120 of ray 300 then has Theta_e == 0.01 to the bit, the `>=` of theta_e_zero)
    "1e10hz_theta_e_edge": ("plain", dict(image_frequency=1.0e10, simulation_rho_cgs=1.0e-14, plasma_rat_high=1163.304882993827), None,
                            {"none", "thin", "cold", "cold_absorbing", "faraday_thick", "theta_e_edge"}),
    "split_unit_1e-12": ("plain", dict(SPLIT, simulation_rho_cgs=1.0e-12), None, {"split_none", "split_thin", "split_thick"}),
    "split_1e15hz": ("plain", dict(SPLIT, image_frequency=1.0e15), None,
                     {"split_none", "split_thin", "split_rotate_only", "split_alpha_zeroed", "split_emission_underflow"}),
    "split_1e13hz_rhigh_1e4": ("plain", dict(SPLIT, image_frequency=1.0e13, plasma_rat_high=1.0e4), None, {"split_none", "split_rotate_only", "split_cold"}),
    "degenerate_nan": ("degenerate", dict(fallback_nan="true"), None, {"none", "thin"}),
    "degenerate_fallback": ("degenerate", dict(FALLBACK), None, {"none", "thin"}),
    "degenerate_unit_1e-12": ("degenerate", dict(FALLBACK, simulation_rho_cgs=1.0e-12), None, {"none", "thin", "thick", "faraday_thick"}),
    "three_frequencies": ("plain", {}, THREE, {"none", "thin", "rotate_only", "alpha_zeroed", "emission_underflow"}),
    "powerlaw_unit_1e-12": ("plain", dict(POWERLAW, simulation_rho_cgs=1.0e-12), None, {"none", "thin", "thick", "faraday_thick"}),
    "powerlaw_1e15hz": ("plain", dict(POWERLAW, image_frequency=1.0e15), None, {"none", "thin"}),
    "kappa_mix_unit_1e-12": ("plain", dict(KAPPA_MIX, simulation_rho_cgs=1.0e-12), None, {"none", "thin", "thick", "faraday_thick"}),
    "kappa_mix_1e15hz": ("plain", dict(KAPPA_MIX, image_frequency=1.0e15), None, {"none", "thin"}),
    "ray_flat_unit_1e-12": ("plain", dict(ray_flat="true", simulation_rho_cgs=1.0e-12), None, {"thin", "thick", "faraday_thick"}),
}
# the three edge settings of the variants test: (R_low, R_high, unit)
TRIPLES = [(1.0, 10.0, 1.0e-12), (1.0, 1.0e4, 1.0e-16), (1.0, 10.0, 1.0e-20)]
# rows that the cap of the loose class names: they must be well conditioned (d_AB < 1e-10). Of the rotation-split thick case the
# Stokes rows: its optical-depth row is a plain sum of alpha dl in which the two builds differ by ~1e-9 at every unit, fixture included
MUST_BE_WELL_CONDITIONED = [("split_unit_1e-12", r) for r in range(4)] + [("230ghz_rhigh_1e4", r) for r in range(5)] + [("1e15hz", r) for r in (1, 2, 3)]
ROWS = ("I", "Q", "U", "V", "tau")


def _params(name):
    kind, overrides, hz, _ = CASES[name]
    fx, params, mock_args = gu.load_case(FIXTURE)
    params = dict(params, **overrides)
    if kind != "plain":
        params["cut_sigma_max"] = -1.0   # (the sigma cut would hide what the degenerate grid changes)
    return params


def _blocks(name):
    """The one-frequency parameter blocks whose oracle renders make up the case's image: the case's own, or one per listed frequency"""
    params, hz = _params(name), CASES[name][2]
    return [params] if hz is None else [fu.one_frequency(params, f) for f in hz]


def _oracle(params, grid, variant="blmath", pixels=None, dump_ray=-1):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    p = bl.Params.from_dict(params)
    n_rays = int(params["camera_resolution"]) ** 2 if pixels is None else len(pixels)
    return oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n_rays, pixel_map=pixels, num_threads=16,
                             variant=variant, dump_ray=dump_ray, max_steps=int(params["ray_max_steps"]), dump_polarized=dump_ray >= 0)


@functools.lru_cache(maxsize=None)
def _reference(name, variant="blmath"):
    """The oracle's image of a case in the layout of the case's render, with sample_num and sample_flags"""
    params, grid, hz = _params(name), _grid(CASES[name][0]), CASES[name][2]
    parts = [_oracle(block, grid, variant) for block in _blocks(name)]
    if hz is None:
        return parts[0]
    image = np.zeros((len(fu.labels(params, len(hz))), parts[0]["image"].shape[1]))
    for l, part in enumerate(parts):
        image[fu.rows_of(params, len(hz), l)] = part["image"]
        assert np.array_equal(part["sample_num"], parts[0]["sample_num"]) and np.array_equal(part["sample_flags"], parts[0]["sample_flags"])
    return dict(image=image, sample_num=parts[0]["sample_num"], sample_flags=parts[0]["sample_flags"])


def _row_names(name):
    params, hz = _params(name), CASES[name][2]
    if hz is None:
        return list(ROWS)
    return [f"{'IQUV'[k] if q == 'light' else q}[{l}]" for q, l, k in fu.labels(params, len(hz))]


@functools.lru_cache(maxsize=None)
def _spread(name):
    """d_AB per image row: how far two legitimate builds of the reference - glibc's math and the pinned library - disagree"""
    a, b = _reference(name, "libm"), _reference(name, "blmath")
    assert np.array_equal(a["sample_num"], b["sample_num"]) and np.array_equal(np.isnan(a["image"]), np.isnan(b["image"]))
    return [_distance(a["image"][r], b["image"][r]) for r in range(b["image"].shape[0])]


def _regimes(params, grid):
    """Which of the coupling step's branches the oracle's samples of DUMP_RAYS enter at frequency 0"""
    found = set()
    split = str(params.get("image_rotation_split", "false")) == "true"
    pixels = np.array(DUMP_RAYS, dtype=np.int32)
    for k in range(len(DUMP_RAYS)):
        d = _oracle(params, grid, pixels=pixels, dump_ray=k)["dump"]
        kte, j, alpha, dtau = d["kte"], d["j"], d["alpha"], d["dtau"]
        assert len(kte) > 0, DUMP_RAYS[k]
        eight = np.stack([j, alpha] + [d[key] for key in ("j_q", "j_v", "alpha_q", "alpha_v", "rho_q", "rho_v")])
        formed = np.isfinite(kte)
        assert np.all(eight[:, ~formed] == 0.0)   # (what `none` says: a sample without coefficients is all zeros)
        assert gu.same_bits(dtau, alpha * d["dlambda"]).all()
        rho_p = np.hypot(d["rho_q"], d["rho_v"])
        cold = formed & (kte / M_E_C2 < 0.01) & (d["rho_q"] == 0.0) & (d["rho_v"] != 0.0)
        rotate_only = formed & (alpha == 0.0) & (rho_p > 0.0)
        here = {
            "none": ~formed,
            "thin": (alpha > 0.0) & (rho_p > 0.0) & (dtau <= 100.0),
            "thick": (alpha > 0.0) & (rho_p > 0.0) & (dtau > (200.0 if split else 100.0)),
            "rotate_only": rotate_only,
            "alpha_zeroed": rotate_only & (j > 0.0) & (d["alpha_q"] == 0.0) & (d["alpha_v"] == 0.0),
            "emission_underflow": formed & (j == 0.0) & np.any(j > 0.0),
            "cold": cold,
        }
        if split:
            here = {"split_" + key: mask for key, mask in here.items()}
        else:
            here["cold_absorbing"] = cold & (alpha > 0.0)
            here["faraday_thick"] = rho_p * d["dlambda"] > 1.0e3
            here["theta_e_edge"] = formed & (kte / M_E_C2 == 0.01) & (d["rho_q"] != 0.0) & np.any(cold) & np.any(kte / M_E_C2 > 0.01)
        found |= {key for key, mask in here.items() if np.any(mask)}
    return found


ALL_REGIMES = {"none", "thin", "thick", "rotate_only", "alpha_zeroed", "emission_underflow", "cold"}
ALL_REGIMES = ALL_REGIMES | {"split_" + r for r in ALL_REGIMES} | {"cold_absorbing", "faraday_thick", "theta_e_edge"}


def test_every_regime_is_claimed():
    claimed = set().union(*[want for _, _, _, want in CASES.values()])
    assert claimed == ALL_REGIMES, sorted(ALL_REGIMES ^ claimed)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_regimes(name, built_library):
    """A case that never enters a branch is no coverage of it: the oracle's dumped samples, over the case's frequencies"""
    kind, overrides, hz, want = CASES[name]
    grid = _grid(kind)
    found = set()
    for block in _blocks(name):
        found |= _regimes(block, grid)
    print(f"{name}: {sorted(found)}")
    assert found >= want, (name, sorted(want - found), sorted(found))
    if kind == "degenerate":   # the field-free and pressure-free cells do reach the image: NaN or zero pixels the plain grid lacks
        image = _reference(name)["image"][0]
        plain = _oracle(_params(name), _grid("plain"))["image"][0]
        assert np.isnan(image).sum() + (image == 0.0).sum() > np.isnan(plain).sum() + (plain == 0.0).sum()


def _class_of(name):
    return [d < 1.0e-10 for d in _spread(name)]


def test_reference_spread_keeps_half_the_rows_well_conditioned(built_library):
    """The cap on the loose class of the tolerant tier's bound, from the oracle alone: at least half of all (case, row) pairs are well
    conditioned (d_AB < 1e-10), the rows the issue names among them"""
    classes = {name: _class_of(name) for name in sorted(CASES)}
    for name in sorted(CASES):
        print(f"{name}: d_AB " + ", ".join(f"{row} {d:.1e}" for row, d in zip(_row_names(name), _spread(name))))
    pairs = [ok for rows in classes.values() for ok in rows]
    assert 2 * sum(pairs) >= len(pairs), (sum(pairs), len(pairs))
    for name, row in MUST_BE_WELL_CONDITIONED:
        assert classes[name][row], (name, ROWS[row], _spread(name)[row])


def _render(params, grid, tier, hz=None, triples=None, twice=False):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid(grid)
        ctx.set_arithmetic(tier)
        if hz is not None:
            ctx.set_frequencies(hz)
        if triples is not None:
            ctx.set_polarized_variants([h for _, h, _ in triples], [u for _, _, u in triples], rat_low=[lo for lo, _, _ in triples])
        got = ctx.render()
        if twice:
            return got, ctx.render()
        return got


@functools.lru_cache(maxsize=None)
def _fresh_exact(name):
    """The exact tier's render of a case (shared by the tests of both tiers)"""
    return _render(_params(name), _grid(CASES[name][0]), "exact", CASES[name][2])


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_tier_is_the_oracle(name):
    got, want = _fresh_exact(name), _reference(name)
    st = got["stats"]
    assert st.arithmetic == 0
    if str(_params(name)["ray_flat"]) == "true":   # (flat rays: bl_shade_polarized2_kernel's locate step does not take them)
        assert st.fused_variant == 0 and st.launches_locate == st.n_chunks
    else:
        assert st.fused_variant == 4 and st.launches_locate == 0
    assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["image"].shape == want["image"].shape
    same = gu.same_bits(got["image"], want["image"])
    assert same.all(), (name, [(row, int((~s).sum())) for row, s in zip(_row_names(name), same) if not s.all()])


@gpu
def test_exact_tier_variants_are_their_fresh_renders():
    """Three edge settings as variants of one render: thick and Faraday-thick steps, cold electrons, the thin fixture at 1e-20"""
    params, grid = _params("fixture"), _grid("plain")
    got = _render(params, grid, "exact", triples=TRIPLES)
    assert got["image_by_variant"].shape[0] == len(TRIPLES)
    for v, (low, high, unit) in enumerate(TRIPLES):
        block = dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=unit)
        fresh, want = _render(block, grid, "exact"), _oracle(block, grid)
        assert np.array_equal(got["sample_num"], fresh["sample_num"]) and np.array_equal(got["sample_flags"], fresh["sample_flags"])
        assert gu.same_bits(got["image_by_variant"][v], fresh["image"]).all(), (v, low, high, unit)
        assert gu.same_bits(got["image_by_variant"][v], want["image"]).all(), (v, low, high, unit)
    assert not gu.same_bits(got["image_by_variant"][0], got["image_by_variant"][2]).all()


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_tolerant_tier_within_the_reference_spread(name):
    exact = _fresh_exact(name)
    got, again = _render(_params(name), _grid(CASES[name][0]), "tolerant", CASES[name][2], twice=True)
    assert got["stats"].arithmetic == 1 and exact["stats"].arithmetic == 0
    assert gu.same_bits(got["image"], again["image"]).all()   # (two renders of one context)
    assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
    assert np.array_equal(np.isnan(got["image"]), np.isnan(exact["image"]))
    failed = []
    for r, (row, d_ab) in enumerate(zip(_row_names(name), _spread(name))):
        d = _distance(got["image"][r], exact["image"][r])
        well = d_ab < 1.0e-10
        print(f"{name} {row}: d_AB {d_ab:.1e}, tolerant vs exact {d:.1e}, {'well conditioned' if well else 'loose'}")
        if not (d < 1.0e-9 if well else d <= max(1.0e-9, 100.0 * d_ab)):
            failed.append((row, d_ab, d))
    assert not failed, (name, failed)
