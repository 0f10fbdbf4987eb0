"""Polarized variants with an electron distribution each (bl_set_polarized_variants_electrons) on host-only contexts (no GPU): the
exported symbols, every argument error's text, the kappa range, the reference's warnings (each once per call), the shape values that
are not read when a fraction is zero, the getter for set, unset and out-of-range variants, that n = 0 clears, that the two earlier
setters drop the mixes, the refusals in the words the triples have, and the keyword of Context.set_polarized_variants."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import golden_util as gu

BL_DEVICE_NONE = -2
BL_E_UNSUPPORTED = 3
BL_E_ARG = 5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOW, HIGH, RHO = [1.0, 1.0, 2.0], [10.0, 40.0, 160.0], [1.0e-17, 1.0e-16, 1.0e-15]
CUTS = [0.1, -1.0, 10.0]
KEYS = ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")
THERMAL = dict(power_frac=0.0, p=0.0, gamma_min=0.0, gamma_max=0.0, kappa_frac=0.0, kappa=0.0, w=0.0)
POWER = dict(THERMAL, power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0)
KAPPA = dict(THERMAL, kappa_frac=0.4, kappa=4.0, w=1.5)
MIX = dict(power_frac=0.2, p=3.0, gamma_min=3.0, gamma_max=500.0, kappa_frac=0.25, kappa=4.3, w=2.5)
WARN_POWER = "Warning: Fraction of power-law electrons outside [0, 1].\n"
WARN_KAPPA = "Warning: Fraction of kappa-distribution electrons outside [0, 1].\n"
WARN_THERMAL = "Warning: Fraction of thermal electrons outside [0, 1].\n"
WARN_INTERPOLATE = "Warning: Polarized transport will interpolate formulas based on kappa.\n"


def _host_context(case, **overrides):
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case(case)
    p = bl.Params.from_dict(dict(params, **overrides))
    return p, bl.Context(p, device=BL_DEVICE_NONE)


def _ptr(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def _mixes(mappings):
    from blacklight_amd import _capi
    array = (_capi.ElectronMix * len(mappings))()
    for v, mapping in enumerate(mappings):
        for key in KEYS:
            setattr(array[v], key, mapping[key])
    return array


def _set(ctx, low, high, rho, cuts, mappings, n=None):
    keep = [_ptr(v) for v in (low, high, rho)] + [_ptr(cuts) if cuts is not None else (None, None)]
    mixes = _mixes(mappings) if mappings is not None else None
    n = keep[2][0].size if n is None else n
    return ctx._lib.bl_set_polarized_variants_electrons(ctx._ctx, n, *(p for _, p in keep), C.cast(mixes, C.c_void_p) if mixes is not None else None)


def _get(ctx, variant):
    from blacklight_amd import _capi
    mix = _capi.ElectronMix()
    rc = ctx._lib.bl_polarized_variant_electrons(ctx._ctx, variant, C.byref(mix))
    return rc, {key: getattr(mix, key) for key in KEYS}


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode().rstrip("\n")


def _warnings(ctx):
    return ctx._lib.bl_warnings(ctx._ctx).decode()


def _state(ctx):
    n = ctx.num_variants
    return (ctx.num_polarized_variants, n, ctx.num_quantities, [ctx.variant_output_path(0, v) for v in range(n)])


def test_symbols_exported_and_declared(built_library):
    from blacklight_amd import _capi
    import blacklight_amd as bl
    lib = C.CDLL(bl.LIB_PATH)
    assert hasattr(lib, "bl_set_polarized_variants_electrons") and hasattr(lib, "bl_polarized_variant_electrons")
    assert len(_capi.lib().bl_set_polarized_variants_electrons.argtypes) == 7
    assert C.sizeof(_capi.ElectronMix) == 64
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+bl_electron_mix\s*\{\s*double\s+power_frac,\s*p,\s*gamma_min,\s*gamma_max;[^}]*double\s+kappa_frac,\s*kappa,\s*w;"
                     r"[^}]*double\s+reserved;[^}]*\}\s*bl_electron_mix;", header)
    assert re.search(r"BL_API\s+int\s+bl_set_polarized_variants_electrons\s*\(\s*bl_ctx\s*\*ctx,\s*int\s+n,\s*const\s+double\s*\*rat_low,\s*const\s+double\s*"
                     r"\*rat_high,\s*const\s+double\s*\*rho_cgs,\s*const\s+double\s*\*sigma_max,\s*const\s+bl_electron_mix\s*\*mix\s*\)", header)
    assert re.search(r"BL_API\s+int\s+bl_polarized_variant_electrons\s*\(\s*const\s+bl_ctx\s*\*ctx,\s*int\s+variant,\s*bl_electron_mix\s*\*out\s*\)", header)
    assert _capi.lib().bl_set_polarized_variants_electrons(None, 0, None, None, None, None, None) == BL_E_ARG   # no context
    assert _capi.lib().bl_polarized_variant_electrons(None, 0, None) == BL_E_ARG


def test_null_mixes_are_the_earlier_setters(built_library, tmp_path):
    p, ctx = _host_context("sim_polarized_kappa", output_file=str(tmp_path / "image.npz"))
    q, plain = _host_context("sim_polarized_kappa", output_file=str(tmp_path / "image.npz"))
    block = _get(plain, 0)[1]
    assert block == dict(THERMAL, kappa_frac=float(p.get("plasma_kappa_frac")), kappa=float(p.get("plasma_kappa")), w=float(p.get("plasma_w")))
    assert _set(ctx, LOW, HIGH, RHO, None, None) == 0
    plain.set_polarized_variants(HIGH, RHO, rat_low=LOW)
    assert _state(ctx) == _state(plain) and _state(ctx)[:2] == (3, 3)
    assert _set(ctx, LOW, HIGH, RHO, CUTS, None) == 0
    plain.set_polarized_variants(HIGH, RHO, rat_low=LOW, sigma_max=CUTS)
    assert _state(ctx) == _state(plain)
    assert [_get(ctx, v) for v in range(3)] == [(0, block)] * 3   # no mix set: the parameter block's own for every variant
    # ... and mixes add no rows, no variants and no tag: they change what variant v is
    assert _set(ctx, LOW, HIGH, RHO, CUTS, [POWER, KAPPA, MIX]) == 0
    assert _state(ctx) == _state(plain)
    ctx.close()
    plain.close()


def test_getter_for_set_unset_and_out_of_range_variants(built_library):
    p, ctx = _host_context("sim_polarized")
    assert _get(ctx, 0) == (0, THERMAL)   # nothing set: variant 0 is the parameter block's render
    assert _get(ctx, 1)[0] == BL_E_ARG and _get(ctx, -1)[0] == BL_E_ARG
    assert ctx._lib.bl_polarized_variant_electrons(ctx._ctx, 0, None) == BL_E_ARG
    assert _set(ctx, LOW, HIGH, RHO, None, [POWER, KAPPA, MIX]) == 0
    assert [_get(ctx, v) for v in range(3)] == [(0, POWER), (0, KAPPA), (0, MIX)]
    assert _get(ctx, 3)[0] == BL_E_ARG and _get(ctx, -1)[0] == BL_E_ARG
    assert ctx.polarized_electrons == [POWER, KAPPA, MIX]
    # n = 0 clears, mixes or not
    assert _set(ctx, LOW, HIGH, RHO, None, [POWER, KAPPA, MIX], n=0) == 0
    assert _state(ctx)[:2] == (0, 1) and _get(ctx, 0) == (0, THERMAL) and _get(ctx, 1)[0] == BL_E_ARG
    assert ctx._lib.bl_set_polarized_variants_electrons(ctx._ctx, 0, None, None, None, None, None) == 0
    ctx.close()


NOT_FINITE = [
    ("power_frac", POWER), ("p", POWER), ("gamma_min", POWER), ("gamma_max", POWER), ("kappa_frac", KAPPA), ("kappa", KAPPA), ("w", KAPPA),
]


@pytest.mark.parametrize("key, base", NOT_FINITE)
def test_a_value_that_is_read_must_be_finite(key, base, built_library):
    p, ctx = _host_context("sim_polarized")
    assert _set(ctx, LOW[:2], HIGH[:2], RHO[:2], [0.5, 2.0], [POWER, KAPPA]) == 0
    before = _state(ctx)
    for index, bad in ((0, math.nan), (1, math.inf), (2, -math.inf)):
        mappings = [MIX, MIX, MIX]
        mappings[index] = dict(base, **{key: bad})
        assert _set(ctx, LOW, HIGH, RHO, CUTS, mappings) == BL_E_ARG
        assert _last_error(ctx) == f"Error: bl_set_polarized_variants_electrons: variant {index} has a {key} that is not finite."
        assert _state(ctx) == before and [_get(ctx, v)[1] for v in range(2)] == [POWER, KAPPA]   # a failed call changes nothing
    assert _warnings(ctx) == ""
    ctx.close()


def test_the_other_arguments_are_checked_as_the_quadruples_are(built_library):
    p, ctx = _host_context("sim_polarized")
    mixes = [MIX, MIX, MIX]
    assert _set(ctx, np.ones(17), np.ones(17), np.full(17, 1.0e-16), np.ones(17), [MIX] * 17) == BL_E_ARG
    assert "0 <= n <= 16" in _last_error(ctx) and "bl_set_polarized_variants" in _last_error(ctx)
    assert _set(ctx, LOW, HIGH, RHO, CUTS, mixes, n=-1) == BL_E_ARG
    assert _set(ctx, LOW, HIGH, [1.0e-16, 0.0, 1.0e-16], CUTS, mixes) == BL_E_ARG and "finite value > 0" in _last_error(ctx)
    assert _set(ctx, LOW, [10.0, math.nan, 10.0], RHO, CUTS, mixes) == BL_E_ARG and "non-finite" in _last_error(ctx)
    assert _set(ctx, LOW, HIGH, RHO, [1.0, math.inf, 1.0], mixes) == BL_E_ARG
    assert _last_error(ctx) == "Error: bl_set_polarized_variants_sigma: the sigma cut of variant 1 is not finite."
    assert ctx.num_polarized_variants == 0
    assert _set(ctx, np.ones(16), np.geomspace(1.0, 160.0, 16), np.geomspace(1.0e-18, 1.0e-14, 16), np.linspace(-1.0, 14.0, 16), [POWER, KAPPA] * 8) == 0
    assert ctx.num_polarized_variants == 16 and _get(ctx, 15) == (0, KAPPA)
    ctx.close()


def test_kappa_outside_the_polarized_fits_is_refused(built_library):
    p, ctx = _host_context("sim_polarized")
    for index, kappa in ((0, 3.4999), (1, 5.0001), (2, 0.0), (1, -4.0)):
        mappings = [KAPPA, KAPPA, KAPPA]
        mappings[index] = dict(KAPPA, kappa=kappa)
        assert _set(ctx, LOW, HIGH, RHO, None, mappings) == BL_E_ARG
        assert _last_error(ctx) == f"Error: bl_set_polarized_variants_electrons: variant {index}: Polarized transport only supports kappa in [3.5, 5]."
        assert ctx.num_polarized_variants == 0 and _warnings(ctx) == ""
    assert _set(ctx, LOW, HIGH, RHO, None, [dict(KAPPA, kappa=3.5), dict(KAPPA, kappa=5.0), dict(KAPPA, kappa=4.5)]) == 0   # the ends are in
    assert _warnings(ctx) == ""   # ... and none of 3.5, 4, 4.5, 5 is interpolated
    ctx.close()


def test_shape_values_of_an_absent_distribution_are_neither_read_nor_checked(built_library):
    p, ctx = _host_context("sim_polarized")
    odd = [dict(power_frac=0.0, p=math.nan, gamma_min=math.inf, gamma_max=-math.inf, kappa_frac=0.4, kappa=4.0, w=1.5),   # no power law
           dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0, kappa=99.0, w=math.nan),          # no kappa electrons
           dict(power_frac=0.0, p=-7.0, gamma_min=0.0, gamma_max=math.nan, kappa_frac=0.0, kappa=math.inf, w=-1.0)]      # thermal
    assert _set(ctx, LOW, HIGH, RHO, None, odd) == 0 and _warnings(ctx) == ""
    for v in range(3):   # the getter returns them as given
        rc, got = _get(ctx, v)
        assert rc == 0
        for key in KEYS:
            assert got[key] == odd[v][key] or (math.isnan(got[key]) and math.isnan(odd[v][key])), (v, key)
    # ... and there is no other range check: the reference has none
    assert _set(ctx, LOW[:1], HIGH[:1], RHO[:1], None, [dict(power_frac=0.3, p=-2.0, gamma_min=-5.0, gamma_max=0.0, kappa_frac=0.1, kappa=4.0, w=-3.0)]) == 0
    ctx.close()


def test_the_four_warnings_each_once_per_call(built_library):
    p, ctx = _host_context("sim_polarized")
    assert _warnings(ctx) == ""
    # two variants with a power-law fraction outside [0, 1], whose thermal fraction is outside too: one line each
    assert _set(ctx, LOW, HIGH, RHO, None, [dict(POWER, power_frac=1.5), dict(POWER, power_frac=-0.25), THERMAL]) == 0
    assert _warnings(ctx) == WARN_POWER + WARN_THERMAL
    # the kappa fraction, and an interpolated kappa in two variants
    assert _set(ctx, LOW, HIGH, RHO, None, [dict(KAPPA, kappa_frac=1.25, kappa=4.3), dict(KAPPA, kappa=3.7), dict(KAPPA, kappa_frac=-0.5)]) == 0
    assert _warnings(ctx) == WARN_POWER + WARN_THERMAL + WARN_KAPPA + WARN_INTERPOLATE + WARN_THERMAL
    # fractions inside [0, 1] whose sum is not: the thermal fraction alone
    before = _warnings(ctx)
    assert _set(ctx, LOW[:1], HIGH[:1], RHO[:1], None, [dict(MIX, power_frac=0.75, kappa_frac=0.75, kappa=4.5)]) == 0
    assert _warnings(ctx) == before + WARN_THERMAL
    # a kappa that is not read warns of nothing, nor does a call without mixes, nor one that fails
    before = _warnings(ctx)
    assert _set(ctx, LOW[:1], HIGH[:1], RHO[:1], None, [dict(THERMAL, kappa=4.3)]) == 0
    assert _set(ctx, LOW, HIGH, RHO, CUTS, None) == 0
    assert _set(ctx, LOW, HIGH, RHO, None, [dict(POWER, power_frac=2.0), dict(KAPPA, kappa=9.0), THERMAL]) == BL_E_ARG
    assert _warnings(ctx) == before
    ctx.close()


def test_the_earlier_setters_drop_the_mixes(built_library):
    p, ctx = _host_context("sim_polarized")
    (_, low), (_, high), (_, rho), (_, cuts) = keep = [_ptr(v) for v in (LOW, HIGH, RHO, CUTS)]
    assert _set(ctx, LOW, HIGH, RHO, CUTS, [POWER, KAPPA, MIX]) == 0 and _get(ctx, 1) == (0, KAPPA)
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 3, low, high, rho) == 0
    assert ctx.num_polarized_variants == 3 and [_get(ctx, v) for v in range(3)] == [(0, THERMAL)] * 3
    assert _set(ctx, LOW, HIGH, RHO, CUTS, [POWER, KAPPA, MIX]) == 0 and _get(ctx, 2) == (0, MIX)
    assert ctx._lib.bl_set_polarized_variants_sigma(ctx._ctx, 3, low, high, rho, cuts) == 0
    assert ctx.num_polarized_variants == 3 and [_get(ctx, v) for v in range(3)] == [(0, THERMAL)] * 3
    # (a refused call of either drops nothing)
    assert _set(ctx, LOW, HIGH, RHO, CUTS, [POWER, KAPPA, MIX]) == 0
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 3, low, None, rho) == BL_E_ARG and _get(ctx, 0) == (0, POWER)
    ctx.close()


REFUSALS = [
    ("sim_dp_interp", {}, 1, "Error: Polarized variants: the context is not polarized (image_polarization = false); bl_set_electron_models and "
                             "bl_set_density_units render the variants of an unpolarized run."),
    ("formula_flat", {}, 1, "Error: Polarized variants: formula mode has neither an electron temperature nor a density (model_type = formula)."),
    ("slow_interp", {"image_polarization": True}, 1, "Error: Polarized variants: slow light renders one variant (slow_light_on = true)."),
    ("sim_polarized_adaptive", {}, 2, "Error: Polarized variants: adaptive refinement reads one image; n >= 2 variants need adaptive_max_level = 0."),
    ("sim_render", {"image_light": True, "image_polarization": True}, 2,
     "Error: Polarized variants: renderings come out once; n >= 2 variants need render_num_images = 0."),
]


@pytest.mark.parametrize("case, overrides, n, message", REFUSALS)
def test_refusals_in_the_words_of_the_triples(case, overrides, n, message, built_library):
    p, ctx = _host_context(case, **overrides)
    args = (np.ones(n), np.full(n, 20.0), np.geomspace(1.0e-17, 1.0e-16, n))
    assert _set(ctx, *args, np.full(n, 1.0), [MIX] * n) == BL_E_UNSUPPORTED
    assert _last_error(ctx) == message
    assert ctx.num_polarized_variants == 0 and ctx.num_variants == 1
    if n == 2:   # one tuple is a single image: allowed, and a refused call after it changes nothing
        assert _set(ctx, [1.0], [20.0], [3.0e-16], [0.5], [KAPPA]) == 0 and ctx.num_polarized_variants == 1
        assert _set(ctx, *args, np.full(n, 1.0), [MIX] * n) == BL_E_UNSUPPORTED and ctx.num_polarized_variants == 1 and _get(ctx, 0) == (0, KAPPA)
    ctx.close()


def test_keyword_takes_one_mapping_or_one_per_variant(built_library):
    import blacklight_amd as bl
    p, ctx = _host_context("sim_polarized_kappa")
    block = ctx.polarized_electrons[0]
    assert not ctx.polarized_electrons_set and block["kappa_frac"] != 0.0
    ctx.set_polarized_variants(HIGH, RHO, electrons=dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0))   # a missing key: the block's value
    assert ctx.polarized_electrons == [dict(block, power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0)] * 3 and ctx.polarized_electrons_set
    ctx.set_polarized_variants(HIGH, RHO, sigma_max=CUTS, electrons=[{}, dict(kappa_frac=0.0), MIX])
    assert ctx.polarized_electrons == [block, dict(block, kappa_frac=0.0), MIX] and ctx.polarized_cuts == CUTS
    for wrong in ([MIX, MIX], [MIX] * 4):
        with pytest.raises(ValueError, match="one mapping or one per variant"):
            ctx.set_polarized_variants(HIGH, RHO, electrons=wrong)
    with pytest.raises(ValueError, match="unknown electron key"):
        ctx.set_polarized_variants(HIGH, RHO, electrons=dict(plasma_kappa=4.0))
    with pytest.raises(bl.BlacklightError) as err:
        ctx.set_polarized_variants(HIGH, RHO, electrons=[MIX, dict(MIX, kappa=6.0), MIX])
    assert err.value.code == BL_E_ARG and "variant 1: Polarized transport only supports kappa in [3.5, 5]." in str(err.value)
    assert ctx.polarized_electrons == [block, dict(block, kappa_frac=0.0), MIX]   # the failed calls changed nothing
    ctx.set_polarized_variants(HIGH, RHO)
    assert ctx.polarized_electrons == [block] * 3 and not ctx.polarized_electrons_set
    ctx.set_polarized_variants([], [], electrons=MIX)
    assert ctx.num_polarized_variants == 0 and ctx.polarized_electrons == [block]
    ctx.close()


def test_the_polarized_fit_leaves_the_mixes_as_it_found_them(built_library):
    from blacklight_amd import flux
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants([7.0, 9.0], [5.0e-17, 6.0e-17], sigma_max=[0.5, -1.0], electrons=[POWER, KAPPA])
    per_jy = 1.0 / flux.total_flux_jy(np.ones((1, 4)), p, 8.1e3)
    seen = []

    def render():   # Stokes-I flux 0.01 R_high rho / 1e-16 for every variant set (a uniform image)
        variants = ctx.polarized_variants
        seen.append(ctx.polarized_electrons_set)
        image = np.zeros((len(variants), 4, 4))
        for v, (high, low, rho) in enumerate(variants):
            image[v, 0] = 0.01 * high * (rho / 1.0e-16) * per_jy
        return dict(image=image.reshape(-1, 4), image_by_variant=image)

    ctx.render = render
    found, renders = ctx.fit_density_units_polarized([(10.0, 1.0)], 1.0, 8.1e3, 1.0e-18, 1.0e-12, rtol=1.0e-3)
    assert renders == len(seen) >= 2 and not any(seen)   # (the trials: the parameter block's mix)
    assert ctx.polarized_variants == [(7.0, 1.0, 5.0e-17), (9.0, 1.0, 6.0e-17)] and ctx.polarized_cuts == [0.5, -1.0]
    assert ctx.polarized_electrons == [POWER, KAPPA] and ctx.polarized_electrons_set
    ctx.close()
