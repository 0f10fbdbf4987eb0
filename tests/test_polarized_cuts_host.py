"""Polarized variants with a sigma cut each (bl_set_polarized_variants_sigma) on host-only contexts (no GPU): the exported symbol, that
sigma_max = NULL is bl_set_polarized_variants, the argument error of a non-finite cut, the refusals in the words the triples have,
that a refused call changes nothing, that bl_set_polarized_variants clears the cuts, that bl_set_sigma_cuts still refuses polarized
contexts, and the keyword of Context.set_polarized_variants (broadcast, length check, what the flux fit restores)."""
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


def _host_context(case, **overrides):
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case(case)
    p = bl.Params.from_dict(dict(params, **overrides))
    return p, bl.Context(p, device=BL_DEVICE_NONE)


def _ptr(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def _set(ctx, low, high, rho, cuts, n=None):
    keep = [_ptr(v) for v in (low, high, rho)] + [_ptr(cuts) if cuts is not None else (None, None)]
    n = keep[2][0].size if n is None else n
    return ctx._lib.bl_set_polarized_variants_sigma(ctx._ctx, n, *(p for _, p in keep))


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode().rstrip("\n")


def _state(ctx):
    """What a host-only context shows of its variants: the counts, the image rows and every variant's file name"""
    n = ctx.num_variants
    return (ctx.num_polarized_variants, n, ctx.num_quantities, [ctx.variant_output_path(0, v) for v in range(n)])


def test_symbol_exported_and_declared(built_library):
    from blacklight_amd import _capi
    import blacklight_amd as bl
    assert hasattr(C.CDLL(bl.LIB_PATH), "bl_set_polarized_variants_sigma")
    assert len(_capi.lib().bl_set_polarized_variants_sigma.argtypes) == 6
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    assert re.search(r"BL_API\s+int\s+bl_set_polarized_variants_sigma\s*\(\s*bl_ctx\s*\*ctx,\s*int\s+n,\s*const\s+double\s*\*rat_low,\s*const\s+double\s*\*rat_high,"
                     r"\s*const\s+double\s*\*rho_cgs,\s*const\s+double\s*\*sigma_max\s*\)", header)
    assert _capi.lib().bl_set_polarized_variants_sigma(None, 0, None, None, None, None) == BL_E_ARG   # no context


def test_null_cuts_are_bl_set_polarized_variants(built_library, tmp_path):
    p, with_null = _host_context("sim_polarized", output_file=str(tmp_path / "image.npz"))
    q, plain = _host_context("sim_polarized", output_file=str(tmp_path / "image.npz"))
    n_q = plain.num_quantities
    assert _set(with_null, LOW, HIGH, RHO, None) == 0
    plain.set_polarized_variants(HIGH, RHO, rat_low=LOW)
    assert _state(with_null) == _state(plain) and _state(plain)[:3] == (3, 3, 3 * n_q)
    assert _state(plain)[3][1].endswith("image.v01.npz")
    # ... and cuts add no rows, no variants and no tag: they change what variant v is
    assert _set(with_null, LOW, HIGH, RHO, CUTS) == 0
    assert _state(with_null) == _state(plain)
    assert _set(with_null, LOW, HIGH, RHO, CUTS, n=0) == 0 and _state(with_null)[:3] == (0, 1, n_q)   # n = 0 restores, cuts or not
    assert with_null._lib.bl_set_polarized_variants_sigma(with_null._ctx, 0, None, None, None, None) == 0
    with_null.close()
    plain.close()


def test_a_non_finite_cut_is_an_argument_error_that_changes_nothing(built_library):
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants(HIGH[:2], RHO[:2], rat_low=LOW[:2], sigma_max=[0.5, 2.0])
    before = _state(ctx)
    for index, bad in ((0, math.nan), (1, math.inf), (2, -math.inf)):
        cuts = list(CUTS)
        cuts[index] = bad
        assert _set(ctx, LOW, HIGH, RHO, cuts) == BL_E_ARG
        assert _last_error(ctx) == f"Error: bl_set_polarized_variants_sigma: the sigma cut of variant {index} is not finite."
        assert _state(ctx) == before and ctx.polarized_cuts == [0.5, 2.0]
    # the other arguments are checked as the triples': the same texts
    assert _set(ctx, np.ones(17), np.ones(17), np.full(17, 1.0e-16), np.ones(17)) == BL_E_ARG
    assert "0 <= n <= 16" in _last_error(ctx) and "bl_set_polarized_variants" in _last_error(ctx)
    assert _set(ctx, LOW, HIGH, RHO, CUTS, n=-1) == BL_E_ARG
    assert _set(ctx, LOW, HIGH, [1.0e-16, 0.0, 1.0e-16], CUTS) == BL_E_ARG and "finite value > 0" in _last_error(ctx)
    assert _set(ctx, LOW, [10.0, math.nan, 10.0], RHO, CUTS) == BL_E_ARG and "non-finite" in _last_error(ctx)
    good, ptr = _ptr([1.0, 1.0])
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr)):
        assert ctx._lib.bl_set_polarized_variants_sigma(ctx._ctx, 2, *args) == BL_E_ARG
    assert _state(ctx) == before
    assert _set(ctx, np.ones(16), np.geomspace(1.0, 160.0, 16), np.geomspace(1.0e-18, 1.0e-14, 16), np.linspace(-1.0, 14.0, 16)) == 0
    assert ctx.num_polarized_variants == 16
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
    assert _set(ctx, *args, np.full(n, 1.0)) == BL_E_UNSUPPORTED
    assert _last_error(ctx) == message
    assert ctx.num_polarized_variants == 0 and ctx.num_variants == 1
    low, high, rho = (_ptr(a) for a in args)   # ... the words bl_set_polarized_variants has
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, n, low[1], high[1], rho[1]) == BL_E_UNSUPPORTED and _last_error(ctx) == message
    if n == 2:   # one quadruple is a single image: allowed, and a refused call after it changes nothing
        assert _set(ctx, [1.0], [20.0], [3.0e-16], [0.5]) == 0 and ctx.num_polarized_variants == 1
        assert _set(ctx, *args, np.full(n, 1.0)) == BL_E_UNSUPPORTED and ctx.num_polarized_variants == 1
    ctx.close()


def test_bl_set_polarized_variants_clears_the_cuts(built_library):
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants(HIGH, RHO, rat_low=LOW, sigma_max=CUTS)
    assert ctx.polarized_cuts == CUTS and ctx.num_polarized_variants == 3
    ctx.set_polarized_variants(HIGH, RHO, rat_low=LOW)
    assert ctx.polarized_cuts is None and ctx.num_polarized_variants == 3
    assert ctx.polarized_variants == [(h, lo, u) for h, lo, u in zip(HIGH, LOW, RHO)]
    ctx.set_polarized_variants(HIGH, RHO, rat_low=LOW, sigma_max=CUTS)
    ctx.set_polarized_variants([], [])
    assert ctx.polarized_cuts is None and ctx.num_polarized_variants == 0
    # ... and the C entry point of that name itself, behind a call with cuts: accepted, the same counts, and refused calls of either
    # kind after it change nothing (what it does to the cuts only a render shows: tests/test_gpu_polarized_cuts.py, the series test)
    assert _set(ctx, LOW, HIGH, RHO, CUTS) == 0 and ctx.num_polarized_variants == 3
    before = _state(ctx)
    (_, low), (_, high), (_, rho) = keep = [_ptr(v) for v in (LOW[:2], HIGH[:2], RHO[:2])]
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 2, low, high, rho) == 0 and ctx.num_polarized_variants == 2
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 3, low, None, rho) == BL_E_ARG and ctx.num_polarized_variants == 2
    assert _set(ctx, LOW, HIGH, RHO, [1.0, math.inf, 1.0]) == BL_E_ARG and ctx.num_polarized_variants == 2
    assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 0, None, None, None) == 0 and _state(ctx)[:2] == (0, 1) and before[:2] == (3, 3)
    ctx.close()


def test_bl_set_sigma_cuts_still_refuses_polarized_contexts(built_library):
    import blacklight_amd as bl
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants(HIGH, RHO, rat_low=LOW, sigma_max=CUTS)
    with pytest.raises(bl.BlacklightError) as err:
        ctx.set_sigma_cuts([1.0])
    assert err.value.code == BL_E_UNSUPPORTED
    assert str(err.value) == "Error: Sigma cuts: the polarized axis is not built yet; polarized runs render one sigma cut (image_polarization = true)."
    assert ctx.num_sigma_cuts == 0 and ctx.num_polarized_variants == 3 and ctx.polarized_cuts == CUTS
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    comment = header[header.index("/* Sigma cuts (cut_sigma_max"):header.index("#define BL_MAX_SIGMA_CUTS")]
    assert "bl_set_polarized_variants_sigma" in comment   # the comment on that call points at the polarized door
    ctx.close()


def test_keyword_broadcasts_a_scalar_and_rejects_a_length_mismatch(built_library):
    p, ctx = _host_context("sim_polarized")
    assert ctx.polarized_cuts is None
    ctx.set_polarized_variants(HIGH, RHO, sigma_max=3.0)
    assert ctx.polarized_cuts == [3.0, 3.0, 3.0] and ctx.num_polarized_variants == 3
    ctx.set_polarized_variants(40.0, 1.0e-16, sigma_max=[-1.0])
    assert ctx.polarized_cuts == [-1.0] and ctx.polarized_variants == [(40.0, 1.0, 1.0e-16)]
    for wrong in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], []):
        with pytest.raises(ValueError, match="one value per variant"):
            ctx.set_polarized_variants(HIGH, RHO, sigma_max=wrong)
        assert ctx.polarized_cuts == [-1.0] and ctx.num_polarized_variants == 1
    import blacklight_amd as bl
    with pytest.raises(bl.BlacklightError) as err:
        ctx.set_polarized_variants(HIGH, RHO, sigma_max=[1.0, math.nan, 1.0])
    assert err.value.code == BL_E_ARG and "variant 1 is not finite" in str(err.value)
    assert ctx.polarized_cuts == [-1.0] and ctx.num_polarized_variants == 1
    ctx.close()


def test_the_polarized_fit_leaves_the_cuts_as_it_found_them(built_library):
    from blacklight_amd import flux
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants([7.0, 9.0], [5.0e-17, 6.0e-17], sigma_max=[0.5, -1.0])
    per_jy = 1.0 / flux.total_flux_jy(np.ones((1, 4)), p, 8.1e3)
    seen = []

    def render():   # Stokes-I flux 0.01 R_high rho / 1e-16 for every variant set (a uniform image)
        variants = ctx.polarized_variants
        seen.append(ctx.polarized_cuts)
        image = np.zeros((len(variants), 4, 4))
        for v, (high, low, rho) in enumerate(variants):
            image[v, 0] = 0.01 * high * (rho / 1.0e-16) * per_jy
        return dict(image=image.reshape(-1, 4), image_by_variant=image)

    ctx.render = render
    found, renders = ctx.fit_density_units_polarized([(10.0, 1.0)], 1.0, 8.1e3, 1.0e-18, 1.0e-12, rtol=1.0e-3)
    assert renders == len(seen) >= 2 and all(cuts is None for cuts in seen)   # (the trials: the parameter block's cut)
    assert abs(found[0][1] - 1.0) <= 1.0e-3
    assert ctx.polarized_variants == [(7.0, 1.0, 5.0e-17), (9.0, 1.0, 6.0e-17)] and ctx.polarized_cuts == [0.5, -1.0]
    assert ctx.num_polarized_variants == 2
    ctx.close()
