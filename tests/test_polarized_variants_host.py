"""Polarized variants (bl_set_polarized_variants) on host-only contexts (no GPU): the exported symbols, argument validation, what is
refused and why, the image row count, the host steps that read one image, the Stokes fluxes and net polarization of an image and
the stepping of the polarized flux fit (against a stub render)."""
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


def _host_context(case, **overrides):
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case(case)
    params = dict(params, **overrides)
    p = bl.Params.from_dict(params)
    return p, bl.Context(p, device=BL_DEVICE_NONE)


def _arr(values):
    return np.ascontiguousarray(values, dtype=np.float64)


def _set(ctx, low, high, rho, n=None):
    low, high, rho = _arr(low), _arr(high), _arr(rho)
    n = rho.size if n is None else n
    return ctx._lib.bl_set_polarized_variants(ctx._ctx, n, low.ctypes.data_as(C.c_void_p), high.ctypes.data_as(C.c_void_p),
                                              rho.ctypes.data_as(C.c_void_p))


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode()


def test_symbols_exported_and_declared(built_library):
    from blacklight_amd import _capi
    lib = _capi.lib()
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_set_polarized_variants", "bl_num_polarized_variants"):
        assert hasattr(lib, name)
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_POLARIZED_VARIANTS\s+16\b", header)


def test_variants_scale_the_image_rows(built_library):
    p, ctx = _host_context("sim_polarized")
    n_q = ctx.num_quantities
    assert ctx.num_polarized_variants == 0 and ctx.polarized_variants == []
    ctx.set_polarized_variants([1.0, 40.0, 160.0], [1.0e-17, 1.0e-16, 1.0e-15])
    assert ctx.num_polarized_variants == 3 and ctx.num_quantities == 3 * n_q
    assert ctx.polarized_variants == [(1.0, 1.0, 1.0e-17), (40.0, 1.0, 1.0e-16), (160.0, 1.0, 1.0e-15)]
    ctx.set_polarized_variants(20.0, 2.0e-16, rat_low=2.0)   # n = 1: one triple instead of the parameter block's, same rows
    assert ctx.num_polarized_variants == 1 and ctx.num_quantities == n_q
    assert ctx.polarized_variants == [(20.0, 2.0, 2.0e-16)]
    ctx.set_polarized_variants([], [])                       # n = 0 restores
    assert ctx.num_polarized_variants == 0 and ctx.num_quantities == n_q and ctx.polarized_variants == []
    ctx.close()


def test_bad_arguments(built_library):
    p, ctx = _host_context("sim_polarized")
    lib = ctx._lib
    one = np.ones(17)
    assert _set(ctx, one, one, np.full(17, 1.0e-16)) == BL_E_ARG
    assert "16" in _last_error(ctx) and "bl_set_polarized_variants" in _last_error(ctx)
    assert _set(ctx, [1.0], [1.0], [1.0e-16], n=-1) == BL_E_ARG
    for bad in (math.nan, math.inf, 0.0, -1.0e-16):
        assert _set(ctx, [1.0, 1.0], [10.0, 10.0], [1.0e-16, bad]) == BL_E_ARG, bad
        assert "finite value > 0" in _last_error(ctx)
    for bad in (math.nan, math.inf, -math.inf):
        assert _set(ctx, [1.0, bad], [10.0, 10.0], [1.0e-16, 1.0e-16]) == BL_E_ARG, bad
        assert "non-finite" in _last_error(ctx)
        assert _set(ctx, [1.0, 1.0], [bad, 10.0], [1.0e-16, 1.0e-16]) == BL_E_ARG, bad
        assert "non-finite" in _last_error(ctx)
    good = _arr([1.0, 1.0])
    ptr = good.ctypes.data_as(C.c_void_p)
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert lib.bl_set_polarized_variants(ctx._ctx, 2, *args) == BL_E_ARG
    assert lib.bl_set_polarized_variants(None, 0, None, None, None) == BL_E_ARG
    assert lib.bl_num_polarized_variants(None) == -1
    assert ctx.num_polarized_variants == 0   # (nothing was set by a refused call)
    assert lib.bl_set_polarized_variants(ctx._ctx, 0, None, None, None) == 0
    assert _set(ctx, np.ones(16), np.geomspace(1.0, 160.0, 16), np.geomspace(1.0e-18, 1.0e-14, 16)) == 0
    assert ctx.num_polarized_variants == 16
    assert _set(ctx, [1.0], [math.nan], [1.0e-16]) == BL_E_ARG   # (a refused call changes nothing)
    assert ctx.num_polarized_variants == 16
    ctx.close()


@pytest.mark.parametrize("case, overrides, n, words", [
    ("sim_dp_interp", {}, 1, "not polarized"),
    ("formula_flat", {}, 1, "formula mode"),
    ("slow_interp", {"image_polarization": True}, 1, "slow light"),
    ("sim_polarized_adaptive", {}, 2, "adaptive"),
    ("sim_render", {"image_light": True, "image_polarization": True}, 2, "render_num_images"),
])
def test_refused_configurations(case, overrides, n, words, built_library):
    p, ctx = _host_context(case, **overrides)
    assert _set(ctx, np.ones(n), np.full(n, 20.0), np.geomspace(1.0e-17, 1.0e-16, n)) == BL_E_UNSUPPORTED
    assert "Polarized variants" in _last_error(ctx) and words in _last_error(ctx)
    assert ctx.num_polarized_variants == 0
    ctx.close()


def test_refusal_of_an_unpolarized_context_names_the_other_calls(built_library):
    p, ctx = _host_context("sim_dp_interp")
    assert _set(ctx, [1.0], [20.0], [1.0e-16]) == BL_E_UNSUPPORTED
    assert "bl_set_electron_models" in _last_error(ctx) and "bl_set_density_units" in _last_error(ctx)
    ctx.close()


def test_one_variant_is_allowed_with_adaptive_refinement_and_code_kappa(built_library):
    p, ctx = _host_context("sim_polarized_adaptive")
    assert _set(ctx, [1.0], [20.0], [3.0e-16]) == 0 and ctx.num_polarized_variants == 1
    ctx.close()
    p, ctx = _host_context("sim_polarized", plasma_model="code_kappa")
    assert _set(ctx, [1.0, 1.0], [20.0, 40.0], [3.0e-16, 1.0e-16]) == 0 and ctx.num_polarized_variants == 2
    ctx.close()


def test_the_unpolarized_setters_still_refuse_polarized_runs(built_library):
    p, ctx = _host_context("sim_polarized")
    one = _arr([1.0])
    assert ctx._lib.bl_set_electron_models(ctx._ctx, 1, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == BL_E_UNSUPPORTED
    assert "polarized runs render one electron model" in _last_error(ctx)
    unit = _arr([1.0e-16])
    assert ctx._lib.bl_set_density_units(ctx._ctx, 1, unit.ctypes.data_as(C.c_void_p)) == BL_E_UNSUPPORTED
    assert "polarized runs render one density unit" in _last_error(ctx)
    ctx.close()


def test_host_steps_refuse_several_variants(tmp_path, built_library):
    import blacklight_amd as bl
    p, ctx = _host_context("sim_polarized")
    ctx.set_polarized_variants([10.0, 40.0], [1.0e-17, 1.0e-16])
    n_pix = int(p.get("camera_resolution")) ** 2
    image = np.zeros((ctx.num_quantities, n_pix))
    with pytest.raises(bl.BlacklightError) as err:
        ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))
    assert err.value.code == BL_E_UNSUPPORTED and "variant axis" in str(err.value)
    flags = np.zeros(1, dtype=np.uint8)
    n_refined = C.c_int32(0)
    rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 1, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                     C.byref(n_refined), None)
    assert rc == BL_E_UNSUPPORTED and "polarized variants" in _last_error(ctx)
    ctx.set_polarized_variants([], [])
    image = np.zeros((ctx.num_quantities, n_pix))
    ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))   # (the reference's layout again)
    assert (tmp_path / "out.npz").exists()
    rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 1, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                     C.byref(n_refined), None)
    assert rc == 0
    ctx.close()


def test_stokes_flux_and_net_polarization_by_hand(built_library):
    from blacklight_amd import flux
    p, ctx = _host_context("sim_polarized")
    ctx.close()
    nan = math.nan
    image = np.array([[4.0, 8.0, nan, 6.0], [1.0, nan, 3.0, 2.0], [0.0, 4.0, nan, 2.0], [-1.0, -1.0, -1.0, nan],   # frequency 0
                      [2.0, 2.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0], [-1.0, -1.0, -1.0, -1.0], [0.5, 0.5, 0.5, 0.5]])  # frequency 1
    omega = flux.camera_solid_angle(p, 8.1e3) / 1.0e-23
    i, q, u, v = flux.stokes_flux_jy(image, p, 8.1e3)
    assert (i, q, u, v) == pytest.approx((6.0 * omega, 2.0 * omega, 2.0 * omega, -1.0 * omega), rel=1e-14)   # (each row's own NaN pixels left out)
    assert i == flux.total_flux_jy(image, p, 8.1e3, frequency=0)
    m_net, v_net, evpa = flux.net_polarization((i, q, u, v))
    assert m_net == pytest.approx(math.sqrt(8.0) / 6.0, rel=1e-14) and v_net == pytest.approx(-1.0 / 6.0, rel=1e-14)
    assert evpa == pytest.approx(math.pi / 8.0, rel=1e-14)
    second = flux.stokes_flux_jy(image, p, 8.1e3, frequency=1)
    assert second == pytest.approx((2.0 * omega, 0.0, -1.0 * omega, 0.5 * omega), rel=1e-14)
    assert flux.net_polarization(second) == pytest.approx((0.5, 0.25, -math.pi / 4.0), rel=1e-14)
    with pytest.raises(ValueError):
        flux.stokes_flux_jy(image, p, 8.1e3, frequency=2)


def _stub_render(ctx, p, exponents, rho_ref, flux_ref, distance_pc, calls):
    """A render whose Stokes-I flux is flux_ref R_high (rho / rho_ref)^exponent[R_high] for every variant set (a uniform image), with
    Q = 0.3 I, U = 0.4 I, V = -0.1 I"""
    from blacklight_amd import flux
    per_jy = 1.0 / flux.total_flux_jy(np.ones((1, 4)), p, distance_pc)

    def render():
        variants = ctx.polarized_variants
        assert variants and len(variants) == ctx.num_polarized_variants <= 16
        calls.append(list(variants))
        image = np.empty((len(variants), 4, 4))
        for v, (high, low, rho) in enumerate(variants):
            i_jy = flux_ref * high * (rho / rho_ref) ** exponents[high]
            for s, factor in enumerate((1.0, 0.3, 0.4, -0.1)):
                image[v, s] = factor * i_jy * per_jy
        return dict(image=image.reshape(-1, 4), image_by_variant=image)
    return render


def test_polarized_fit_steps_all_pairs_together(built_library):
    p, ctx = _host_context("sim_polarized")
    calls = []
    exponents = {10.0: 2.0, 40.0: 1.5, 160.0: 0.5}
    ctx.set_polarized_variants(7.0, 5.0e-17)
    ctx.render = _stub_render(ctx, p, exponents, 1.0e-16, 0.01, 8.1e3, calls)
    pairs = [(10.0, 1.0), (40.0, 1.0), (160.0, 1.0)]
    found, renders = ctx.fit_density_units_polarized(pairs, 2.4, 8.1e3, 1.0e-19, 1.0e-13, rtol=1.0e-4)
    assert renders == len(calls) and 2 <= renders <= 6   # (a power law is a line in the logarithms: the first secant step lands)
    assert sorted((h, lo) for h, lo, _ in calls[0]) == sorted(pairs + pairs)   # (the first render: both ends of every pair's bracket)
    assert {rho for _, _, rho in calls[0]} == {1.0e-19, 1.0e-13}
    for later in calls[1:]:   # every later render: one trial per unfinished pair
        assert len({(h, lo) for h, lo, _ in later}) == len(later) <= 3
    for (high, low), (rho, flux_jy, m_net, v_net) in zip(pairs, found):
        assert abs(flux_jy - 2.4) <= 1.0e-4 * 2.4
        assert rho == pytest.approx(1.0e-16 * (2.4 / (0.01 * high)) ** (1.0 / exponents[high]), rel=2.0e-4 / exponents[high])
        assert m_net == pytest.approx(0.5, rel=1e-12) and v_net == pytest.approx(-0.1, rel=1e-12)
    assert ctx.polarized_variants == [(7.0, 1.0, 5.0e-17)] and ctx.num_polarized_variants == 1   # (restored)
    ctx.close()


def test_polarized_fit_splits_more_than_sixteen_trials(built_library):
    p, ctx = _host_context("sim_polarized")
    calls = []
    highs = [float(h) for h in range(1, 11)]   # ten pairs: twenty bracket ends
    ctx.render = _stub_render(ctx, p, {h: 1.0 for h in highs}, 1.0e-16, 0.01, 8.1e3, calls)
    found, renders = ctx.fit_density_units_polarized([(h, 1.0) for h in highs], 1.0, 8.1e3, 1.0e-18, 1.0e-12, rtol=1.0e-3)
    assert [len(c) for c in calls[:2]] == [16, 4] and renders == len(calls)
    for h, (rho, flux_jy, _, _) in zip(highs, found):
        assert abs(flux_jy - 1.0) <= 1.0e-3 and rho == pytest.approx(1.0e-14 / h, rel=2.0e-3)
    assert ctx.num_polarized_variants == 0   # (restored: none were set)
    ctx.close()


def test_polarized_fit_raises_on_an_unbracketed_target(built_library):
    p, ctx = _host_context("sim_polarized")
    calls = []
    ctx.render = _stub_render(ctx, p, {10.0: 1.0}, 1.0e-16, 0.05, 8.1e3, calls)
    with pytest.raises(ValueError, match="does not bracket"):
        ctx.fit_density_units_polarized([(10.0, 1.0)], 100.0, 8.1e3, 1.0e-17, 1.0e-15)
    assert len(calls) == 1 and ctx.num_polarized_variants == 0
    ctx.close()
