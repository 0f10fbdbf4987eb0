"""Density units (bl_set_density_units) on host-only contexts (no GPU): argument validation, what is refused and why, the image row
count with and without electron models, the host steps that read one image, the total flux of an image and the flux fit's search
(against a stub render)."""
import ctypes as C
import math

import numpy as np
import pytest

import golden_util as gu

BL_DEVICE_NONE = -2
BL_E_UNSUPPORTED = 3
BL_E_ARG = 5


def _host_context(case, **overrides):
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case(case)
    params = dict(params, **overrides)
    p = bl.Params.from_dict(params)
    return p, bl.Context(p, device=BL_DEVICE_NONE)


def _set(ctx, units, n=None):
    units = np.ascontiguousarray(units, dtype=np.float64)
    n = units.size if n is None else n
    return ctx._lib.bl_set_density_units(ctx._ctx, n, units.ctypes.data_as(C.c_void_p))


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode()


def test_units_scale_the_image_rows(built_library):
    p, ctx = _host_context("sim_multifreq")
    n_q = ctx.num_quantities
    assert ctx.num_density_units == 0 and ctx.density_units == []
    ctx.set_density_units([1.0e-17, 1.0e-16, 1.0e-15])
    assert ctx.num_density_units == 3 and ctx.num_quantities == 3 * n_q
    assert ctx.density_units == [1.0e-17, 1.0e-16, 1.0e-15]
    ctx.set_electron_models([10.0, 40.0])                 # models x units, model-major
    assert ctx.num_quantities == 2 * 3 * n_q
    ctx.set_density_units(2.0e-16)                       # n = 1: one unit instead of the parameter block's, same rows
    assert ctx.num_density_units == 1 and ctx.num_quantities == 2 * n_q
    ctx.set_electron_models([])
    assert ctx.num_quantities == n_q
    ctx.set_density_units([])
    assert ctx.num_density_units == 0 and ctx.num_quantities == n_q
    ctx.close()


def test_bad_arguments(built_library):
    p, ctx = _host_context("sim_dp_interp")
    lib = ctx._lib
    assert _set(ctx, np.full(17, 1.0e-16)) == BL_E_ARG
    assert "16" in _last_error(ctx)
    assert _set(ctx, [1.0e-16], n=-1) == BL_E_ARG
    for bad in (math.nan, math.inf, 0.0, -1.0e-16):
        assert _set(ctx, [1.0e-16, bad]) == BL_E_ARG, bad
        assert "finite value > 0" in _last_error(ctx)
    assert lib.bl_set_density_units(ctx._ctx, 2, None) == BL_E_ARG
    assert lib.bl_set_density_units(None, 0, None) == BL_E_ARG
    assert lib.bl_num_density_units(None) == -1
    assert ctx.num_density_units == 0   # (nothing was set by a refused call)
    assert lib.bl_set_density_units(ctx._ctx, 0, None) == 0
    assert _set(ctx, np.geomspace(1.0e-18, 1.0e-14, 16)) == 0
    assert ctx.num_density_units == 16
    ctx.close()


@pytest.mark.parametrize("case, overrides, n, words", [
    ("formula_flat", {}, 1, "formula mode"),
    ("sim_polarized", {}, 1, "polarized"),
    ("slow_interp", {}, 1, "slow light"),
    ("sim_adaptive", {}, 2, "adaptive"),
    ("sim_render", {}, 2, "rho"),                                                       # a rendering reads rho
    ("sim_render", {"render_1_1_quantity": "B"}, 2, "B"),                               # ... or B
    ("sim_render", {"render_1_1_quantity": "sigma", "cut_rho_min": 1.0e-19}, 2, "cut"),   # a rho cut decides what a rendering sees
])
def test_refused_configurations(case, overrides, n, words, built_library):
    p, ctx = _host_context(case, **overrides)
    assert _set(ctx, np.geomspace(1.0e-17, 1.0e-16, n)) == BL_E_UNSUPPORTED
    assert "Density units" in _last_error(ctx) and words in _last_error(ctx)
    assert ctx.num_density_units == 0
    ctx.close()


def test_one_unit_is_allowed_with_adaptive_refinement(built_library):
    p, ctx = _host_context("sim_adaptive")
    assert _set(ctx, [3.0e-16]) == 0
    assert ctx.num_density_units == 1
    ctx.close()


def test_renderings_no_unit_enters_are_allowed(built_library):
    p, ctx = _host_context("sim_render", render_1_1_quantity="sigma")   # sigma and 1 / beta only (and a sigma cut)
    assert _set(ctx, [1.0e-17, 1.0e-16]) == 0
    assert ctx.num_density_units == 2
    ctx.close()


def test_host_steps_refuse_several_units(tmp_path, built_library):
    import blacklight_amd as bl
    p, ctx = _host_context("sim_dp_interp")
    ctx.set_density_units([1.0e-17, 1.0e-16])
    n_pix = int(p.get("camera_resolution")) ** 2
    image = np.zeros((ctx.num_quantities, n_pix))
    with pytest.raises(bl.BlacklightError) as err:
        ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))
    assert err.value.code == BL_E_UNSUPPORTED and "density-unit" in str(err.value)
    flags = np.zeros(1, dtype=np.uint8)
    n_refined = C.c_int32(0)
    rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 1, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                     C.byref(n_refined), None)
    assert rc == BL_E_UNSUPPORTED and "density units" in _last_error(ctx)
    ctx.set_density_units([])
    image = np.zeros((ctx.num_quantities, n_pix))
    ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))   # (the reference's layout again)
    assert (tmp_path / "out.npz").exists()
    rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 1, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                     C.byref(n_refined), None)
    assert rc == 0
    ctx.close()


def test_total_flux_by_hand(built_library):
    from blacklight_amd import flux
    p, ctx = _host_context("sim_dp_interp")
    ctx.close()
    image = np.array([[1.0e-3, 3.0e-3, math.nan, 2.0e-3], [7.0, 7.0, 7.0, 7.0]])
    # by hand: 24 r_g of a 4.152e6 M_sun hole seen from 8.1 kpc, the mean of the three pixels that are not NaN
    c, g_msun, pc = 2.99792458e10, 1.32712440018e26, 9.69394202136e18 / math.pi
    r_g = g_msun * 4.152e6 / c ** 2
    w = 2.0 * math.atan(12.0 * r_g / (8.1e3 * pc))
    want = 2.0e-3 * w * w / 1.0e-23
    assert flux.total_flux_jy(image, p, 8.1e3) == pytest.approx(want, rel=1e-14)
    assert flux.total_flux_jy(image, p, 8.1e3, frequency=1) == pytest.approx(7.0 * w * w / 1.0e-23, rel=1e-14)
    assert flux.total_flux_jy(image[0], p, 8.1e3) == pytest.approx(want, rel=1e-14)


def _stub_render(ctx, p, exponent, rho_ref, flux_ref, distance_pc, calls):
    """A render whose total flux is flux_ref (rho / rho_ref)^exponent for every unit and model set (a uniform image)"""
    from blacklight_amd import flux
    per_jy = 1.0 / flux.total_flux_jy(np.ones((1, 4)), p, distance_pc)

    def render():
        units = ctx.density_units or [float(p.get("simulation_rho_cgs"))]
        n_models = max(1, ctx.num_electron_models)
        calls.append((list(units), ctx.electron_models))
        image = np.empty((n_models, len(units), 1, 4))
        for m in range(n_models):
            high = ctx.electron_models[m][0] if ctx.electron_models else 1.0
            for u, rho in enumerate(units):
                image[m, u] = flux_ref * high * (rho / rho_ref) ** exponent * per_jy
        return dict(image=image.reshape(-1, 4), image_by_unit=image)
    return render


@pytest.mark.parametrize("exponent", [0.5, 2.0, -1.5])
def test_fit_converges_on_a_power_law(exponent, built_library):
    p, ctx = _host_context("sim_dp_interp")
    calls = []
    ctx.set_density_units([5.0e-17])
    ctx.render = _stub_render(ctx, p, exponent, 1.0e-16, 0.5, 8.1e3, calls)
    rho, got, renders = ctx.fit_density_unit(0.8, 8.1e3, 1.0e-19, 1.0e-13, rtol=1.0e-4)
    assert abs(got - 0.8) <= 1.0e-4 * 0.8
    assert rho == pytest.approx(1.0e-16 * 1.6 ** (1.0 / exponent), rel=2.0e-4 / abs(exponent))
    assert renders == len(calls) and 2 <= renders <= 8
    assert all(len(units) == 16 for units, _ in calls)   # (per_render units in each render)
    assert ctx.density_units == [5.0e-17] and ctx.num_density_units == 1   # (restored)
    ctx.close()


def test_fit_per_model_and_restores(built_library):
    p, ctx = _host_context("sim_dp_interp")
    calls = []
    ctx.set_electron_models([10.0, 40.0])
    ctx.render = _stub_render(ctx, p, 1.0, 1.0e-16, 0.1, 8.1e3, calls)
    rho, got, renders = ctx.fit_density_unit(2.0, 8.1e3, 1.0e-18, 1.0e-14, rtol=1.0e-3, per_render=8)
    assert len(rho) == len(got) == 2
    for high, r, f in zip((10.0, 40.0), rho, got):
        assert abs(f - 2.0) <= 2.0e-3 and r == pytest.approx(1.0e-16 * 2.0 / (0.1 * high), rel=2.0e-3)
    assert all(len(models) == 1 for _, models in calls)   # (one model per render)
    assert ctx.electron_models == [(10.0, 1.0), (40.0, 1.0)] and ctx.num_electron_models == 2
    assert ctx.density_units == [] and ctx.num_density_units == 0
    ctx.close()


def test_fit_raises_on_an_unbracketed_target(built_library):
    p, ctx = _host_context("sim_dp_interp")
    calls = []
    ctx.render = _stub_render(ctx, p, 1.0, 1.0e-16, 0.5, 8.1e3, calls)
    with pytest.raises(ValueError, match="does not bracket") as err:
        ctx.fit_density_unit(100.0, 8.1e3, 1.0e-17, 1.0e-15)
    assert "0.05" in str(err.value) and "5 Jy" in str(err.value)   # (the flux range it found)
    assert len(calls) == 1 and ctx.density_units == [] and ctx.num_density_units == 0
    ctx.close()
