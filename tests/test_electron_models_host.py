"""Electron-temperature models (bl_set_electron_models) on host-only contexts (no GPU): argument validation, what is refused and
why, the image row count, and the host steps that read one image (bl_adaptive_refine, bl_write_output)."""
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


def _set(ctx, rat_low, rat_high, n=None):
    low = np.ascontiguousarray(rat_low, dtype=np.float64)
    high = np.ascontiguousarray(rat_high, dtype=np.float64)
    n = low.size if n is None else n
    return ctx._lib.bl_set_electron_models(ctx._ctx, n, low.ctypes.data_as(C.c_void_p), high.ctypes.data_as(C.c_void_p))


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode()


def test_models_scale_the_image_rows(built_library):
    p, ctx = _host_context("sim_multifreq")
    n_q = ctx.num_quantities
    assert ctx.num_electron_models == 0 and ctx.electron_models == []
    ctx.set_electron_models([1.0, 10.0, 40.0, 160.0])
    assert ctx.num_electron_models == 4
    assert ctx.num_quantities == 4 * n_q
    assert ctx.electron_models == [(1.0, 1.0), (10.0, 1.0), (40.0, 1.0), (160.0, 1.0)]
    ctx.set_electron_models(20.0, rat_low=[1.0, 2.0])   # (broadcast)
    assert ctx.electron_models == [(20.0, 1.0), (20.0, 2.0)]
    assert ctx.num_quantities == 2 * n_q
    ctx.set_electron_models(7.0)                         # n = 1: one pair instead of the parameter block's, same rows
    assert ctx.num_electron_models == 1 and ctx.num_quantities == n_q
    ctx.set_electron_models([])
    assert ctx.num_electron_models == 0 and ctx.num_quantities == n_q
    ctx.close()


def test_bad_arguments(built_library):
    p, ctx = _host_context("sim_dp_interp")
    lib = ctx._lib
    assert _set(ctx, np.ones(17), np.ones(17)) == BL_E_ARG
    assert "16" in _last_error(ctx)
    assert _set(ctx, [1.0], [1.0], n=-1) == BL_E_ARG
    assert _set(ctx, [1.0, math.nan], [1.0, 10.0]) == BL_E_ARG
    assert "not finite" in _last_error(ctx)
    assert _set(ctx, [1.0], [math.inf]) == BL_E_ARG
    assert lib.bl_set_electron_models(ctx._ctx, 2, None, None) == BL_E_ARG
    assert lib.bl_set_electron_models(None, 0, None, None) == BL_E_ARG
    assert ctx.num_electron_models == 0   # (nothing was set by a refused call)
    assert lib.bl_set_electron_models(ctx._ctx, 0, None, None) == 0
    assert _set(ctx, np.ones(16), np.arange(1.0, 17.0)) == 0
    assert ctx.num_electron_models == 16
    ctx.close()


@pytest.mark.parametrize("case, overrides, n, words", [
    ("formula_flat", {}, 1, "formula mode"),
    ("sim_polarized", {}, 1, "polarized"),
    ("sim_code_kappa", {}, 1, "code_kappa"),
    ("slow_interp", {}, 1, "slow light"),
    ("sim_adaptive", {}, 2, "adaptive"),
    ("sim_render_light", {}, 2, "Theta_e"),                            # a rendering reads Theta_e
    ("sim_render", {"cut_theta_e_min": 1.0}, 2, "Theta_e"),           # a Theta_e cut decides which cells a rendering sees
])
def test_refused_configurations(case, overrides, n, words, built_library):
    p, ctx = _host_context(case, **overrides)
    assert _set(ctx, np.ones(n), np.linspace(1.0, 10.0, n)) == BL_E_UNSUPPORTED
    assert words in _last_error(ctx)
    assert ctx.num_electron_models == 0
    ctx.close()


@pytest.mark.parametrize("case", ["sim_adaptive", "sim_render_light"])
def test_one_model_is_always_allowed(case, built_library):
    p, ctx = _host_context(case)
    assert _set(ctx, [1.0], [40.0]) == 0
    assert ctx.num_electron_models == 1
    ctx.close()


def test_renderings_no_model_enters_are_allowed(built_library):
    p, ctx = _host_context("sim_render")
    assert _set(ctx, [1.0, 1.0], [10.0, 40.0]) == 0
    ctx.close()


def test_host_steps_refuse_several_models(tmp_path, built_library):
    import blacklight_amd as bl
    p, ctx = _host_context("sim_dp_interp")
    ctx.set_electron_models([1.0, 10.0])
    n_pix = int(p.get("camera_resolution")) ** 2
    image = np.zeros((ctx.num_quantities, n_pix))
    with pytest.raises(bl.BlacklightError) as err:
        ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))
    assert err.value.code == BL_E_UNSUPPORTED and "electron-model" in str(err.value)
    flags = np.zeros(1, dtype=np.uint8)
    n_refined = C.c_int32(0)
    rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 1, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                     C.byref(n_refined), None)
    assert rc == BL_E_UNSUPPORTED and "one image" in _last_error(ctx)
    ctx.set_electron_models([])
    image = np.zeros((ctx.num_quantities, n_pix))
    ctx.write_output([dict(image=image)], path=str(tmp_path / "out.npz"))   # (the reference's layout again)
    assert (tmp_path / "out.npz").exists()
    ctx.close()
