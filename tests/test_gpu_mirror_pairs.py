"""GPU: one ray traced per mirror pair (bl_stats.mirror_pairs) against every ray traced (BL_SWITCH_NO_MIRROR_PAIRS).

With zero spin and the camera in the plane phi = 0 - no roll, no azimuthal velocity - pixel (row, res - 1 - col) starts as the mirror
image in y = 0 of pixel (row, col), and the zero-spin Dormand-Prince stepper keeps it so bit for bit. A paired render traces the left half
of the frame and shades every sample record twice: as it is, and with the sign bits of y and k_y flipped for the mirror pixel. Nothing
downstream is shared - the mirrored sample reads other cells - so the plasma here is modulated in phi: a frame assembled by copying the
left half would fail every comparison below (the guard in _pair asserts that the unpaired frame is not symmetric).

Every case compares a render with its twin under the switch ("off"): the exact tier and the reproducible tolerant tier bit for bit,
composed maps to the 1e-10 per pixel the project asserts between tiers. The cameras and variants the plan must leave unpaired render
with mirror_pairs == 0 and off's outputs."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_GRIDS = {}
_RENDERS = {}


def _grid(n_r=32, n_th=32, n_ph=64):
    """The mock with rho and p multiplied by 1 + 0.3 sin(phi + 0.7): nothing about it is symmetric in y."""
    key = (n_r, n_th, n_ph)
    if key not in _GRIDS:
        from blacklight_amd import mock
        grid = mock.generate(n_r=n_r, n_th=n_th, n_ph=n_ph)
        prim = grid.prim.copy()
        phi = np.asarray(grid.x3v, dtype=np.float64).reshape(-1)
        prim[0:2] *= (1.0 + 0.3 * np.sin(phi + 0.7)).astype(np.float32)[None, None, :, None, None]
        _GRIDS[key] = dataclasses.replace(grid, prim=np.ascontiguousarray(prim))
    return _GRIDS[key]


def _params(**overrides):
    import bench
    return dict(bench.WORKLOAD, camera_resolution=64, **overrides)


def _render(pairs, tier="exact", reproducible=False, flat=False, grid=None, pixel_map=None, guard_band=None, **overrides):
    """One render (kept: a reference is rendered once and shared, and nobody writes to it)."""
    key = (pairs, tier, reproducible, flat, id(grid) if grid is not None else 0, pixel_map is not None, guard_band, tuple(sorted(overrides.items())))
    if key in _RENDERS:
        return _RENDERS[key]
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(_params(**overrides))) as ctx:
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        ctx.debug_set_switches(*((["FLAT_ORDER"] if flat else []) + ([] if pairs else ["NO_MIRROR_PAIRS"])))
        if guard_band is not None:
            ctx.debug_set_guard_band(guard_band)
        ctx.set_grid(grid if grid is not None else _grid())
        out = ctx.render(pixel_map=pixel_map)
        out["stats"] = ctx.stats
    _RENDERS[key] = out
    return out


def _same_counts(on, off):
    assert np.array_equal(on["sample_num"], off["sample_num"])
    assert np.array_equal(on["sample_flags"], off["sample_flags"])
    a, b = on["stats"], off["stats"]
    assert (a.n_rays, a.n_samples, a.n_gathers, a.n_flagged, a.max_sample_num) == (b.n_rays, b.n_samples, b.n_gathers, b.n_flagged, b.max_sample_num)
    assert a.launches_geodesic == a.launches_shade == a.launches_transfer == a.n_chunks == 1
    assert (b.launches_geodesic, b.launches_shade, b.launches_transfer, b.n_chunks) == (1, 1, 1, 1)
    assert a.xcd_order == b.xcd_order and a.local_angles == b.local_angles and a.algorithmic_bytes == b.algorithmic_bytes


def _same_bits(on, off):
    assert np.array_equal(on["image"].view(np.int64), off["image"].view(np.int64))


def _pair(tier="exact", reproducible=False, flat=False, paired=1, guard=True, **overrides):
    on = _render(True, tier, reproducible, flat, **overrides)
    off = _render(False, tier, reproducible, flat, **overrides)
    assert on["stats"].mirror_pairs == paired and off["stats"].mirror_pairs == 0
    import blacklight_amd._capi as _capi
    assert off["stats"].switches & _capi.SWITCHES["NO_MIRROR_PAIRS"] and not on["stats"].switches & _capi.SWITCHES["NO_MIRROR_PAIRS"]
    res = int(round(np.sqrt(off["image"].shape[-1])))
    frame = off["image"].reshape(-1, res, res)
    # the guard: the unpaired frame's left half is NOT its flipped right half (a copied frame could not pass)
    assert not guard or not np.array_equal(np.nan_to_num(frame[..., : res // 2]), np.nan_to_num(frame[..., : res // 2 - 1 : -1]))
    _same_counts(on, off)
    return on, off


# ---------------------------------------------------------------------------------------------------------------- cases 1 - 4
@pytest.mark.parametrize("flat", [False, True])
def test_exact_tier_is_the_unpaired_frame_bit_for_bit(flat):
    on, off = _pair("exact", flat=flat)
    _same_bits(on, off)
    assert on["stats"].fused_variant == 3


def test_samples_emitted_count_the_whole_frame():
    """n_samples_emitted counts the records the stepper wrote - twice for a paired render, whose every record stands for two - not the
    record slots its waves took (those include each wave's partly filled last block and differ from launch to launch): the paired and
    the unpaired render report the same number, and no fewer than the samples kept."""
    on, off = _pair("exact")
    print("n_samples_emitted: paired", on["stats"].n_samples_emitted, "unpaired", off["stats"].n_samples_emitted)
    assert on["stats"].n_samples_emitted == off["stats"].n_samples_emitted
    assert on["stats"].n_samples_emitted >= on["stats"].n_samples > 0


@pytest.mark.parametrize("flat", [False, True])
def test_reproducible_tolerant_tier_is_the_unpaired_frame_bit_for_bit(flat):
    on, off = _pair("tolerant", reproducible=True, flat=flat)
    _same_bits(on, off)
    assert on["stats"].fused_variant == 2 and on["stats"].composed_maps == 0
    # (the exact second pass ran over listed records of both halves: their index decode, sign flips and rows)
    assert on["stats"].n_deferred == off["stats"].n_deferred and on["stats"].n_deferred > 0


@pytest.mark.parametrize("reproducible", [True, False])
def test_exact_second_pass_over_every_record_when_its_list_overflows(reproducible):
    """A guard band of 0.5 leaves more samples to the exact pass than its list of 2^20 entries holds: that pass then walks every record
    of both halves - per-sample rows (reproducible) and rows by record index behind composed maps."""
    on = _render(True, "tolerant", reproducible=reproducible, guard_band=0.5)
    off = _render(False, "tolerant", reproducible=reproducible, guard_band=0.5)
    assert on["stats"].mirror_pairs == 1 and off["stats"].mirror_pairs == 0
    print("guard band 0.5: deferred", on["stats"].n_deferred, off["stats"].n_deferred, "of", on["stats"].n_samples_emitted)
    assert on["stats"].n_deferred == off["stats"].n_deferred and on["stats"].n_deferred > (1 << 20)
    _same_counts(on, off)
    if reproducible:
        _same_bits(on, off)
    else:
        both = np.isfinite(off["image"])
        assert np.array_equal(np.isfinite(on["image"]), both) and np.array_equal(np.isnan(on["image"]), np.isnan(off["image"]))
        assert np.allclose(on["image"][both], off["image"][both], rtol=1.0e-10, atol=0.0)


@pytest.mark.parametrize("flat", [False, True])
def test_composed_maps_agree_with_the_exact_tier_per_pixel(flat):
    on, off = _pair("tolerant", flat=flat)
    exact = _render(True, "exact", flat=flat)
    assert on["stats"].composed_maps == 1 and on["stats"].xcd_order == (0 if flat else 1)
    assert on["stats"].n_deferred == off["stats"].n_deferred
    assert np.array_equal(on["sample_num"], exact["sample_num"]) and np.array_equal(on["sample_flags"], exact["sample_flags"])
    a, b = on["image"], exact["image"]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a), np.isnan(off["image"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        worst = np.nanmax(np.where(b != 0.0, np.abs(a - b) / scale, np.abs(a - b)))
    print("composed maps, paired vs exact tier: worst relative difference per pixel", worst)
    assert worst <= 1.0e-10


# ---------------------------------------------------------------------------------------------------------------- case 5
def test_optically_thick_steps_write_expanded_rows_for_both_halves():
    for reproducible in (True, False):
        on, off = _pair("tolerant", reproducible=reproducible, image_frequency=5.0e9)
        if reproducible:
            _same_bits(on, off)
        else:
            both = np.isfinite(off["image"])
            assert np.array_equal(np.isfinite(on["image"]), both)
            assert np.allclose(on["image"][both], off["image"][both], rtol=1.0e-10, atol=0.0)


def test_polar_axis_camera_leaves_the_exact_pass_its_samples_in_both_halves():
    on = _render(True, "tolerant", reproducible=True, camera_th=0.0)
    off = _render(False, "tolerant", reproducible=True, camera_th=0.0)
    print("camera_th = 0: mirror_pairs", on["stats"].mirror_pairs, "deferred", on["stats"].n_deferred, off["stats"].n_deferred)
    assert off["stats"].mirror_pairs == 0
    _same_counts(on, off)
    assert on["stats"].n_deferred == off["stats"].n_deferred and on["stats"].n_deferred > 0
    _same_bits(on, off)


def test_flagged_rays_are_flagged_in_both_halves():
    # (sixty steps end no ray of this camera: every pixel is flagged and NaN, so the guard has nothing to tell apart here)
    on, off = _pair("tolerant", reproducible=True, guard=False, ray_max_steps=60)
    assert off["stats"].n_flagged > 0 and np.isnan(off["image"]).any()
    _same_bits(on, off)


# ---------------------------------------------------------------------------------------------------------------- case 6
def test_series_shades_the_resident_half_for_both_halves():
    import blacklight_amd as bl
    first = _grid()
    prim = first.prim.copy()
    prim[0:2] *= np.float32(1.07)
    second = dataclasses.replace(first, prim=prim)
    frames = {}
    for pairs in (True, False):
        with bl.Context(bl.Params.from_dict(_params())) as ctx:
            ctx.set_arithmetic("exact")
            ctx.set_geodesic_reuse(True)
            ctx.debug_set_switches(*([] if pairs else ["NO_MIRROR_PAIRS"]))
            for grid in (first, second):
                ctx.set_grid(grid)
                out = ctx.render()
                out["stats"] = ctx.stats
            frames[pairs] = out
    on, off = frames[True], frames[False]
    assert on["stats"].mirror_pairs == 1 and off["stats"].mirror_pairs == 0
    for out in (on, off):
        assert out["stats"].geodesics_reused == 1 and out["stats"].launches_geodesic == 0
    assert np.array_equal(on["sample_num"], off["sample_num"]) and np.array_equal(on["sample_flags"], off["sample_flags"])
    assert on["stats"].n_samples == off["stats"].n_samples and on["stats"].n_gathers == off["stats"].n_gathers
    _same_bits(on, off)
    assert not np.array_equal(on["image"], _render(True, "exact")["image"])   # (the second snapshot's frame, not the first's)


# ---------------------------------------------------------------------------------------------------------------- case 7
@pytest.mark.parametrize("overrides", [dict(simulation_a=0.5), dict(camera_ph=30.0), dict(camera_rotation=20.0), dict(camera_uphn=0.1),
                                       dict(camera_resolution=72),
                                       dict(image_num_frequencies=4, image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log"),
                                       dict(image_polarization=True)],
                         ids=lambda o: next(iter(o)))
def test_everything_else_is_not_paired(overrides):
    for tier in ("exact", "tolerant"):
        params = dict(overrides)
        res = params.pop("camera_resolution", None)
        import blacklight_amd as bl
        outs = []
        for pairs in (True, False):
            full = _params(**params)
            if res is not None:
                full["camera_resolution"] = res
            with bl.Context(bl.Params.from_dict(full)) as ctx:
                ctx.set_arithmetic(tier)
                ctx.set_reproducible(True)
                ctx.debug_set_switches(*([] if pairs else ["NO_MIRROR_PAIRS"]))
                ctx.set_grid(_grid())
                out = ctx.render()
                out["stats"] = ctx.stats
            outs.append(out)
        on, off = outs
        assert on["stats"].mirror_pairs == 0 and off["stats"].mirror_pairs == 0, tier
        assert np.array_equal(on["sample_num"], off["sample_num"]) and np.array_equal(on["sample_flags"], off["sample_flags"])
        assert on["stats"].n_samples == off["stats"].n_samples
        _same_bits(on, off)


def test_a_pixel_map_of_the_left_half_is_not_paired():
    res = 64
    left = (np.arange(res)[:, None] * res + np.arange(res // 2)[None, :]).reshape(-1).astype(np.int32)
    for tier in ("exact", "tolerant"):
        on = _render(True, tier, reproducible=True, pixel_map=left)
        off = _render(False, tier, reproducible=True, pixel_map=left)
        whole = _render(False, tier, reproducible=True)
        assert on["stats"].mirror_pairs == 0 and off["stats"].mirror_pairs == 0
        assert np.array_equal(on["sample_num"], off["sample_num"]) and np.array_equal(on["sample_num"], whole["sample_num"][left])
        _same_bits(on, off)
        assert np.array_equal(on["image"].view(np.int64), whole["image"][:, left].view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- case 8
@pytest.mark.parametrize("res", [32, 128])
def test_one_and_several_super_tiles_per_half(res):
    """32 x 32: half a super-tile per half; 128 x 128: a whole one and more. Over the 32^3 mock."""
    grid = _grid(32, 32, 32)
    import blacklight_amd as bl
    outs = []
    for pairs in (True, False):
        with bl.Context(bl.Params.from_dict(dict(_params(), camera_resolution=res))) as ctx:
            ctx.set_arithmetic("exact")
            ctx.debug_set_switches(*([] if pairs else ["NO_MIRROR_PAIRS"]))
            ctx.set_grid(grid)
            out = ctx.render()
            out["stats"] = ctx.stats
        outs.append(out)
    on, off = outs
    assert on["stats"].mirror_pairs == 1 and off["stats"].mirror_pairs == 0
    _same_counts(on, off)
    _same_bits(on, off)
    # ... and the tolerant tier's list walk over several lists
    outs = []
    for pairs in (True, False):
        with bl.Context(bl.Params.from_dict(dict(_params(), camera_resolution=res))) as ctx:
            ctx.set_arithmetic("tolerant")
            ctx.set_reproducible(True)
            ctx.debug_set_switches(*([] if pairs else ["NO_MIRROR_PAIRS"]))
            ctx.set_grid(grid)
            out = ctx.render()
            out["stats"] = ctx.stats
        outs.append(out)
    on, off = outs
    assert on["stats"].mirror_pairs == 1 and on["stats"].xcd_order == 1
    _same_counts(on, off)
    _same_bits(on, off)
