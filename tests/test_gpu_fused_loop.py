"""GPU: the forms of bl_shade_fused2_kernel's loop that a render chooses between must give the same frames.

Cut block (fused2::cut_selection): one upper threshold on sigma takes a short form - the threshold and its band alone - and every other
set of active thresholds the general block; BL_SWITCH_GENERAL_CUTS forces the general block. For each set of cuts below the default
frame and the switch's are the same bits under bl_set_reproducible (image, sample_num, flags, samples left to the exact pass), and
both agree with the exact tier per pixel within the tolerant tier's 1e-10 of the pixel's own value, NaN for NaN. The thresholds were
chosen on the CPU oracle so that each cut alone takes about half of the frame's flux away; test_the_cuts_remove_a_share_of_the_flux
holds them to "neither nothing nor everything" on a 16^2 frame, without a GPU.

Segment scan (composed maps): the default frame against the bl_set_reproducible frame
of the same render, 1e-12 per pixel, at 64^2 and over a 72 x 72 window of a 96^2 camera (5 184 rays: the last wave is part full, rays
end anywhere in a row of sixteen lanes); bl_stats says that maps were composed and that samples went to the exact pass, whose rows
keep their samples' own records.

Spin: one frame at a = 0.9 (a spinning instantiation) against the exact tier.

Frames: 64^2 plane camera over the 64 x 64 x 128 mock, as tests/test_gpu_local_angles.py."""
import os
import sys

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu
import oracle_api

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PER_PIXEL = 1.0e-10   # the fused kernel against the exact tier: per pixel, relative to the pixel's own value (tests/test_gpu_cuts_each.py imports it)
NO_CUT = dict(cut_sigma_max=-1.0)
CUTS = {
    "none": dict(NO_CUT),
    "sigma_max": dict(cut_sigma_max=0.0033),
    "sigma_min_max": dict(cut_sigma_min=0.0025, cut_sigma_max=0.0045),
    "rho_min": dict(NO_CUT, cut_rho_min=3.4e-17),
    "theta_e_max": dict(NO_CUT, cut_theta_e_max=4.2),
    "b_min": dict(NO_CUT, cut_b_min=39.0),
    "all_seven": dict(cut_rho_min=2.5e-17, cut_n_e_min=1.2e7, cut_p_gas_max=1200.0, cut_theta_e_max=6.0, cut_b_min=30.0, cut_sigma_max=0.005,
                      cut_beta_inverse_max=0.1),
}


@pytest.fixture(scope="module")
def frame_grid():
    from blacklight_amd import mock
    return mock.generate(n_r=64, n_th=64, n_ph=128)


def _render(grid, overrides, tier="tolerant", reproducible=True, switch=None, resolution=64, pixel_map=None):
    import blacklight_amd as bl
    import bench
    params = dict(bench.WORKLOAD, camera_resolution=resolution, **overrides)
    with bl.Context(bl.Params.from_dict(params)) as c:
        c.set_arithmetic(tier)
        c.set_reproducible(reproducible)
        if switch is not None:
            c.debug_set_switches(switch)
        c.set_grid(grid)
        out = c.render(pixel_map=pixel_map) if pixel_map is not None else c.render()
        out["stats"] = c.stats
    return out


_exact = {}


def _exact_frame(grid, name, overrides):
    if name not in _exact:
        _exact[name] = _render(grid, overrides, "exact")
    return _exact[name]


def _relative_per_pixel(got, want):
    a, b = got["image"], want["image"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b)
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        return float(np.nanmax(np.where(b != 0.0, err / scale, err)))


def _same_rays(got, want):
    assert np.array_equal(got["sample_num"], want["sample_num"])
    assert np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["stats"].n_samples == want["stats"].n_samples


def _oracle_flux(grid, overrides):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import bench
    p = bl.Params.from_dict(dict(bench.WORKLOAD, camera_resolution=16, **overrides))
    out = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=256, num_threads=4)
    return float(np.nansum(out["image"][0]))


def test_the_cuts_remove_a_share_of_the_flux(built_library, frame_grid):
    whole = _oracle_flux(frame_grid, CUTS["none"])
    assert whole > 0.0
    for name, cuts in CUTS.items():
        if name == "none":
            continue
        share = _oracle_flux(frame_grid, cuts) / whole
        print(f"{name}: {share:.3f} of the flux left")
        assert 0.05 <= share <= 0.95, (name, share)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CUTS))
def test_cut_forms_give_the_same_frame(frame_grid, name):
    from blacklight_amd import _capi
    cuts = CUTS[name]
    exact = _exact_frame(frame_grid, name, cuts)
    default = _render(frame_grid, cuts)
    general = _render(frame_grid, cuts, switch="GENERAL_CUTS")
    assert default["stats"].fused_variant == 2 and general["stats"].fused_variant == 2
    assert default["stats"].switches == 0 and general["stats"].switches == _capi.SWITCHES["GENERAL_CUTS"]
    assert default["stats"].composed_maps == 0 and general["stats"].composed_maps == 0
    print(f"{name}: default vs exact {_relative_per_pixel(default, exact):.2e}, general vs exact {_relative_per_pixel(general, exact):.2e}, "
          f"deferred {default['stats'].n_deferred} / {general['stats'].n_deferred} of {default['stats'].n_samples}")
    _same_rays(default, general)
    assert default["stats"].n_deferred == general["stats"].n_deferred
    assert default["stats"].n_gathers == general["stats"].n_gathers
    assert gu.same_bits(default["image"], general["image"]).all()
    for tolerant in (default, general):
        _same_rays(tolerant, exact)
        assert _relative_per_pixel(tolerant, exact) <= PER_PIXEL
    if name != "none":   # (the cut is seen: the frame is not the frame without it)
        assert not gu.same_bits(exact["image"], _exact_frame(frame_grid, "none", CUTS["none"])["image"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, 72])
def test_composed_maps_match_the_records(frame_grid, window):
    cuts = CUTS["sigma_max"]
    resolution, pixels = 64, None
    if window is not None:
        resolution = 96
        iv, iu = np.mgrid[0:window, 0:window]
        pixels = ((iv + 12) * resolution + (iu + 12)).reshape(-1).astype(np.int32)
    composed = _render(frame_grid, cuts, reproducible=False, resolution=resolution, pixel_map=pixels)
    records = _render(frame_grid, cuts, reproducible=True, resolution=resolution, pixel_map=pixels)
    assert composed["stats"].fused_variant == 2 and records["stats"].fused_variant == 2
    assert composed["stats"].composed_maps == 1 and records["stats"].composed_maps == 0
    assert composed["stats"].n_deferred > 0   # (rows of sixteen lanes that hold one keep their samples' own records)
    assert composed["image"].shape[-1] == (window or 64) ** 2
    _same_rays(composed, records)
    assert composed["stats"].n_deferred == records["stats"].n_deferred
    worst = _relative_per_pixel(composed, records)
    print(f"window {window}: composed vs records {worst:.2e}, deferred {composed['stats'].n_deferred} of {composed['stats'].n_samples}")
    assert worst <= 1.0e-12


@pytest.mark.gpu
def test_a_frame_with_spin(frame_grid):
    cuts = dict(CUTS["sigma_max"], simulation_a=0.9)
    exact = _render(frame_grid, cuts, "exact")
    tolerant = _render(frame_grid, cuts)
    general = _render(frame_grid, cuts, switch="GENERAL_CUTS")
    assert tolerant["stats"].fused_variant == 2
    print(f"a = 0.9: vs exact {_relative_per_pixel(tolerant, exact):.2e}, local_angles {tolerant['stats'].local_angles}, "
          f"deferred {tolerant['stats'].n_deferred} of {tolerant['stats'].n_samples}")
    _same_rays(tolerant, exact)
    assert _relative_per_pixel(tolerant, exact) <= PER_PIXEL
    _same_rays(tolerant, general)
    assert gu.same_bits(tolerant["image"], general["image"]).all()
