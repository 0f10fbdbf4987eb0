"""GPU: the inputs at which a changed select or a changed per-ray read of bl_shade_fused2_kernel can go wrong.

The kernel reads a ray's k_t and momentum factor as one pair (BlShadeArgs::ray_constants), and its compare-and-select forms - the face
margins, the cell clamps, the record of a step that does not absorb, the <= 0 rule of the trilinear read, `no_field` - are what the
frames below exercise at their edges (profiles/fused_selects.md: forms that were measured and not kept). Every case renders a 64 x 64
camera over the 32^3 mock and holds, as tests/test_gpu_fused_loop.py does,

  * the tolerant frame to the exact tier's within 1e-10 per pixel of the pixel's own intensity, NaN for NaN,
  * sample_num, the flags and the NaN masks to equality,
  * two renders under bl_set_reproducible to the same bits.

  a  the benchmark's physics
  b  a camera on the polar axis: a 64 x 64 window of a 65 x 65 camera at camera_th = 0, whose centre pixel's ray has x = y = 0 at every
     sample (rho = 0: NaN phi on the local-angle path, pp2 == 0 in shade(), margins that must stay NaN). Rendered alone, that pixel
     must leave every sample it gathers to the exact pass.
  c  the field set to zero in a ring of cells and the density at the mock's floor in another (no_field, reciprocals of zero, samples on
     both sides of cut_sigma_max): each ring must change the exact frame.
  d  spin 0.9 (the <false, ...> instantiations)
  e  absorbing frames: image_frequency lowered to 23 GHz, where by an optical-depth image of the exact tier some pixels have a step of
     delta_tau >= 2^-10 and none above kDeltaTauMax = 100 (a step through expm1), and to 5 GHz, where some have a step above 100 (an
     optically thick one): a ray of n samples and optical depth tau has a step of at least tau / n and none above tau.

The 32^3 mock's phi cells are too wide for the search's local angles (kLocalAngleReach), so a, b and d run once more over the
32 x 32 x 64 mock, where the plan takes them (bl_stats::local_angles)."""
import os
import sys

import numpy as np
import pytest
import torch   # noqa: F401 (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

RESOLUTION = 64
EXPM1_FREQUENCY, THICK_FREQUENCY = 2.3e10, 5.0e9
_iv, _iu = np.mgrid[0:RESOLUTION, 0:RESOLUTION]
AXIS_WINDOW = (_iv * (RESOLUTION + 1) + _iu).reshape(-1).astype(np.int32)   # pixel (32, 32) of the 65 x 65 camera looks down the axis
AXIS_PIXEL = np.array([(RESOLUTION // 2) * (RESOLUTION + 1) + RESOLUTION // 2], dtype=np.int32)
AXIS = dict(camera_th=0.0, camera_resolution=RESOLUTION + 1)

# name -> (grid, parameter overrides, pixel map)
CASES = {
    "a_benchmark": ("mock", {}, None),
    "b_polar_axis": ("mock", AXIS, AXIS_WINDOW),
    "c_no_field_and_floor": ("rings", {}, None),
    "d_spin": ("mock", dict(simulation_a=0.9), None),
    "e_absorbing_expm1": ("mock", dict(image_frequency=EXPM1_FREQUENCY), None),
    "e_absorbing_thick": ("mock", dict(image_frequency=THICK_FREQUENCY), None),
    "a_benchmark_local_angles": ("mock_64_phi", {}, None),
    "b_polar_axis_local_angles": ("mock_64_phi", AXIS, AXIS_WINDOW),
    "d_spin_local_angles": ("mock_64_phi", dict(simulation_a=0.9), None),
}


def _with_rings(grid, field=True, floor=True):
    """The grid with B = 0 in the ring of cells r 8..12 x theta 13..18 and rho at the mock's floor in r 16..20 x theta 13..18 (all phi:
    the camera's rays cross the midplane in both)."""
    import dataclasses
    from blacklight_amd import mock
    prim = grid.prim.copy()
    if field:
        prim[5:8, :, :, 13:19, 8:13] = 0.0
    if floor:
        prim[0, :, :, 13:19, 16:21] = np.float32(mock.DEFAULTS["rho_floor"])
    return dataclasses.replace(grid, prim=prim)


@pytest.fixture(scope="module")
def grids():
    from blacklight_amd import mock
    plain = mock.generate(n_r=32, n_th=32, n_ph=32)
    return {"mock": plain, "rings": _with_rings(plain), "field_ring": _with_rings(plain, floor=False), "floor_ring": _with_rings(plain, field=False),
            "mock_64_phi": mock.generate(n_r=32, n_th=32, n_ph=64)}


def _render(grid, overrides, tier="tolerant", pixel_map=None):
    import blacklight_amd as bl
    import bench
    params = dict(bench.WORKLOAD, camera_resolution=RESOLUTION)
    params.update(overrides)
    with bl.Context(bl.Params.from_dict(params)) as c:
        c.set_arithmetic(tier)
        c.set_reproducible(True)
        c.set_grid(grid)
        return c.render(pixel_map=pixel_map) if pixel_map is not None else c.render()


_frames = {}


def _frame(grids, grid_name, overrides, tier, pixel_map=None, key=None):
    """One render per (case, tier), shared among the tests and left unchanged."""
    key = (key or (grid_name, tuple(sorted(overrides.items()))), tier)
    if key not in _frames:
        _frames[key] = _render(grids[grid_name], overrides, tier, pixel_map)
    return _frames[key]


def _case(grids, name, tier):
    grid_name, overrides, pixel_map = CASES[name]
    return _frame(grids, grid_name, overrides, tier, pixel_map, key=name)


def _relative_per_pixel(got, want):
    a, b = got["image"], want["image"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b)
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        return float(np.nanmax(np.where(b != 0.0, err / scale, err)))


@pytest.mark.parametrize("name", list(CASES))
def test_tolerant_frame_against_the_exact_tier(grids, name):
    exact = _case(grids, name, "exact")
    tolerant = _case(grids, name, "tolerant")
    st = tolerant["stats"]
    assert st.fused_variant == 2
    assert st.local_angles == (1 if name.endswith("local_angles") else 0)
    assert tolerant["image"].shape[-1] == RESOLUTION * RESOLUTION
    worst = _relative_per_pixel(tolerant, exact)
    print(f"{name}: tolerant vs exact {worst:.2e}, deferred {st.n_deferred} of {st.n_samples} samples, {st.n_gathers} gathers, "
          f"{int(np.isnan(exact['image']).sum())} NaN pixels, local_angles {st.local_angles}")
    assert np.array_equal(tolerant["sample_num"], exact["sample_num"])
    assert np.array_equal(tolerant["sample_flags"], exact["sample_flags"])
    assert st.n_samples == exact["stats"].n_samples
    assert worst <= 1.0e-10
    assert np.nanmax(exact["image"]) > 0.0   # (a frame, not a blank)


@pytest.mark.parametrize("name", list(CASES))
def test_two_reproducible_renders_have_the_same_bits(grids, name):
    grid_name, overrides, pixel_map = CASES[name]
    first = _case(grids, name, "tolerant")
    second = _render(grids[grid_name], overrides, "tolerant", pixel_map)
    assert gu.same_bits(first["image"], second["image"]).all()
    assert np.array_equal(first["sample_num"], second["sample_num"])
    assert np.array_equal(first["sample_flags"], second["sample_flags"])
    assert first["stats"].n_deferred == second["stats"].n_deferred
    assert first["stats"].n_gathers == second["stats"].n_gathers


@pytest.mark.parametrize("grid_name", ["mock", "mock_64_phi"])
def test_the_axis_ray_is_left_to_the_exact_pass(grids, grid_name):
    """b: the centre pixel of the 65 x 65 camera alone - x = y = 0 at every sample, so every sample it gathers is deferred - and, for
    contrast, a pixel near it alone, which is not on the axis."""
    on_axis = _render(grids[grid_name], AXIS, "tolerant", AXIS_PIXEL)
    beside = _render(grids[grid_name], AXIS, "tolerant", AXIS_PIXEL + 2 * (RESOLUTION + 1) + 1)   # (one across, two up: off the seam and off a face of phi)
    st, st_beside = on_axis["stats"], beside["stats"]
    print(f"{grid_name}: axis ray {st.n_deferred} deferred of {st.n_gathers} gathers; a pixel beside it {st_beside.n_deferred} of {st_beside.n_gathers}")
    assert st.n_gathers > 0 and st.n_deferred == st.n_gathers
    assert st_beside.n_gathers > 0 and st_beside.n_deferred < st_beside.n_gathers
    assert _case(grids, "b_polar_axis" + ("_local_angles" if grid_name == "mock_64_phi" else ""), "tolerant")["stats"].n_deferred >= st.n_deferred


def test_each_ring_changes_the_frame(grids):
    """c: the rays cross the ring without a field and the ring at the density floor, and the sigma cut takes samples of the latter."""
    plain = _case(grids, "a_benchmark", "exact")
    both = _case(grids, "c_no_field_and_floor", "exact")
    field = _frame(grids, "field_ring", {}, "exact")
    floor = _frame(grids, "floor_ring", {}, "exact")
    uncut = _frame(grids, "floor_ring", dict(cut_sigma_max=-1.0), "exact")
    changed = {k: int((~gu.same_bits(v["image"], plain["image"])).sum()) for k, v in (("field", field), ("floor", floor), ("both", both))}
    print(f"pixels changed: {changed}; by the sigma cut in the floor ring {int((~gu.same_bits(floor['image'], uncut['image'])).sum())}")
    assert changed["field"] > 0 and changed["floor"] > 0
    assert not gu.same_bits(both["image"], field["image"]).all() and not gu.same_bits(both["image"], floor["image"]).all()
    # samples on both sides of cut_sigma_max: the cut removes samples (the frames differ) and leaves samples (the frame is not blank)
    assert not gu.same_bits(floor["image"], uncut["image"]).all()
    assert np.nanmax(both["image"]) > 0.0
    assert _case(grids, "c_no_field_and_floor", "tolerant")["stats"].n_deferred > 0


@pytest.mark.parametrize("name,frequency", [("e_absorbing_expm1", EXPM1_FREQUENCY), ("e_absorbing_thick", THICK_FREQUENCY)])
def test_the_absorbing_frames_have_expm1_and_thick_steps(grids, name, frequency):
    """e: by the exact tier's optical-depth image at the case's frequency."""
    out = _frame(grids, "mock", dict(image_frequency=frequency, image_tau=True), "exact")
    assert out["image"].shape[0] == 2
    tau, n = out["image"][1], np.maximum(out["sample_num"], 1)
    with np.errstate(invalid="ignore"):
        through_expm1 = int(((tau / n >= 2.0 ** -10) & (tau <= 100.0)).sum())
        thick = int((tau / n > 100.0).sum())
    print(f"frequency {frequency:g}: tau up to {np.nanmax(tau):.3g}; pixels with a step through expm1 {through_expm1}, with a thick step {thick}")
    assert (through_expm1 if name == "e_absorbing_expm1" else thick) > 0
    # (the frame the other tests compare is this one's first row)
    assert gu.same_bits(out["image"][0], _case(grids, name, "exact")["image"][0]).all()
