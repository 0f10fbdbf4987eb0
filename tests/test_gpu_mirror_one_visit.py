"""GPU: the paired walk of bl_shade_fused2_kernel, in which a sample record and its mirror image are shaded in one visit.

Every group of 64 records enters the kernel's pipeline twice in succession, as it is and as its mirror in y = 0. The mirror entry loads
nothing but its cells: the record, the per-ray constants, r and theta of the locate step and the geometry of the coefficient arithmetic are
the plain entry's. What it does on its own is phi - looked up through the table like any sample's, not reflected - and
everything the cell values enter.

As in tests/test_gpu_mirror_pairs.py every case compares a paired render with its twin under NO_MIRROR_PAIRS, over a mock modulated in phi
so that a copied half frame could not pass: the reproducible tolerant tier bit for bit with equal counts, composed maps within 1e-10 per pixel
of the exact tier. The cases are the places where the shared part could differ from locating and shading the mirror sample from scratch:
both angle paths in both walks, a phi axis without mirror symmetry, the seam of phi, a last group that is partly dead, and an unpaired
render through the same instantiation."""
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


def _grid(n_r=32, n_th=32, n_ph=64, shift=0.0):
    """The mock with rho and p multiplied by 1 + 0.3 sin(phi + 0.7), as in tests/test_gpu_mirror_pairs.py. shift != 0: the interior phi faces
    moved by up to `shift` cells with a smooth function that has no mirror symmetry, the centres the midpoints of the moved faces."""
    key = (n_r, n_th, n_ph, shift)
    if key not in _GRIDS:
        from blacklight_amd import mock
        grid = mock.generate(n_r=n_r, n_th=n_th, n_ph=n_ph)
        prim = grid.prim.copy()
        phi = np.asarray(grid.x3v, dtype=np.float64).reshape(-1)
        prim[0:2] *= (1.0 + 0.3 * np.sin(phi + 0.7)).astype(np.float32)[None, None, :, None, None]
        grid = dataclasses.replace(grid, prim=np.ascontiguousarray(prim))
        if shift != 0.0:
            faces = np.asarray(grid.x3f, dtype=np.float64).reshape(-1).copy()
            width = 2.0 * np.pi / n_ph
            u = faces[1:-1] / (2.0 * np.pi)
            # (sin(2 pi u + 1) + sin(6 pi u + 0.3) / 2: neither even nor odd about u = 1 / 2; at most 1.5, so the faces move by at most `shift` cells)
            faces[1:-1] += shift * width * (np.sin(2.0 * np.pi * u + 1.0) + 0.5 * np.sin(6.0 * np.pi * u + 0.3)) / 1.5
            faces = faces.astype(np.float32).astype(np.float64)   # (what a snapshot file holds)
            assert np.all(np.diff(faces) > 0.0)
            moved = faces[1:-1] - np.asarray(grid.x3f).reshape(-1)[1:-1]
            assert np.abs(moved + moved[::-1]).max() > 0.1 * shift * width   # (no mirror symmetry about pi)
            centres = 0.5 * (faces[:-1] + faces[1:])
            grid = dataclasses.replace(grid, x3f=np.ascontiguousarray(faces[None, :]), x3v=np.ascontiguousarray(centres[None, :]))
        _GRIDS[key] = grid
    return _GRIDS[key]


def _render(pairs, tier, reproducible=False, switches=(), grid_key=(), res=64, again=False, **overrides):
    """One render (kept: a reference is rendered once and shared, and nobody writes to it). again: a second one of the same, kept beside it."""
    key = (pairs, tier, reproducible, tuple(switches), tuple(grid_key), res, again, tuple(sorted(overrides.items())))
    if key not in _RENDERS:
        import bench
        import blacklight_amd as bl
        with bl.Context(bl.Params.from_dict(dict(bench.WORKLOAD, camera_resolution=res, **overrides))) as ctx:
            ctx.set_arithmetic(tier)
            ctx.set_reproducible(reproducible)
            ctx.debug_set_switches(*(list(switches) + ([] if pairs else ["NO_MIRROR_PAIRS"])))
            ctx.set_grid(_grid(*grid_key))
            out = ctx.render()
            out["stats"] = ctx.stats
        _RENDERS[key] = out
    return _RENDERS[key]


def _worst_relative(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        return np.nanmax(np.where(b != 0.0, np.abs(a - b) / scale, np.abs(a - b)))


def _check(switches=(), grid_key=(), res=64, paired=1, fused=2, local=None, **overrides):
    """Paired against unpaired: the reproducible tolerant tier bit for bit, composed maps within 1e-10 per pixel of the exact tier."""
    kw = dict(switches=switches, grid_key=grid_key, res=res, **overrides)
    on, off = _render(True, "tolerant", True, **kw), _render(False, "tolerant", True, **kw)
    a, b = on["stats"], off["stats"]
    assert a.mirror_pairs == paired and b.mirror_pairs == 0
    assert a.fused_variant == b.fused_variant == fused
    if local is not None:
        assert a.local_angles == b.local_angles == local
    frame = off["image"].reshape(-1, res, res)
    # (the unpaired frame's left half is not its flipped right half: a copied frame could not pass)
    assert not np.array_equal(np.nan_to_num(frame[..., : res // 2]), np.nan_to_num(frame[..., : res // 2 - 1 : -1]))
    print("deferred: paired", a.n_deferred, "unpaired", b.n_deferred, "of", a.n_samples, "samples; local_angles", a.local_angles, "fused_variant", a.fused_variant)
    assert np.array_equal(on["image"].view(np.int64), off["image"].view(np.int64))
    assert a.n_deferred == b.n_deferred
    assert np.array_equal(on["sample_num"], off["sample_num"]) and np.array_equal(on["sample_flags"], off["sample_flags"])
    assert (a.n_samples, a.n_gathers, a.n_flagged) == (b.n_samples, b.n_gathers, b.n_flagged)
    composed, exact = _render(True, "tolerant", False, **kw), _render(True, "exact", False, **kw)
    assert composed["stats"].mirror_pairs == paired
    assert np.array_equal(composed["sample_num"], exact["sample_num"]) and np.array_equal(composed["sample_flags"], exact["sample_flags"])
    worst = _worst_relative(composed["image"], exact["image"])
    print("composed maps, paired, against the exact tier: worst relative difference per pixel", worst)
    assert worst <= 1.0e-10
    return on, off


# ---------------------------------------------------------------------------------------------------------------- both angle paths
@pytest.mark.parametrize("flat", [False, True], ids=["lists", "flat"])
@pytest.mark.parametrize("path", ["local", "global_by_switch", "global_32_cubed"])
def test_both_angle_paths_in_both_walks(path, flat):
    switches = (["FLAT_ORDER"] if flat else []) + (["GLOBAL_ANGLES"] if path == "global_by_switch" else [])
    grid_key = (32, 32, 32) if path == "global_32_cubed" else ()
    on, _ = _check(switches=switches, grid_key=grid_key, local=1 if path == "local" else 0)
    assert on["stats"].xcd_order == (0 if flat else 1)
    assert on["stats"].n_deferred > 0


# ---------------------------------------------------------------------------------------------------------------- phi without symmetry
@pytest.mark.parametrize("shift,fused", [(0.1, None), (5.0e-5, 2)], ids=["tenth_of_a_cell", "within_the_even_spacing"])
def test_a_phi_axis_that_is_not_symmetric_about_pi(shift, fused):
    """With phi faces that are not mirror images of each other about pi, the mirror sample's cell and fraction are not the reflected ones of
    the plain sample: only a phi looked up through the table agrees with the unpaired render. Faces moved by a tenth of a cell are not
    evenly spaced to the 1e-4 of a cell bl_shade_fused2_kernel asks for, so that grid goes whichever way the plan sends it (the same
    way paired and unpaired: asserted); faces moved by 5e-5 of a cell stay with the fused kernel, and a reflected fraction would be off by
    as much."""
    grid_key = (32, 32, 64, shift)
    probe = _render(False, "tolerant", True, grid_key=grid_key)
    print("phi faces moved by", shift, "cells: fused_variant", probe["stats"].fused_variant, "local_angles", probe["stats"].local_angles)
    if fused is not None:
        assert probe["stats"].fused_variant == fused
    paired = _render(True, "tolerant", True, grid_key=grid_key)["stats"].mirror_pairs
    _check(grid_key=grid_key, paired=paired, fused=probe["stats"].fused_variant)
    if fused is not None:
        assert paired == 1
        # (and the moved faces matter: the frame is not the even grid's)
        assert not np.array_equal(probe["image"].view(np.int64), _render(False, "tolerant", True)["image"].view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- the seam
def test_the_seam_of_phi():
    """Eight phi cells, global angles: most samples of the middle columns lie in the first or the last phi cell and their mirror images in
    the other of the two, on the other side of the seam at 0 / 2 pi."""
    on, off = _check(switches=["GLOBAL_ANGLES"], grid_key=(32, 32, 8), res=32, local=0)
    assert on["stats"].n_deferred == off["stats"].n_deferred and on["stats"].n_deferred > 0


# ---------------------------------------------------------------------------------------------------------------- a partly dead group
@pytest.mark.parametrize("res", [32, 48])
def test_a_partly_dead_last_group(res):
    """Frames whose record counts are not a multiple of the walk's batch of 16 groups: the last batch of a list is short, and its last
    group's mirror entry follows it like any other."""
    on, off = _check(res=res)
    a, b = on["stats"], off["stats"]
    print("records: n_samples_emitted", a.n_samples_emitted, "n_gathers", a.n_gathers)
    assert a.n_samples_emitted % (2 * 16 * 64) != 0
    assert a.n_samples_emitted == b.n_samples_emitted and a.n_gathers == b.n_gathers and a.algorithmic_bytes == b.algorithmic_bytes


# ---------------------------------------------------------------------------------------------------------------- unpaired
def test_an_unpaired_render_through_the_same_instantiation():
    """camera_ph = 30 does not pair: the same kernel instantiation walks every group once, in the loop written for that."""
    first = _render(True, "tolerant", True, camera_ph=30.0)
    assert first["stats"].mirror_pairs == 0 and first["stats"].fused_variant == 2
    second = _render(True, "tolerant", True, again=True, camera_ph=30.0)
    for out in (first, second):
        st = out["stats"]
        print("unpaired: composed_maps", st.composed_maps, "local_angles", st.local_angles, "xcd_order", st.xcd_order, "deferred", st.n_deferred, "samples", st.n_samples)
    assert first["image"] is not second["image"]
    assert np.array_equal(first["image"].view(np.int64), second["image"].view(np.int64))
    composed, exact = _render(True, "tolerant", False, camera_ph=30.0), _render(True, "exact", False, camera_ph=30.0)
    assert composed["stats"].mirror_pairs == 0 and composed["stats"].composed_maps == 1
    worst = _worst_relative(composed["image"], exact["image"])
    print("unpaired, composed maps against the exact tier: worst relative difference per pixel", worst)
    assert worst <= 1.0e-10
