"""GPU: the trace order per XCD (BlTraceArgs::xcd_state, the default) against one queue and a flat walk of the records
(BL_SWITCH_FLAT_ORDER).

The benchmark frame's rays are dealt to one queue per XCD in 64 x 64-pixel super-tiles, each XCD's record blocks are listed, and the
fused coefficient kernel walks the list of the XCD it runs on. Placement changes only speed: the rays, their samples and every count
must be the same, the exact tier and the reproducible tolerant tier bit for bit; composed maps group neighbouring records, whose order
follows the order of the records, so their intensities agree to rounding. A frame forced into several chunks and a series over kept
geodesics must give what the flat order gives. bl_stats.xcd_order says which order ran."""
import os
import sys

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def bench_grid():
    from blacklight_amd import mock
    return mock.generate(n_r=256, n_th=256, n_ph=256)


def _params(res):
    import bench
    return dict(bench.WORKLOAD, camera_resolution=res)


def _render(grid, res, xcd, tier="tolerant", reproducible=False, cap=None):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(_params(res))) as ctx:
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        ctx.set_tail_policy("wide")   # (at 256^2 BL_TAIL_AUTO splits off the photon ring's rays, which the order leaves alone)
        if cap is not None:
            ctx.set_scratch_limit(int(cap))
        if not xcd:
            ctx.debug_set_switches("FLAT_ORDER")
        ctx.set_grid(grid)
        out = ctx.render()
        out["stats"] = ctx.stats
    return out


def _same_rays(got, want):
    assert np.array_equal(got["sample_num"], want["sample_num"])
    assert np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["stats"].n_chunks == want["stats"].n_chunks
    assert got["stats"].n_samples == want["stats"].n_samples


def _close_per_pixel(got, want, tolerance=1.0e-12):
    a, b = got["image"], want["image"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b)
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        assert np.nanmax(np.where(b != 0.0, err / scale, err)) <= tolerance


@pytest.mark.parametrize("res", [256, 1024])
def test_tolerant_frame_matches_the_flat_order(bench_grid, res):
    xcd, flat = _render(bench_grid, res, True), _render(bench_grid, res, False)
    assert xcd["stats"].switches == 0 and flat["stats"].switches != 0
    assert xcd["stats"].xcd_order == 1 and flat["stats"].xcd_order == 0
    assert xcd["stats"].n_chunks == 1
    _same_rays(xcd, flat)
    # every record shaded exactly once: as many samples read the grid, as many were deferred
    assert xcd["stats"].n_gathers == flat["stats"].n_gathers
    assert xcd["stats"].composed_maps == 1
    _close_per_pixel(xcd, flat)


@pytest.mark.parametrize("res", [256, 1024])
def test_exact_and_reproducible_frames_are_the_same_bits(bench_grid, res):
    for tier, reproducible in (("exact", False), ("tolerant", True)):
        xcd = _render(bench_grid, res, True, tier, reproducible)
        flat = _render(bench_grid, res, False, tier, reproducible)
        # (the exact tier's kernel does not walk the lists: the order stays flat there whatever the switch says)
        assert xcd["stats"].xcd_order == (1 if tier == "tolerant" else 0) and flat["stats"].xcd_order == 0
        _same_rays(xcd, flat)
        assert xcd["stats"].n_gathers == flat["stats"].n_gathers
        assert gu.same_bits(xcd["image"], flat["image"]).all(), (tier, reproducible)


def test_frame_of_several_chunks_matches_the_flat_order(bench_grid):
    one = _render(bench_grid, 256, False)
    # records and shading arrays for about half the frame's samples: the gate closes and the rays it left go to the next chunk (the
    # per-XCD order is planned only where one chunk is sure to take the frame: it stays off here)
    cap = int(0.5 * one["stats"].n_samples_emitted * (64 + 16 + 16 + 1))
    xcd, flat = _render(bench_grid, 256, True, cap=cap), _render(bench_grid, 256, False, cap=cap)
    assert flat["stats"].n_chunks >= 2 and xcd["stats"].n_chunks >= 2
    assert xcd["stats"].xcd_order == 0
    assert np.array_equal(xcd["sample_num"], one["sample_num"]) and np.array_equal(xcd["sample_flags"], one["sample_flags"])
    assert xcd["stats"].n_samples == one["stats"].n_samples
    _close_per_pixel(xcd, flat)
    _close_per_pixel(xcd, one)


def test_series_over_kept_geodesics_matches_fresh_renders(bench_grid):
    import dataclasses
    import blacklight_amd as bl
    snaps = []
    for n in range(4):
        prim = bench_grid.prim.copy()
        prim[0:2] *= np.float32(1.0 + 0.11 * n)
        snaps.append(dataclasses.replace(bench_grid, prim=prim))
    with bl.Context(bl.Params.from_dict(_params(256))) as ctx:
        ctx.set_arithmetic("tolerant")
        ctx.set_geodesic_reuse(True)
        ctx.set_tail_policy("wide")
        frames = []
        for grid in snaps:
            ctx.set_grid(grid)
            out = ctx.render()
            out["stats"] = ctx.stats
            frames.append(out)
    assert [f["stats"].geodesics_reused for f in frames][1:] == [1, 1, 1]
    assert frames[0]["stats"].xcd_order == 1   # (the frames over its records walk them flat)
    for n in (1, 2, 3):
        fresh = _render(snaps[n], 256, False)
        _same_rays(frames[n], fresh)
        fresh = _render(snaps[n], 256, True)
        _same_rays(frames[n], fresh)
        assert frames[n]["stats"].n_gathers == fresh["stats"].n_gathers
        _close_per_pixel(frames[n], fresh)
