"""GPU: a snapshot staged from device memory (bl_set_grid_device, Context.set_grid_device) renders what the same snapshot staged from
host memory renders, bit for bit - and so the reference's goldens - whatever the layout ([variable][block] or [block][variable]), the
element type (float32, or float64 rounded on the device), the grid's kind (one block, merged blocks, a mesh with refinement, inter-block
interpolation, the electron entropy plane of plasma_model = code_kappa, slow-light slices) and the moment (beside a running render,
behind work still queued on the caller's stream). The host hands over geometry only: every grid below goes in with prim = None."""
import dataclasses
import functools
import json
import os
import threading

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu
E_ARG = 5
NOT_DEVICE = ("Error: bl_device_cells: prim must be device memory of the context's device, with n_elements elements inside one allocation; "
              "host arrays go through bl_set_grid.\n")


def _bare(grid):
    return dataclasses.replace(grid, prim=None)


def _tensor(prim, dims="vb", dtype=None):
    """The host array [variable][block][k][j][i] as a device tensor in the layout `dims` names"""
    t = torch.from_numpy(np.ascontiguousarray(prim)).cuda()
    if dtype is not None:
        t = t.to(dtype)
    return t.transpose(0, 1).contiguous() if dims == "bv" else t


@functools.lru_cache(maxsize=None)
def _case(name):
    fx, params, mock_args = gu.load_case(name)
    return fx, params, gu.golden_grid(mock_args)


def _render(params, stage, tier="exact", reproducible=False):
    import blacklight_amd as bl
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic(tier)
        ctx.set_reproducible(reproducible)
        stage(ctx)
        out = ctx.render()
        out["host_bytes"] = ctx.grid_host_bytes
        return out


@functools.lru_cache(maxsize=None)
def _host_render(name, tier="exact", reproducible=False):
    fx, params, grid = _case(name)
    return _render(params, lambda ctx: ctx.set_grid(grid), tier, reproducible)


def _device_render(name, dims="vb", tier="exact", reproducible=False, prim=None, dtype=None):
    fx, params, grid = _case(name)
    t = _tensor(grid.prim if prim is None else prim, dims, dtype)
    return _render(params, lambda ctx: ctx.set_grid_device(_bare(grid), t, dims=dims), tier, reproducible)


def _same(got, want):
    assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["image"].shape == want["image"].shape and gu.same_bits(got["image"], want["image"]).all()


def _is_the_golden(name, got):
    fx = _case(name)[0]
    n_pix = got["sample_num"].size
    assert np.array_equal(got["sample_num"], fx["B_sample_num"]) and np.array_equal(got["sample_flags"], fx["B_sample_flags"])
    want = gu.expected_image(fx, "B", n_pix)
    assert got["image"].shape == want.shape and gu.same_bits(got["image"], want).all()


def test_one_block_both_tiers(built_library):
    """sim_dp_interp, 32 x 24 x 32 cells: the golden and the host-staged render in the exact tier, the host-staged render in the
    tolerant tier; and the host copies the tables only"""
    got = _device_render("sim_dp_interp")
    _is_the_golden("sim_dp_interp", got)
    _same(got, _host_render("sim_dp_interp"))
    _same(_device_render("sim_dp_interp", tier="tolerant", reproducible=True), _host_render("sim_dp_interp", "tolerant", True))
    cell_bytes = 32 * 24 * 32 * 8 * 4
    assert cell_bytes == 786432 and 0 < got["host_bytes"] < cell_bytes <= _host_render("sim_dp_interp")["host_bytes"]


@pytest.mark.parametrize("dims", ["bv", "vb"])
def test_merged_blocks_in_both_layouts(built_library, dims):
    """sim_multiblock: 8 blocks of 16 x 12 x 16 merged into one array, from a tensor stored [block][variable] and from one stored [variable][block]"""
    got = _device_render("sim_multiblock", dims)
    _is_the_golden("sim_multiblock", got)
    assert got["stats"].launches_locate == _host_render("sim_multiblock")["stats"].launches_locate


def test_mesh_with_refinement(built_library):
    """sim_refined: 36 blocks of 8 x 6 x 8 that stay block by block"""
    assert _case("sim_refined")[2].prim.shape[1:] == (36, 8, 6, 8)
    _is_the_golden("sim_refined", _device_render("sim_refined"))
    _is_the_golden("sim_refined", _device_render("sim_refined", "bv"))


def test_inter_block_interpolation(built_library):
    _is_the_golden("sim_blockinterp", _device_render("sim_blockinterp", "bv"))


@pytest.mark.parametrize("case,dims", [("sim_code_kappa", "vb"), ("sim_code_kappa_fallback", "vb"), ("sim_code_kappa_fallback", "bv")])
def test_electron_entropy_plane(built_library, case, dims):
    """plasma_model = code_kappa: the ninth variable goes to a plane of its own - as it lies for one block, to the blocks' places for
    eight merged ones (the staging kernel's one-plane mode)"""
    grid = _case(case)[2]
    assert grid.prim.shape[0] == 9 and grid.ind_kappa == 8 and grid.prim.shape[1] == (1 if case == "sim_code_kappa" else 8)
    _is_the_golden(case, _device_render(case, dims))


def test_float64_cells_are_rounded_to_nearest(built_library):
    fx, params, grid = _case("sim_dp_interp")
    p64 = grid.prim.astype(np.float64) * (1.0 + 1.0e-3 * np.random.default_rng(7).random(grid.prim.shape))
    rounded = p64.astype(np.float32)
    assert np.isfinite(rounded).all()
    # what truncation toward zero would give: the neighbour towards zero wherever rounding went away from it
    truncated = np.where(np.abs(rounded.astype(np.float64)) > np.abs(p64), np.nextafter(rounded, np.float32(0.0)), rounded)
    assert np.mean(truncated != rounded) >= 0.25
    assert np.mean(rounded != grid.prim) >= 0.5
    got = _device_render("sim_dp_interp", prim=p64)
    assert got["host_bytes"] < 786432
    want = _render(params, lambda ctx: ctx.set_grid(dataclasses.replace(grid, prim=rounded)))
    _same(got, want)
    assert not gu.same_bits(got["image"], _host_render("sim_dp_interp")["image"]).all()


def test_polarized(built_library):
    _is_the_golden("sim_polarized", _device_render("sim_polarized"))


def test_slow_light_slices(built_library):
    """The window of slow_interp handed over slice by slice from device tensors, shifted as the reader shifts it: the images of the
    host-staged window (which test_gpu_slow_light.py holds to the reference's)"""
    import blacklight_amd as bl
    fx = np.load(os.path.join(gu.GOLDEN_DIR, "slow_interp.npz"), allow_pickle=False)
    params = json.loads(str(fx["params"]))
    grids = gu.slow_light_grids(fx)
    file_times = [float(t) for t in fx["file_times"]]
    tensors = [_tensor(g.prim) for g in grids]

    def run(from_device):
        images = []
        with bl.Context(bl.Params.from_dict(params)) as ctx:
            ctx.set_arithmetic("exact")
            held = None
            for image, (t_cam, files) in enumerate(gu.slow_light_windows(params, file_times)):
                new = len(files) if held is None or files[0] - held[0] >= len(files) else files[0] - held[0]
                if 0 < new < len(files):
                    ctx.shift_grid_slices(new)
                for n in range(new):
                    if from_device:
                        ctx.set_grid_slice_device(n, _bare(grids[files[n]]), tensors[files[n]], file_times[files[n]])
                        assert ctx.grid_host_bytes < tensors[files[n]].numel() * 4
                    else:
                        ctx.set_grid_slice(n, grids[files[n]], file_times[files[n]])
                held = files
                ctx.set_snapshot(image)
                images.append(ctx.render())
        return images

    got, want = run(True), run(False)
    assert len(got) == len(want) >= 2
    for a, b in zip(got, want):
        _same(a, b)
    assert gu.same_bits(got[0]["image"], np.stack([fx[f"B_0_{name}"].reshape(-1) for name in ("I_nu", "tau") if f"B_0_{name}" in fx.files])).all()


def test_resident_series_and_staging_beside_the_render(built_library):
    """Three snapshots resident as one tensor [3][8][1][48][48][48]: frames 2 and 3 shade the records of frame 1 and are the
    host-staged frames; the same with frames 2 and 3 staged from a second thread while the render before them runs; a tensor on
    another geometry from that thread waits its turn"""
    import bench
    import blacklight_amd as bl
    from blacklight_amd import mock
    params = dict(bench.WORKLOAD, camera_resolution=96)
    base = mock.generate(n_r=48, n_th=48, n_ph=48)
    snaps = []
    for n in range(3):   # (tests/test_gpu_series.py::_snapshots)
        prim = base.prim.copy()
        prim[0:2] *= np.float32(1.0 + 0.11 * n)
        snaps.append(dataclasses.replace(base, prim=prim))
    series = torch.from_numpy(np.stack([s.prim for s in snaps])).cuda()
    assert tuple(series.shape) == (3, 8, 1, 48, 48, 48)
    geometry = _bare(base)
    want = []
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        for grid in snaps:
            ctx.set_grid(grid)
            want.append(ctx.render())
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        got = []
        for n in range(3):
            ctx.set_grid_device(geometry, series[n])
            got.append(ctx.render())
        assert [g["stats"].geodesics_reused for g in got] == [0, 1, 1]
        for a, b in zip(got, want):
            _same(a, b)
        assert not gu.same_bits(got[0]["image"], got[1]["image"]).all()
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid_device(geometry, series[0])
        got, staged = [], None

        def stage(tensor, go):
            go.wait()   # (set by the rendering thread on its way into bl_render: the cells are staged beside the render)
            ctx.set_grid_device(geometry, tensor)

        for n in range(3):
            if staged is not None:
                staged.join()
            staged = None
            go = threading.Event()
            if n + 1 < 3:
                staged = threading.Thread(target=stage, args=(series[n + 1], go))
                staged.start()
            go.set()
            got.append(ctx.render())
        assert [g["stats"].geodesics_reused for g in got] == [0, 1, 1]
        for a, b in zip(got, want):
            _same(a, b)
        other = mock.generate(n_r=32, n_th=32, n_ph=32)
        other_tensor = _tensor(other.prim)
        worker = threading.Thread(target=ctx.set_grid_device, args=(_bare(other), other_tensor))
        worker.start()
        during = ctx.render()   # (either grid, whole: the two calls exclude each other)
        worker.join()
        after = ctx.render()
    alone = _render(params, lambda c: c.set_grid(other))
    _same(after, alone)
    assert gu.same_bits(during["image"], want[-1]["image"]).all() or gu.same_bits(during["image"], alone["image"]).all()


def test_staging_waits_for_the_callers_stream(built_library):
    """The tensor is filled on a side stream - a copy from pinned memory, then multiplications and divisions by a power of two in
    place, so that the data arrives late - and handed over with that stream and no synchronisation: the golden. Then the tensor is
    zeroed as soon as the call has returned: still the golden, the call had finished with the caller's memory."""
    import blacklight_amd as bl
    fx, params, grid = _case("sim_multiblock")
    pinned = torch.from_numpy(grid.prim).pin_memory()
    tensor = torch.full(grid.prim.shape, float("nan"), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        with torch.cuda.stream(side):
            tensor.copy_(pinned, non_blocking=True)
            for _ in range(32):
                tensor.mul_(1024.0)
                tensor.div_(1024.0)
        ctx.set_grid_device(_bare(grid), tensor, stream=side.cuda_stream)
        tensor.zero_()
        _is_the_golden("sim_multiblock", ctx.render())
        torch.cuda.synchronize()
        assert not tensor.any()
        _is_the_golden("sim_multiblock", ctx.render())


def test_what_is_not_device_memory_is_refused(built_library):
    """A pinned host buffer through the C call itself: BL_E_ARG with its text, nothing launched, and the grid in place still renders
    its image. A CPU tensor through the Python call: ValueError."""
    import ctypes as C
    import blacklight_amd as bl
    from blacklight_amd import _capi
    fx, params, grid = _case("sim_dp_interp")
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(grid)
        pinned = ctx.pinned_array(grid.prim.shape, np.float32)
        pinned[...] = grid.prim
        desc = _bare(grid).desc()
        cells = _capi.DeviceCells()
        cells.prim, cells.dtype = pinned.ctypes.data, _capi.BL_CELLS_F32
        cells.var_stride = cells.block_stride = 32 * 24 * 32
        cells.n_elements = pinned.size
        rc = ctx._lib.bl_set_grid_device(ctx._ctx, C.byref(desc), C.byref(cells))
        assert (rc, ctx._lib.bl_last_error(ctx._ctx).decode()) == (E_ARG, NOT_DEVICE)
        with pytest.raises(ValueError):
            ctx.set_grid_device(grid, torch.from_numpy(grid.prim))
        _is_the_golden("sim_dp_interp", ctx.render())
