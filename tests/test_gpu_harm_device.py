"""iharm3d-family primitives staged from device memory (bl_set_grid_device_harm, bl_set_grid_slice_device_harm, bl_harm_convert_device):
the harm form of the staging kernel against the host conversion of the same header and cells (bl_harm_convert_host, which
tests/test_harm_host.py holds to the file reader's bytes), and renders after it against the renders after set_grid(Snapshot) and the
reference's images of the fixtures.

Shapes (n1, n2, n3, n_prim) of the synthetic arrays: a single cell; 17 x 3 x 5, inside one tile of 32 i's by 8 k's with a ragged edge in
both; 64 x 2 x 64, two whole tiles in i and a whole chunk of eight tiles in k; 65 x 1 x 33, one past the tile in i and in k with a
single-element axis, ten variables in a permuted order; 3 x 2 x 130, two chunks of k and two cells of a third, thirteen variables
permuted. Finite values are compared bit for bit, NaNs by position."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READER_DIR = os.path.join(gu.GOLDEN_DIR, "reader")
FIXTURES = {"mks": ("expected_iharm3d.npz", "iharm3d_mock.h5", ("plain", "spin")), "fmks": ("expected_fmks.npz", "iharm3d_fmks.h5", ("interp", "nearest"))}
SHAPES = [(1, 1, 1, 8), (17, 3, 5, 8), (64, 2, 64, 8), (65, 1, 33, 10), (3, 2, 130, 13)]
PERMUTED = {10: (7, 2, 9, 0, 5, 3, 8, 1, 4), 13: (12, 0, 6, 11, 3, 9, 1, 7, 10)}   # rho, UU, U1..3, B1..3, entropy


def fixture_params(kind, case, **overrides):
    from blacklight_amd import Params
    expected, file, _ = FIXTURES[kind]
    fx = np.load(os.path.join(READER_DIR, expected), allow_pickle=False)
    params = json.loads(str(fx[f"{case}_params"]))
    params["simulation_file"] = os.path.join(READER_DIR, file)
    params.update(overrides)
    return fx, Params.from_dict({k: v for k, v in params.items() if v is not None})


def same_planes(got, want):
    """Finite values bit for bit (a -0.0 is no 0.0), NaNs by position"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def synthetic_header(kind, shape, code_kappa):
    """A header of the fixture's kind with the counts and the variable order of `shape`"""
    from blacklight_amd import Snapshot
    _, p = fixture_params(kind, FIXTURES[kind][2][0], **(dict(plasma_model="code_kappa", simulation_kappa_name="RHO") if code_kappa else {}))
    with Snapshot(p, raw=True) as raw:
        header = raw.harm_header
    n1, n2, n3, n_prim = shape
    # (the fixture's extent in x^1 and x^2 over the new counts; x^3 over the circle)
    header.dx[0], header.dx[1], header.dx[2] = header.dx[0] * header.n1 / n1, header.dx[1] * header.n2 / n2, 2.0 * np.pi / n3
    header.n1, header.n2, header.n3, header.n_prim = n1, n2, n3, n_prim
    order = PERMUTED.get(n_prim, tuple(range(8)) + (0,))
    for name, index in zip(("ind_rho", "ind_uu", "ind_u1", "ind_u2", "ind_u3", "ind_b1", "ind_b2", "ind_b3", "ind_kappa"), order):
        setattr(header, name, index)
    return p, header


def synthetic_prims(shape, seed, special=False):
    rng = np.random.default_rng(seed)
    prims = rng.standard_normal(shape) * 0.3
    prims[..., :] += rng.random(shape) * 0.2
    if special and prims[..., 0].size >= 3:
        flat = prims.reshape(-1, shape[3])
        flat[0, :] = np.nan                                   # a NaN cell
        flat[1, :] = -0.0                                     # a cell of negative zeros
        flat[2, :] = 1.0e-42                                  # a cell that is denormal in float32
        flat[-1, :] = [(-1.0) ** v * 4.0e-40 for v in range(shape[3])]
    return prims


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", ["mks", "fmks"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_conversion_equals_the_host_conversion(built_library, shape, kind, dtype):
    import torch
    from blacklight_amd import Context
    from blacklight_amd.snapshot import HarmGrid
    p, header = synthetic_header(kind, shape, code_kappa=False)
    grid = HarmGrid(p, header)
    wide = synthetic_prims(shape, seed=sum(shape), special=shape == (17, 3, 5, 8))
    given = wide.astype(np.float32) if dtype == "float32" else wide
    want = grid.convert_host(given.astype(np.float32))   # (F64 cells are rounded to float first, as a float32 file would hold them)
    with Context(p) as ctx:
        got = ctx.harm_convert_device(grid, torch.from_numpy(given).cuda())
        assert got.shape == (8, shape[2], shape[1], shape[0]) and got.dtype == torch.float32
        assert same_planes(got.cpu().numpy(), want)
        if shape == (17, 3, 5, 8):
            assert np.isnan(want).any() and np.signbit(want[0].reshape(-1)).any() and ((np.abs(want[0]) < 1.0e-38) & (want[0] != 0)).any()
    grid.close()


@pytest.mark.parametrize("kind", ["mks", "fmks"])
def test_entropy_plane(built_library, kind):
    """plasma_model = code_kappa: the ninth plane, from a ninth variable of a permuted array and from the array's own variables"""
    import torch
    from blacklight_amd import Context
    from blacklight_amd.snapshot import HarmGrid
    for shape in ((65, 1, 33, 10), (17, 3, 5, 8)):
        p, header = synthetic_header(kind, shape, code_kappa=True)
        grid = HarmGrid(p, header)
        prims = synthetic_prims(shape, seed=7).astype(np.float32)
        want = grid.convert_host(prims)
        assert want.shape[0] == 9 and same_planes(want[8], prims[..., header.ind_kappa].transpose(2, 1, 0))
        with Context(p) as ctx:
            got = ctx.harm_convert_device(grid, torch.from_numpy(prims).cuda())
            assert same_planes(got.cpu().numpy(), want)
        grid.close()


@pytest.mark.parametrize("kind", ["mks", "fmks"])
def test_fixture_conversion(built_library, kind):
    import torch
    from blacklight_amd import Context, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    _, p = fixture_params(kind, FIXTURES[kind][2][0])
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
    with Snapshot(p) as snap:
        arrays = snap.arrays()
    grid = HarmGrid(p, header)
    with Context(p) as ctx:
        got = ctx.harm_convert_device(grid, torch.from_numpy(prims).cuda()).cpu().numpy()
    assert same_planes(got, grid.convert_host(prims))
    for q, name in enumerate(("ind_rho", "ind_pgas", "ind_uu1", "ind_uu2", "ind_uu3", "ind_bb1", "ind_bb2", "ind_bb3")):
        assert got[q].tobytes() == arrays["prim"][arrays["indices"][name], 0].tobytes(), name


def _render(ctx):
    out = ctx.render()
    return out["image"].copy(), out["sample_num"].copy(), out["sample_flags"].copy()


def _same_render(a, b):
    return gu.same_bits(a[0], b[0]).all() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kind,case", [("mks", "plain"), ("mks", "spin"), ("fmks", "interp"), ("fmks", "nearest")])
def test_render_after_device_staging(built_library, kind, case):
    """Both tiers after set_grid_device_harm against set_grid(Snapshot) bit for bit, the exact tier against the reference's image; then
    the series' fast path with other cells, float64 this time"""
    import torch
    from blacklight_amd import Context, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    fx, p = fixture_params(kind, case)
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
    grid = HarmGrid(p, header)
    rows = ["I_nu"] + (["tau"] if f"{case}_B_tau" in fx.files else [])
    golden = np.stack([fx[f"{case}_B_{name}"].reshape(-1) for name in rows])
    with Context(p) as ctx, Context(p) as by_file:
        ctx.set_arithmetic("exact")
        by_file.set_arithmetic("exact")
        with Snapshot(p) as snap:
            by_file.set_grid(snap)
        ctx.set_grid_device_harm(grid, torch.from_numpy(prims).cuda())
        # tables and no cells: what the host planes' call copied, less its eight planes, and the point table (20 doubles a point)
        assert ctx.grid_host_bytes == by_file.grid_host_bytes - 8 * 4 * header.n1 * header.n2 * header.n3 + 160 * header.n1 * header.n2
        want, got = _render(by_file), _render(ctx)
        assert _same_render(got, want) and gu.same_bits(got[0], golden).all()
        for c in (ctx, by_file):
            c.set_arithmetic("tolerant")
            c.set_reproducible(True)
        assert _same_render(_render(ctx), _render(by_file))
        # the next snapshot of a series: the same geometry, other cells - nothing comes from the host, the render reads the new cells
        scaled = prims.astype(np.float64)
        scaled[..., header.ind_rho] *= 1.5
        ctx.set_grid_device_harm(grid, torch.from_numpy(scaled).cuda())
        assert ctx.grid_host_bytes == 0
        planes = grid.convert_host(scaled.astype(np.float32))
        by_file.set_grid_device(_Converted(grid), torch.from_numpy(planes[:, None]).cuda())
        moved, moved_want = _render(ctx), _render(by_file)
        assert _same_render(moved, moved_want) and not gu.same_bits(moved[0], got[0]).all()
    grid.close()


class _Converted:
    """A HarmGrid as set_grid_device takes a grid: the description for converted planes"""

    def __init__(self, grid):
        self.grid = grid

    def desc(self):
        from blacklight_amd import _capi
        return _capi.GridDesc.from_buffer_copy(self.grid.desc(converted=True))


@pytest.mark.parametrize("case", ["interp", "nearest"])
def test_slow_light_slices(built_library, case):
    """The fmksslow window staged slice by slice from device memory against the library's own window of files, exact tier"""
    import torch
    from blacklight_amd import Context, Params, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    fx = np.load(os.path.join(READER_DIR, "expected_fmks_slow.npz"), allow_pickle=False)
    params = json.loads(str(fx[f"{case}_params"]))
    params["simulation_file"] = os.path.join(READER_DIR, "fmksslow_{02d}.h5")
    p = Params.from_dict({k: v for k, v in params.items() if k != "output_file"})
    file_times = [float(t) for t in fx["file_times"]]
    raws = {}
    for number in range(len(file_times)):
        with Snapshot(p, file_number=number, raw=True) as raw:
            assert raw.time == file_times[number]
            raws[number] = (raw.harm_header, torch.from_numpy(raw.harm_prims()).cuda())
    grid = HarmGrid(p, raws[0][0])
    rows = ["I_nu"] + (["tau"] if f"{case}_B_0_tau" in fx.files else [])
    with Context(p) as ctx, Context(p) as by_file:
        ctx.set_arithmetic("exact")
        by_file.set_arithmetic("exact")
        for image, (t_cam, files) in enumerate(gu.slow_light_windows(params, file_times)):
            for n, f in enumerate(files):
                ctx.set_grid_slice_device_harm(n, grid, raws[f][1], file_times[f])
            ctx.set_snapshot(image)
            by_file.slow_light_read(image)
            got, want = _render(ctx), _render(by_file)
            assert _same_render(got, want), image
            assert gu.same_bits(got[0], np.stack([fx[f"{case}_B_{image}_{name}"].reshape(-1) for name in rows])).all(), image
    grid.close()


def _nine_variables(prims, header):
    """The fixture's cells with a ninth variable, an entropy that is no copy of another variable"""
    entropy = prims[..., header.ind_rho:header.ind_rho + 1] * np.float32(1.7) + np.float32(0.01)
    wide = type(header).from_buffer_copy(header)
    wide.n_prim, wide.ind_kappa = header.n_prim + 1, header.n_prim
    return np.ascontiguousarray(np.concatenate([prims, entropy], axis=3)), wide


@pytest.mark.parametrize("kind,case", [("mks", "plain"), ("fmks", "interp")])
def test_render_with_the_entropy_staged_on_the_device(built_library, kind, case):
    """plasma_model = code_kappa through set_grid_device_harm - the launch that places the entropy plane where the sampler reads it - in
    the exact tier: with the entropy a variable the file has, against set_grid(Snapshot); with a ninth variable, against the converted
    planes staged by set_grid_device; then the plain form of the kernel on the context that ran the harm form."""
    import torch
    from blacklight_amd import Context, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    _, p = fixture_params(kind, case, plasma_model="code_kappa", simulation_kappa_name="RHO")
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
    grid = HarmGrid(p, header)
    with Context(p) as ctx, Context(p) as other:
        ctx.set_arithmetic("exact")
        other.set_arithmetic("exact")
        with Snapshot(p) as snap:
            other.set_grid(snap)
        ctx.set_grid_device_harm(grid, torch.from_numpy(prims).cuda())
        named = _render(ctx)
        assert _same_render(named, _render(other))
        wide_prims, wide_header = _nine_variables(prims, header)
        wide = HarmGrid(p, wide_header)
        planes = wide.convert_host(wide_prims)
        assert planes.shape[0] == 9
        other.set_grid_device(_Converted(wide), torch.from_numpy(planes[:, None]).cuda())
        ctx.set_grid_device_harm(wide, torch.from_numpy(wide_prims).double().cuda())
        ninth, want = _render(ctx), _render(other)
        assert _same_render(ninth, want) and not gu.same_bits(ninth[0], named[0]).all()   # (the plane is read: another entropy, another image)
        ctx.set_grid_device(_Converted(wide), torch.from_numpy(planes[:, None]).cuda())
        assert _same_render(_render(ctx), want)
        wide.close()
    grid.close()


def test_slow_light_slice_with_the_entropy(built_library):
    """A window of slices with plasma_model = code_kappa: every slice's entropy plane from the device array"""
    import torch
    from blacklight_amd import Context, Params, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    fx = np.load(os.path.join(READER_DIR, "expected_fmks_slow.npz"), allow_pickle=False)
    params = dict(json.loads(str(fx["interp_params"])), plasma_model="code_kappa", simulation_kappa_name="RHO")
    params["simulation_file"] = os.path.join(READER_DIR, "fmksslow_{02d}.h5")
    p = Params.from_dict({k: v for k, v in params.items() if k != "output_file"})
    file_times = [float(t) for t in fx["file_times"]]
    t_cam, files = next(iter(gu.slow_light_windows(params, file_times)))
    grid = None
    with Context(p) as ctx, Context(p) as by_file:
        ctx.set_arithmetic("exact")
        by_file.set_arithmetic("exact")
        for n, f in enumerate(files):
            with Snapshot(p, file_number=f, raw=True) as raw:
                grid = grid or HarmGrid(p, raw.harm_header)
                ctx.set_grid_slice_device_harm(n, grid, torch.from_numpy(raw.harm_prims()).cuda(), file_times[f])
        ctx.set_snapshot(0)
        by_file.slow_light_read(0)
        assert _same_render(_render(ctx), _render(by_file))
    grid.close()


def test_refusals_on_the_device(built_library):
    import torch
    from blacklight_amd import BlacklightError, Context, Snapshot, _capi
    from blacklight_amd.snapshot import HarmGrid
    _, p = fixture_params("mks", "plain")
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
    grid = HarmGrid(p, header)
    on_device = torch.from_numpy(prims).cuda()
    L = _capi.lib()
    with Context(p) as ctx:
        def cells(prim, dtype=0, n_elements=prims.size):
            c = _capi.HarmCells()
            c.prim, c.dtype, c.n_elements = prim, dtype, n_elements
            return c

        def refused(c, text):
            for rc in (L.bl_set_grid_device_harm(ctx._ctx, grid.handle, C.byref(c)),
                       L.bl_harm_convert_device(ctx._ctx, grid.handle, C.byref(c), on_device.data_ptr())):
                assert (rc, L.bl_last_error(ctx._ctx).decode()) == (5, f"Error: {text}\n")

        pointer_text = "bl_harm_cells: prim must be device memory of the context's device, with n_elements elements inside one allocation."
        refused(cells(prims.ctypes.data), pointer_text)                                                     # a host array
        pinned = torch.from_numpy(prims).pin_memory()
        refused(cells(pinned.data_ptr()), pointer_text)                                                     # ... pinned or not
        refused(cells(on_device.data_ptr(), n_elements=1 << 40), pointer_text)                              # past the allocation's end
        refused(cells(on_device.data_ptr(), n_elements=prims.size - 1), "bl_harm_cells: n_elements is smaller than n1 * n2 * n3 * n_prim.")
        refused(cells(on_device.data_ptr() + 2), "bl_harm_cells: prim is not aligned to its element type.")
        refused(cells(on_device.data_ptr(), dtype=3), "bl_harm_cells: dtype must be BL_CELLS_F32 or BL_CELLS_F64.")
        if torch.cuda.device_count() > 1:
            other = torch.from_numpy(prims).to("cuda:1")
            refused(cells(other.data_ptr()), pointer_text)                                                  # another device
            with pytest.raises(ValueError):
                ctx.set_grid_device_harm(grid, other)
        for bad in (prims, torch.from_numpy(prims), on_device.to(torch.float16), on_device[:, :, ::2], on_device[:-1]):
            with pytest.raises(ValueError):
                ctx.set_grid_device_harm(grid, bad)
        with pytest.raises(BlacklightError, match="before bl_set_grid"):   # a refused call left no grid behind
            ctx.render()
    grid.close()


def test_resource_report(built_library):
    from blacklight_amd import build as bl_build
    text = open(os.path.join(bl_build.OBJ, "bl_api.resources.txt")).read()
    assert text.count("Function Name:") == 1 and "Function Name: bl_interleave_cells_kernel" in text
    assert "ScratchSize [bytes/lane]: 0" in text and "Occupancy [waves/SIMD]: 8" in text
    # the harm form's LDS is dynamic - plain launches ask for none - and its registers stay within the 64 that eight waves allow
    assert "LDS Size [bytes/block]: 0" in text
    vgprs = int(text.split(" VGPRs: ")[1].split()[0])
    assert 22 < vgprs <= 64   # (22: the plain form alone)
