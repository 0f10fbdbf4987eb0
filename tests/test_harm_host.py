"""iharm3d-family primitives without a GPU: the header-to-grid steps and the primitive conversion of blacklight_amd/csrc/bl_harm.h
and bl_harm.cpp, driven on their own (bl_harm_grid_create, bl_harm_convert_host) over what the raw reader (bl_snapshot_open_raw) hands
out of the iharm3d fixtures, against the ordinary reader of the same files: cells byte for byte, geometry value for value.
The reader runs the same functions, and tests/test_snapshot_reader.py with the goldens of the renders holds its bytes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READER_DIR = os.path.join(gu.GOLDEN_DIR, "reader")
FIXTURES = {"mks": ("expected_iharm3d.npz", "iharm3d_mock.h5", "plain"), "fmks": ("expected_fmks.npz", "iharm3d_fmks.h5", "interp")}
COORDINATES = ("x1f", "x2f", "x3f", "x1v", "x2v", "x3v")
INDICES = ("ind_rho", "ind_pgas", "ind_uu1", "ind_uu2", "ind_uu3", "ind_bb1", "ind_bb2", "ind_bb3")


def fixture_params(kind, case=None, **overrides):
    from blacklight_amd import Params
    expected, file, default_case = FIXTURES[kind]
    fx = np.load(os.path.join(READER_DIR, expected), allow_pickle=False)
    params = json.loads(str(fx[f"{case or default_case}_params"]))
    params["simulation_file"] = os.path.join(READER_DIR, file)
    params.update(overrides)
    return Params.from_dict({k: v for k, v in params.items() if v is not None})


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_symbols_and_struct_sizes(built_library):
    from blacklight_amd import _capi
    L = _capi.lib()
    for name in ("bl_harm_grid_create", "bl_harm_grid_desc", "bl_harm_grid_warnings", "bl_harm_grid_planes", "bl_harm_grid_free", "bl_harm_convert_host",
                 "bl_harm_header_sizeof", "bl_harm_cells_sizeof", "bl_snapshot_open_raw", "bl_snapshot_harm_header", "bl_snapshot_harm_prims",
                 "bl_set_grid_device_harm", "bl_set_grid_slice_device_harm", "bl_harm_convert_device"):
        assert hasattr(L, name), name
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_harm_header", "bl_harm_cells", "bl_set_grid_device_harm", "bl_set_grid_slice_device_harm", "bl_harm_convert_device", "bl_snapshot_open_raw"):
        assert name in header, name
    assert C.sizeof(_capi.HarmHeader) == L.bl_harm_header_sizeof() == 184
    assert C.sizeof(_capi.HarmCells) == L.bl_harm_cells_sizeof() == 32
    assert C.sizeof(_capi.DeviceCells) == L.bl_device_cells_sizeof() == 48   # bl_device_cells stays what it is


@pytest.mark.parametrize("kind", ["mks", "fmks"])
def test_fixture_through_the_raw_reader_equals_the_reader(built_library, kind):
    from blacklight_amd import Snapshot
    from blacklight_amd.snapshot import HarmGrid
    p = fixture_params(kind)
    with Snapshot(p) as snap:
        want = snap.arrays()
        d = snap.desc()
        want_scalars = {f: getattr(d, f) for f in ("n_blocks", "n_i", "n_j", "n_k", "n_var", "plasma_gamma", "plasma_gamma_i", "plasma_gamma_e",
                                                   "sks_map_n1", "sks_map_n2", "sks_map_r_in", "sks_map_dr", "sks_map_dtheta", "n_3_root")}
        want_bounds = list(d.simulation_bounds)
        want_map = None
        if kind == "fmks":
            want_map = np.ctypeslib.as_array(C.cast(d.sks_map, C.POINTER(C.c_double)), (2, d.sks_map_n2, d.sks_map_n1)).copy()
        want_warnings, want_time = snap.warnings, snap.time
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
        assert raw.desc().prim is None and raw.time == want_time and raw.warnings == want_warnings
    assert prims.dtype == np.float32 and prims.shape == (header.n1, header.n2, header.n3, header.n_prim)
    assert header.metric == (1 if kind == "fmks" else 0)
    grid = HarmGrid(p, header)
    assert grid.warnings == want_warnings and grid.planes == 8
    # cells: the planes of the host conversion are the reader's, byte for byte
    planes = grid.convert_host(prims)
    assert planes.shape == (8, header.n3, header.n2, header.n1)
    for q, name in enumerate(INDICES):
        assert same_bytes(planes[q], want["prim"][want["indices"][name], 0]), name
    # ... and they are no copy of the input: the vectors moved, the internal energy became a pressure
    assert not same_bytes(planes[2], np.ascontiguousarray(prims[..., header.ind_u1].transpose(2, 1, 0)))
    assert not same_bytes(planes[1], np.ascontiguousarray(prims[..., header.ind_uu].transpose(2, 1, 0)))
    assert same_bytes(planes[0], np.ascontiguousarray(prims[..., header.ind_rho].transpose(2, 1, 0)))
    # geometry: coordinates, variable and adiabatic indices, bounds, map
    g = grid.desc()
    assert g.prim is None
    for f, value in want_scalars.items():
        assert getattr(g, f) == value, f
    for name in INDICES + ("ind_kappa",):
        assert getattr(g, name) == want["indices"][name], name
    for name, n in zip(COORDINATES, (g.n_i + 1, g.n_j + 1, g.n_k + 1, g.n_i, g.n_j, g.n_k)):
        got = np.ctypeslib.as_array(C.cast(getattr(g, name), C.POINTER(C.c_double)), (n,))
        assert same_bytes(got, want[name][0]), name
    assert list(g.simulation_bounds) == want_bounds
    if kind == "fmks":
        got_map = np.ctypeslib.as_array(C.cast(g.sks_map, C.POINTER(C.c_double)), (2, g.sks_map_n2, g.sks_map_n1))
        assert same_bytes(got_map, want_map)
    else:
        assert g.sks_map is None
    converted = grid.desc(converted=True)
    assert converted.n_var == 8 and [getattr(converted, name) for name in INDICES] == list(range(8))
    grid.close()


def test_warnings_are_the_readers(built_library):
    from blacklight_amd import Snapshot
    from blacklight_amd.snapshot import HarmGrid
    p = fixture_params("mks", "spin")
    with Snapshot(p) as snap:
        want, want_gamma = snap.warnings, snap.desc().plasma_gamma
    assert "Given spin of" in want and "adiabatic index" in want
    with Snapshot(p, raw=True) as raw:
        grid = HarmGrid(p, raw.harm_header)
    assert grid.warnings == want and grid.desc().plasma_gamma == want_gamma
    given = grid.header.n1
    header = grid.header
    mine = type(header).from_buffer_copy(header)
    other = HarmGrid(p, mine)
    mine.n1 = given + 5   # the grid keeps a copy of the header it was made from
    assert other.shape[0] == given and other.desc().n_i == given


def test_entropy_plane_with_code_kappa(built_library):
    """plasma_model = code_kappa: a ninth plane, the entropy variable copied where the header says it lies (here: a second look at RHO)"""
    from blacklight_amd import Snapshot
    from blacklight_amd.snapshot import HarmGrid
    p = fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="RHO")
    with Snapshot(p, raw=True) as raw:
        header, prims = raw.harm_header, raw.harm_prims()
    assert header.ind_kappa == header.ind_rho
    grid = HarmGrid(p, header)
    planes = grid.convert_host(prims)
    assert grid.planes == 9 and planes.shape[0] == 9 and grid.desc().ind_kappa == header.ind_rho and grid.desc(converted=True).ind_kappa == 8
    assert same_bytes(planes[8], np.ascontiguousarray(prims[..., header.ind_rho].transpose(2, 1, 0)))
    with Snapshot(p) as snap:   # ... which is the plane the reader's description names
        arrays = snap.arrays()
    assert same_bytes(planes[8], arrays["prim"][arrays["indices"]["ind_kappa"], 0])


def test_refusals(built_library):
    import copy
    from blacklight_amd import BlacklightError, Snapshot
    from blacklight_amd.snapshot import HarmGrid
    p = fixture_params("mks")
    with Snapshot(p, raw=True) as raw:
        good = raw.harm_header

    def refused(match, params=p, **changes):
        header = copy.copy(good)
        for key, value in changes.items():
            setattr(header, key, value)
        with pytest.raises(BlacklightError, match=match) as caught:
            HarmGrid(params, header)
        return caught.value

    assert refused("Array dimension mismatch.", n2=0).code == 1
    refused("Array dimension mismatch.", n1=65537)
    refused("Array dimension mismatch.", n3=-4)
    refused('Unable to locate "RHO" slice of "prims" in data file.', ind_rho=-1)
    refused('Unable to locate "U2" slice of "prims" in data file.', ind_u2=good.n_prim)
    refused('Unable to locate "B3" slice of "prims" in data file.', ind_b3=-1)
    refused("Inconsistency in number of primitive variables.", n_prim=0)
    refused("Could not find total adiabatic index in input or data file.", params=fixture_params("mks", plasma_gamma=None), gam=float("nan"))
    assert refused("simulation_coord = fmks needs a file whose header/metric is FMKS or MMKS.", params=fixture_params("mks", simulation_coord="fmks")).code == 3
    refused("Invalid simulation_coord for Harm format.", params=fixture_params("mks", simulation_coord="cks"))
    refused("Unable to locate electron entropy slice", params=fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="KEL"))
    kappa = fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="RHO")
    for aliased in (good.ind_uu, good.ind_u1, good.ind_b3):
        assert refused("ind_kappa names the internal energy or a vector component", params=kappa, ind_kappa=aliased).code == 3
    # the raw reader refuses what the reader refuses, and every other format
    with pytest.raises(BlacklightError, match="electron entropy slice"):
        Snapshot(fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="KEL"), raw=True)
    fx, params, _ = gu.load_case("sim_dp_interp")
    from blacklight_amd import Params
    with pytest.raises(BlacklightError, match="iharm3d only"):
        Snapshot(Params.from_dict(dict(params, simulation_file=os.path.join(READER_DIR, "series_0003.athdf"))), raw=True)
    with Snapshot(p) as ordinary:
        with pytest.raises(BlacklightError, match="raw=True"):
            ordinary.harm_header


def test_device_calls_on_a_host_only_context(built_library):
    """What is decided before anything is launched: the description's refusals with their texts, then the host-only context's own"""
    from blacklight_amd import Context, Snapshot, _capi
    from blacklight_amd.snapshot import HarmGrid
    p = fixture_params("mks")
    with Snapshot(p, raw=True) as raw:
        header = raw.harm_header
    grid = HarmGrid(p, header)
    needed = header.n1 * header.n2 * header.n3 * header.n_prim
    L = _capi.lib()
    with Context(p, device=-2) as ctx:
        def call(which, prim=0x10000, dtype=0, n_elements=needed, cells=True, handle=grid.handle):
            c = _capi.HarmCells()
            c.prim, c.dtype, c.n_elements = prim or None, dtype, n_elements
            handed = C.byref(c) if cells else None
            if which == "set":
                rc = L.bl_set_grid_device_harm(ctx._ctx, handle, handed)
            elif which == "slice":
                rc = L.bl_set_grid_slice_device_harm(ctx._ctx, 0, handle, handed, 0.0)
            else:
                rc = L.bl_harm_convert_device(ctx._ctx, handle, handed, 0x20000)
            return rc, L.bl_last_error(ctx._ctx).decode()

        for which in ("set", "slice", "convert"):
            assert call(which, cells=False) == (5, "Error: bl_harm_cells: the description is NULL.\n")
            assert call(which, handle=None) == (5, "Error: bl_harm_cells: the grid is NULL.\n")
            assert call(which, prim=0) == (5, "Error: bl_harm_cells: prim is NULL.\n")
            assert call(which, dtype=2) == (5, "Error: bl_harm_cells: dtype must be BL_CELLS_F32 or BL_CELLS_F64.\n")
            assert call(which, prim=0x10004, dtype=1) == (5, "Error: bl_harm_cells: prim is not aligned to its element type.\n")
            assert call(which, n_elements=needed - 1) == (5, "Error: bl_harm_cells: n_elements is smaller than n1 * n2 * n3 * n_prim.\n")
        # a grid made under another plasma model than the context's
        entropy_header = type(header).from_buffer_copy(header)
        entropy_header.ind_kappa = header.ind_rho
        with_entropy = HarmGrid(fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="RHO"), entropy_header)
        mismatch = "Error: bl_harm_grid: made with another plasma_model than the context's (one of them reads the electron entropy, plasma_model = code_kappa).\n"
        assert call("set", handle=with_entropy.handle) == (5, mismatch)
        with Context(fixture_params("mks", plasma_model="code_kappa", simulation_kappa_name="RHO"), device=-2) as kappa_ctx:
            c = _capi.HarmCells()
            c.prim, c.dtype, c.n_elements = 0x10000, 0, needed
            assert L.bl_set_grid_device_harm(kappa_ctx._ctx, grid.handle, C.byref(c)) == 5 and L.bl_last_error(kappa_ctx._ctx).decode() == mismatch
            assert L.bl_set_grid_device_harm(kappa_ctx._ctx, with_entropy.handle, C.byref(c)) == 4
        assert call("set") == (4, "Error: Host-only context: no HIP device selected (the hot path has no CPU fallback).\n")
        assert call("convert") == (4, "Error: Host-only context: no HIP device selected (the hot path has no CPU fallback).\n")
        assert L.bl_grid_host_bytes(ctx._ctx) == 0
        # Python refuses what is no device tensor before the C call
        import torch
        prims = np.zeros(grid.shape, dtype=np.float32)
        for bad in (prims, torch.from_numpy(prims)):
            for method in (ctx.set_grid_device_harm, ctx.harm_convert_device):
                with pytest.raises(ValueError):
                    method(grid, bad)
