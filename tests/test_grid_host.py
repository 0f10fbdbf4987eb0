"""The grid set-up without a GPU (blacklight_amd/csrc/bl_grid.cpp through tests/grid_host_main.cpp): a description's arrays go to a flat
file, the program calls BuildGridTables and prints the refusal or a dump of every table and scalar. Held to: the Python restatements of
the three LDS budgets (tests/test_gpu_table_budgets.py, imported); one grid described as one block and as eight; the lattice, the
blocks' rows, the (level, location) hash and the bucket tables read the way a kernel reads them, in numpy; every refusal's code and
text as bl_set_grid always gave them; and digests recorded from the set-up code as it was before it moved into bl_grid.cpp
(tests/golden/grid_tables.json). Once built plainly, once under AddressSanitizer and UndefinedBehaviorSanitizer.

Grids: blacklight_amd.mock.generate through golden_util's split_grid, refined_grid and subdivide_blocks at the sizes of
test_gpu_table_budgets.py, and the iharm3d FMKS dump of tests/golden/reader.

Not reached: "Multi-block grid too large for the block lattice of this build." asks for more than 2^28 boxes or 2^32 cells. Along an
axis there are at most two distinct boundaries per block, so 2^28 boxes take at least 323 blocks none of which shares a boundary with
another on any axis - no mesh of the generators above - and the lattice of such a grid alone is a gigabyte on the host."""
import concurrent.futures
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
from blacklight_amd import build as bl_build
from test_gpu_table_budgets import BLOCK_INTERP, MESHES, N_STAGED, _lds_table_bytes, _mesh, _mesh_bytes, _single_block

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
GOLDEN = os.path.join(gu.GOLDEN_DIR, "grid_tables.json")
E_UNSUPPORTED, E_ARG = 3, 5                      # include/blacklight_amd.h
COORD_SKS, COORD_FMKS, CODE_KAPPA = 1, 2, 1
COORDS = ("x1f", "x2f", "x3f", "x1v", "x2v", "x3v")
# bl_set_grid's refusals, word for word
BAD_GRID = "Bad grid description."
BAD_MESH = "Multi-block grid has blocks that overlap or faces that do not ascend."
BAD_INDEX = "Grid variable index out of range."
BAD_FMKS = "simulation_coord = fmks needs a single block and the reader's sks_map in bl_grid_desc."
NO_TABLE = "simulation_block_interp = true needs the MeshBlock table (levels, locations, n_3_root) in bl_grid_desc."
BAD_LEVEL = "Bad MeshBlock level."
BAD_LOCATION = "MeshBlock location outside the range of this build."
TOO_MANY = "More than 65535 cells along an axis of the merged grid."
SLOW_BUDGET = "Slow light on a grid whose coordinate tables exceed the 60 KiB LDS budget is not built."


def _build(directory, extra):
    """The stand-alone program from its two translation units (side by side), with the host compiler. The library's headers name HIP
    types, so the HIP headers are on the include path; nothing of HIP is linked."""
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(bl_build.hipcc()))), "include")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{hip_include}", f"-I{bl_build.INCLUDE}", f"-I{bl_build.CSRC}"]
    sources = [os.path.join(REPO, "tests", "grid_host_main.cpp"), os.path.join(bl_build.CSRC, "bl_grid.cpp")]
    objects = [os.path.join(directory, os.path.basename(src)[:-4] + ".o") for src in sources]
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
        runs = list(pool.map(lambda pair: subprocess.run(["g++", "-c", pair[0], "-o", pair[1]] + flags + extra, capture_output=True, text=True),
                             zip(sources, objects)))
    for run in runs:
        assert run.returncode == 0, run.stderr
    program = os.path.join(directory, "grid_host_main")
    run = subprocess.run(["g++", "-o", program] + objects + extra, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return program


# ---- descriptions ------------------------------------------------------------------------------------------------------------------
def describe(grid, **params):
    """A mock Grid as the dict that write_description() takes: geometry, MeshBlock table, indices as Grid.desc() sets them, no cells"""
    n_var, n_b, n_k, n_j, n_i = grid.prim.shape
    d = dict(n_blocks=n_b, n_i=n_i, n_j=n_j, n_k=n_k, n_var=n_var, indices=[0, 1, max(grid.ind_kappa, 0), 2, 3, 4, 5, 6, 7],
             n_3_root=int(grid.n_3_root) if grid.levels is not None else 0, levels=grid.levels, locations=grid.locations, sks=None, prim=None,
             params=dict(interp=1, block_interp=0, coord=COORD_SKS, plasma_model=0, slow=0))
    d.update({name: getattr(grid, name) for name in COORDS})
    d["params"].update(params)
    return d


def write_description(path, d):
    """grid_host_main.cpp, ReadDescription: int32 head[32], float64 scalars[12], then the arrays that are there"""
    sks = d["sks"]
    present = sum(1 << a for a, name in enumerate(COORDS) if d[name] is not None)
    present |= (64 if d["levels"] is not None else 0) | (128 if d["locations"] is not None else 0) | (256 if sks else 0) | (512 if d["prim"] is not None else 0)
    p = d["params"]
    head = [d["n_blocks"], d["n_i"], d["n_j"], d["n_k"], d["n_var"]] + list(d["indices"]) + [d["n_3_root"]]
    head += [sks["n1"] if sks else 0, sks["n2"] if sks else 0, present, p["interp"], p["block_interp"], p["coord"], p["plasma_model"], p["slow"]]
    scalars = [0.0, 0.0, 0.0] + ([sks["r_in"], sks["dr"], sks["dtheta"]] + list(sks["bounds"]) if sks else [0.0] * 9)
    with open(path, "wb") as f:
        np.array(head + [0] * (32 - len(head)), dtype="<i4").tofile(f)
        np.array(scalars, dtype="<f8").tofile(f)
        for name in COORDS:
            if d[name] is not None:
                np.ascontiguousarray(d[name], dtype="<f8").tofile(f)
        for name in ("levels", "locations"):
            if d[name] is not None:
                np.ascontiguousarray(d[name], dtype="<i4").tofile(f)
        if sks:
            np.ascontiguousarray(sks["map"], dtype="<f8").tofile(f)
        if d["prim"] is not None:
            np.ascontiguousarray(d["prim"], dtype="<f4").tofile(f)


def fmks_description():
    """The grid of the FMKS goldens (tests/golden/reader/iharm3d_fmks.h5) as the reader hands it over"""
    import ctypes as C
    from blacklight_amd import Params, Snapshot
    fx = np.load(os.path.join(gu.GOLDEN_DIR, "reader", "expected_fmks.npz"), allow_pickle=False)
    params = json.loads(str(fx["interp_params"]))
    params["simulation_file"] = os.path.join(gu.GOLDEN_DIR, "reader", "iharm3d_fmks.h5")
    with Snapshot(Params.from_dict({k: v for k, v in params.items() if v is not None})) as s:
        g, arrays = s.desc(), s.arrays()
        sks = dict(n1=g.sks_map_n1, n2=g.sks_map_n2, r_in=g.sks_map_r_in, dr=g.sks_map_dr, dtheta=g.sks_map_dtheta, bounds=list(g.simulation_bounds),
                   map=np.ctypeslib.as_array(C.cast(g.sks_map, C.POINTER(C.c_double)), shape=(2, g.sks_map_n2, g.sks_map_n1)).copy())
        d = dict(n_blocks=g.n_blocks, n_i=g.n_i, n_j=g.n_j, n_k=g.n_k, n_var=g.n_var, indices=[arrays["indices"][k] for k in
                 ("ind_rho", "ind_pgas", "ind_kappa", "ind_uu1", "ind_uu2", "ind_uu3", "ind_bb1", "ind_bb2", "ind_bb3")],
                 n_3_root=g.n_3_root, levels=None, locations=None, sks=sks, prim=None,
                 params=dict(interp=1, block_interp=0, coord=COORD_FMKS, plasma_model=0, slow=0))
    d.update({name: arrays[name] for name in COORDS})
    return d


def golden_cases():
    """name -> description, for the digests of tests/golden/grid_tables.json"""
    cases = {"one_block": lambda: describe(_single_block(N_STAGED + 1)), "eight_blocks": lambda: describe(_single_block(N_STAGED + 1, (2, 2, 2)))}
    for name in sorted(MESHES):
        cases["mesh_" + name] = lambda name=name: describe(_mesh(*MESHES[name][:2]))
    cases["mesh_block_interp"] = lambda: describe(_mesh(*BLOCK_INTERP["1024_lanes"][:2]), block_interp=1)
    cases["fmks"] = fmks_description
    return cases


# ---- the program's output ------------------------------------------------------------------------------------------------------------
def run_program(program, d, directory, name, tables=False):
    """(exit code, the dump parsed, the output's lines)"""
    path = os.path.join(str(directory), name + ".grid")
    write_description(path, d)
    run = subprocess.run([program, path] + ([path] if tables else []), capture_output=True, text=True, timeout=300)
    assert run.returncode in (0, 2), run.stdout[-2000:] + run.stderr[-4000:]   # (anything else: a crash, or a sanitizer's report)
    lines = run.stdout.splitlines()
    out = dict(path=path, tables={}, dev={}, lines=lines)
    if run.returncode == 2:
        _, code, text = lines[0].split(" ", 2)
        out["refused"] = (int(code), text)
        return out
    assert lines[0] == "ok"
    for line in lines[1:]:
        words = line.split()
        if words[0] == "table":
            out["tables"][words[1]] = (int(words[2]), words[3])
        elif words[0] == "dev":
            out["dev"][words[1]] = words[2:]
        else:
            out[words[0]] = words[1:]
    return out


def ints(out, name):
    return [int(w) for w in out["dev"][name]]


def doubles(out, name):
    return np.array([int(w, 16) for w in out["dev"][name]], dtype=np.uint64).view(np.float64)


def table(out, name, dtype):
    return np.fromfile(out["path"] + "." + name, dtype=dtype)


def refusal(program, d, directory, name):
    out = run_program(program, d, directory, name)
    assert "refused" in out, out["lines"][:3]
    return out["refused"]


@pytest.fixture(scope="module")
def plain_program(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("grid_host")), [])


# ---- budgets -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_r", [N_STAGED, N_STAGED + 1])
def test_lds_table_bytes(plain_program, n_r, tmp_path):
    out = run_program(plain_program, describe(_single_block(n_r)), tmp_path, "one")
    staged = (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16
    assert int(out["lds_table_bytes"][0]) == (staged if n_r == N_STAGED else 0)
    assert ints(out, "n_blocks") == [0] and ints(out, "n") == [n_r, 8, 8]


@pytest.mark.parametrize("name", sorted(MESHES))
def test_mesh_bytes(plain_program, name, tmp_path):
    block, split, refined, fused = MESHES[name]
    out = run_program(plain_program, describe(_mesh(block, split)), tmp_path, name)
    assert (ints(out, "refined_lds_bytes")[0], ints(out, "fused_lds_bytes")[0]) == _mesh_bytes(block, split) == (refined, fused)
    assert ints(out, "n_blocks") == [36 * split[0] * split[1] * split[2]] and int(out["lds_table_bytes"][0]) == 0
    assert ("fused_desc" in out["tables"]) == (fused != 0)


def test_mesh_bytes_with_the_block_table(plain_program, tmp_path):
    """8 x 6 x 8 cells split 4 x 2 x 2 with inter-block interpolation: the MeshBlock table and its hash count"""
    block, split, refined, _ = BLOCK_INTERP["1024_lanes"]
    out = run_program(plain_program, describe(_mesh(block, split), block_interp=1), tmp_path, "interp")
    assert ints(out, "refined_lds_bytes")[0] == _mesh_bytes(block, split, True)[0] == refined == 62552
    assert ints(out, "block_interp") == [1] and ints(out, "hash_mask") == [2047] and ints(out, "max_level") == [1]


# ---- one grid, two descriptions ------------------------------------------------------------------------------------------------------
def test_one_block_and_eight_give_the_same_tables(plain_program, tmp_path):
    n_r = N_STAGED + 1
    eight_grid = _single_block(n_r, (2, 2, 2))
    one = run_program(plain_program, describe(_single_block(n_r)), tmp_path, "one", tables=True)
    eight = run_program(plain_program, describe(eight_grid), tmp_path, "eight", tables=True)
    names = [f"{t}{a}" for t in ("xf", "xv", "bucket") for a in range(3)] + ["angle_trig0", "angle_trig1"]
    assert set(names) <= set(one["tables"]) and one["tables"]["xf0"][0] == n_r + 1
    for name in names:
        assert one["tables"][name] == eight["tables"][name], name
    for name in one["dev"]:
        if name != "nb":
            assert one["dev"][name] == eight["dev"][name], name
    assert ints(one, "nb") == [n_r, 8, 8] and ints(eight, "nb") == [n_r // 2, 4, 4]
    assert ints(eight, "stride_row") == [n_r] and ints(eight, "stride_plane") == [n_r * 8] and ints(eight, "n") == [n_r, 8, 8]
    assert one["lds_table_bytes"] == eight["lds_table_bytes"] and one["outer_x1"] == eight["outer_x1"]
    assert one["merged_blocks"] == ["1", "1", "1"] and eight["merged_blocks"] == ["2", "2", "2"]
    assert "has_origin 0" in " ".join(one["placement"]) and "has_origin 1" in " ".join(eight["placement"])
    # a block's first cell where numpy's indices put it; merged_block_at inverts the file's permutation
    origin, block_at = table(eight, "origin", "<u8"), table(eight, "merged_block_at", "<i4")
    assert origin.size == block_at.size == 8
    for blk, (bi, bj, bk) in enumerate(eight_grid.locations):
        assert origin[blk] == np.ravel_multi_index((bk * 4, bj * 4, bi * (n_r // 2)), (8, 8, n_r))
        assert block_at[np.ravel_multi_index((bk, bj, bi), (2, 2, 2))] == blk
    # the coordinate tables are the single block's arrays themselves
    grid = _single_block(n_r)
    for a, name in enumerate(("x1", "x2", "x3")):
        assert np.array_equal(table(eight, f"xf{a}", "<f8").view(np.uint64), getattr(grid, name + "f")[0].view(np.uint64))
        assert np.array_equal(table(eight, f"xv{a}", "<f8").view(np.uint64), getattr(grid, name + "v")[0].view(np.uint64))


def test_kappa_plane_of_eight_blocks_is_the_single_block_plane(plain_program, tmp_path):
    """plasma_model = code_kappa on a merged grid of several blocks: the one plane the host repacks"""
    from blacklight_amd import mock
    one_grid = mock.with_entropy(mock.generate(n_r=16, n_th=8, n_ph=8))
    eight_grid = gu.split_grid(one_grid, 2, 2, 2)
    d = describe(eight_grid, plasma_model=CODE_KAPPA)
    d["prim"] = eight_grid.prim
    out = run_program(plain_program, d, tmp_path, "kappa", tables=True)
    assert np.array_equal(table(out, "kappa", "<f4").view(np.uint32), one_grid.prim[8, 0].reshape(-1).view(np.uint32))


# ---- the tables as a kernel reads them -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["36k_64k", "hbm_none", "block_interp", "hole"])
def test_lattice_rows_and_hash(plain_program, name, tmp_path):
    if name == "hole":
        grid = _drop_block(_single_block(16, (2, 2, 2)), 3)
    else:
        grid = _mesh(*(BLOCK_INTERP["1024_lanes"][:2] if name == "block_interp" else MESHES[name][:2]))
    out = run_program(plain_program, describe(grid, block_interp=int(name == "block_interp")), tmp_path, name, tables=True)
    n_b, nb, n_edge, n_rows = grid.prim.shape[1], ints(out, "nb"), ints(out, "n_edge"), ints(out, "n_rows")
    assert ints(out, "n_blocks") == [n_b] and nb == list(grid.prim.shape[:1:-1])
    lattice = table(out, "lattice", "<i4").reshape(n_edge[2], n_edge[1], n_edge[0])
    edges = [table(out, f"edge{a}", "<f8") for a in range(3)]
    centres, faces = [grid.x1v, grid.x2v, grid.x3v], [grid.x1f, grid.x2f, grid.x3f]
    # every cell centre of every block, looked up through `edge` and `lattice`, names its block
    box = [np.searchsorted(edges[a], centres[a], side="right") - 1 for a in range(3)]   # [n_b][nb[a]]
    found = lattice[box[2][:, :, None, None], box[1][:, None, :, None], box[0][:, None, None, :]]
    assert np.array_equal(found, np.broadcast_to(np.arange(n_b)[:, None, None, None], found.shape))
    assert (lattice == -1).sum() == (1 if name == "hole" else 0)
    if name == "hole":
        assert ints(out, "fused_lds_bytes") == [0] and "fused_desc" not in out["tables"]
    # block_row points at a row whose bits are the block's own
    for a in range(3):
        rows = table(out, f"block_row{a}", "<i4")
        bxf, bxv = table(out, f"bxf{a}", "<f8").reshape(n_rows[a], nb[a] + 1), table(out, f"bxv{a}", "<f8").reshape(n_rows[a], nb[a])
        assert rows.min() == 0 and rows.max() == n_rows[a] - 1
        assert np.array_equal(bxf[rows].view(np.uint64), faces[a].view(np.uint64)) and np.array_equal(bxv[rows].view(np.uint64), centres[a].view(np.uint64))
        assert np.array_equal(doubles(out, "edge_first")[a:a + 1], edges[a][:1]) and np.array_equal(doubles(out, "edge_last")[a:a + 1], edges[a][-1:])
    # each (level, location) probes to its block through the hash
    if name == "block_interp":
        mask = ints(out, "hash_mask")[0]
        keys, blocks = table(out, "hash_keys", "<u8"), table(out, "hash_blocks", "<i4")
        assert np.array_equal(table(out, "levels", "<i4"), grid.levels) and np.array_equal(table(out, "locations", "<i4").reshape(-1, 3), grid.locations)
        for blk in range(n_b):
            loc = [int(v) for v in grid.locations[blk]]
            key = (int(grid.levels[blk]) << 57) | (loc[0] << 38) | (loc[1] << 19) | loc[2]
            slot = (((key * 0x9e3779b97f4a7c15) & (2 ** 64 - 1)) >> 32) & mask
            while int(keys[slot]) != key:
                assert int(keys[slot]) != 2 ** 64 - 1, blk
                slot = (slot + 1) & mask
            assert blocks[slot] == blk
        assert (keys != np.uint64(2 ** 64 - 1)).sum() == n_b


def test_bucket_entries_reach_the_cell(plain_program, tmp_path):
    """A bucket's entry, walked forward over the faces, reaches the cell np.searchsorted gives, and never starts beyond it"""
    n_r = N_STAGED + 1
    out = run_program(plain_program, describe(_single_block(n_r, (2, 2, 2))), tmp_path, "eight", tables=True)
    x0, inv_w, n_bucket = doubles(out, "bucket_x0"), doubles(out, "bucket_inv_w"), ints(out, "n_bucket")
    rng = np.random.default_rng(11)
    for a in range(3):
        xf, bucket = table(out, f"xf{a}", "<f8"), table(out, f"bucket{a}", "<u2")
        n = xf.size - 1
        assert bucket.size == n_bucket[a] == max(512, 8 * n)
        x = np.concatenate([rng.uniform(xf[0], xf[-1], 990), xf[:5], xf[-6:-1]])
        want = np.clip(np.searchsorted(xf, x, side="right") - 1, 0, n - 1)
        start = bucket[np.clip(((x - x0[a]) * inv_w[a]).astype(np.int64), 0, n_bucket[a] - 1)].astype(np.int64)
        assert (start <= want).all()
        for c, w, point in zip(start, want, x):
            while c < n - 1 and point >= xf[c + 1]:
                c += 1
            assert c == w


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _drop_block(grid, blk):
    keep = [b for b in range(grid.prim.shape[1]) if b != blk]
    return dataclasses.replace(grid, prim=np.ascontiguousarray(grid.prim[:, keep]), levels=np.ascontiguousarray(grid.levels[keep]),
                               locations=np.ascontiguousarray(grid.locations[keep]), **{name: np.ascontiguousarray(getattr(grid, name)[keep]) for name in COORDS})


def _duplicate_block(grid):
    """Block 1 lies where block 0 does"""
    return dataclasses.replace(grid, **{name: np.ascontiguousarray(np.concatenate([getattr(grid, name)[:1], getattr(grid, name)[:1], getattr(grid, name)[2:]]))
                                        for name in COORDS})


def check_refusals(program, directory):
    from blacklight_amd import mock
    small, eight = _single_block(16), _single_block(16, (2, 2, 2))
    d = describe(small)
    assert refusal(program, dict(d, n_blocks=0), directory, "no_blocks") == (E_ARG, BAD_GRID)
    assert refusal(program, dict(d, n_k=1, x3f=d["x3f"][:, :2], x3v=d["x3v"][:, :1]), directory, "one_cell") == (E_ARG, BAD_GRID)
    assert refusal(program, dict(d, x2v=None), directory, "no_centres") == (E_ARG, BAD_GRID)
    assert refusal(program, describe(_duplicate_block(eight)), directory, "duplicate") == (E_UNSUPPORTED, BAD_MESH)
    descending = describe(eight)
    descending["x1f"] = descending["x1f"].copy()
    descending["x1f"][5] = descending["x1f"][5][::-1]
    assert refusal(program, descending, directory, "descending") == (E_UNSUPPORTED, BAD_MESH)
    for at in (0, 8):   # (ind_rho, ind_bb3)
        indices = list(d["indices"])
        indices[at] = d["n_var"]
        assert refusal(program, dict(d, indices=indices), directory, "index") == (E_ARG, BAD_INDEX)
    kappa = dict(describe(small, plasma_model=CODE_KAPPA), indices=[0, 1, -1, 2, 3, 4, 5, 6, 7])
    assert refusal(program, kappa, directory, "kappa_index") == (E_ARG, BAD_INDEX)
    assert refusal(program, describe(small, coord=COORD_FMKS), directory, "fmks_no_map") == (E_ARG, BAD_FMKS)
    assert refusal(program, describe(eight, coord=COORD_FMKS), directory, "fmks_blocks") == (E_ARG, BAD_FMKS)
    interp = describe(eight, block_interp=1)
    assert "refused" not in run_program(program, interp, directory, "interp")
    assert refusal(program, dict(interp, levels=None), directory, "no_levels") == (E_ARG, NO_TABLE)
    assert refusal(program, dict(interp, n_3_root=0), directory, "no_root") == (E_ARG, NO_TABLE)
    assert refusal(program, dict(interp, levels=np.where(np.arange(8) == 2, 31, interp["levels"])), directory, "level") == (E_ARG, BAD_LEVEL)
    locations = interp["locations"].copy()
    locations[4, 1] = 1 << 19
    assert refusal(program, dict(interp, locations=locations), directory, "location") == (E_UNSUPPORTED, BAD_LOCATION)
    assert refusal(program, dict(interp, locations=np.zeros_like(locations)), directory, "one_place") == (E_UNSUPPORTED, BAD_MESH)
    assert refusal(program, describe(gu.single_block_table(mock.generate(n_r=65536, n_th=2, n_ph=2))), directory, "long") == (E_UNSUPPORTED, TOO_MANY)
    assert refusal(program, describe(_single_block(N_STAGED + 1), slow=1), directory, "slow") == (E_UNSUPPORTED, SLOW_BUDGET)
    assert "refused" not in run_program(program, describe(_single_block(N_STAGED), slow=1), directory, "slow_fits")
    # a tiling with a hole goes through the lattice
    hole = run_program(program, describe(_drop_block(eight, 3)), directory, "hole")
    assert "refused" not in hole and ints(hole, "n_blocks") == [7] and ints(hole, "fused_lds_bytes") == [0]
    # two faults at once: the one bl_set_grid reaches first
    bad = [0, 1, 0, 2, 3, 4, 5, 6, small.prim.shape[0]]
    assert refusal(program, dict(describe(_duplicate_block(eight)), indices=bad), directory, "duplicate_index") == (E_UNSUPPORTED, BAD_MESH)
    assert refusal(program, dict(describe(_drop_block(eight, 3)), indices=bad), directory, "hole_index") == (E_ARG, BAD_INDEX)


def test_refusals(plain_program, tmp_path):
    check_refusals(plain_program, tmp_path)


# ---- digests from before the move ----------------------------------------------------------------------------------------------------
def comparable(lines):
    """The dump's lines that the set-up code had a counterpart for before it moved (not: the memcmp's answer)"""
    return [line for line in lines[1:] if not line.startswith("same_geometry")]


def check_digests(program, directory, names=None):
    with open(GOLDEN) as f:
        golden = json.load(f)
    cases = golden_cases()
    assert set(golden) == set(cases)
    for name in names or sorted(cases):
        out = run_program(program, cases[name](), directory, name)
        assert "refused" not in out, out["lines"][:1]
        assert out["same_geometry"] == ["1"]
        assert comparable(out["lines"]) == golden[name], name


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_tables_are_those_of_the_code_before_the_move(plain_program, name, tmp_path):
    check_digests(plain_program, tmp_path, [name])


def test_the_same_under_host_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in (statically: a stand-alone binary, nothing
    preloaded): every refusal and every recorded grid. A report ends the program with another exit code than the two run_program takes."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + SANITIZE, capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the host toolchain cannot link the sanitizer runtimes: " + linked.stderr.strip().splitlines()[-1])
    program = _build(str(tmp_path), SANITIZE)
    check_refusals(program, tmp_path)
    check_digests(program, tmp_path)
