"""GPU: the LDS budgets of the grid's coordinate tables, at and across each limit. Every kernel that finds a sample's cell keeps the
tables in LDS when they fit and switches to another launch shape, other pointers or another kernel family when they do not; the
switches are byte thresholds compared on the host ("tables:"). Each case renders a small frame over a grid built
for one regime, checks on the `tables:` and `kernels:` debug lines that the render was in that regime - a case that drifts into another
fails instead of passing vacuously - and compares with the CPU oracle, which has no budgets.

Single block, n_r x 8 x 8 cells of blacklight_amd.mock.generate (the camera lies outside the grid, so every ray crosses the highest
radial cells on its way in and out):
  fused kernels      64 (n_r + 8 + 8) + 384 <= 64 KiB: n_r = 1002 is the last shape that fits, 1003 the first that does not
  lds_table_bytes    (2 n + 1) 8 + max(512, 8 n) 2 bytes per axis <= 60 KiB: n_r = 1847 stages, 1848 is searched in HBM

Meshes with refinement: refined_grid() of a 4 bi x 4 bj x 4 bk mock, every block cut by subdivide_blocks(). MESHES records the bytes
that the host computes for each (BlGridDevice::refined_lds_bytes, ::fused_lds_bytes), restated by _mesh_bytes() from the mesh's counts
and asserted against what the `tables:` line reports.

Not reached, and why:
  * bl_launch_locate's and bl_launch_shade_fused2's "1 block" branches (grid < 4, grid < 8): `grid` is a multiple of the device's
    compute units (16 x, 1 x and 8 x their number), whatever the frame; no device of eight or more units takes them.
  * the exact second pass with a mesh's tables beyond BL_REDO_TABLES_LDS *and* inter-block interpolation behind the fused kernel: that
    kernel asks for blocks of twelve cells per axis, so tables of 48 KiB take 576 blocks of 12^3 cells, a 192 x 96 x 96 grid. The second
    pass on tables in HBM is covered behind the fused kernel over every other grid here (redo=hbm)."""
import functools
import json

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

EXPECTED = 1.0e-11            # tests/test_gpu_tolerant.py: tolerant against exact tier, unpolarized
EXPECTED_POLARIZED = 1.0e-9   # ... and polarized (test_tolerant_tier_on_the_goldens)
KIB = 1024

# A camera of test_randomised_configurations_against_oracle's ranges that looks into the grid from outside it (r_max = 52.2)
CAMERA = dict(camera_type="plane", camera_r=60.0, camera_th=63.0, camera_ph=111.0, camera_rotation=-20.0, camera_width=30.0,
              fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)
FOUR_FREQUENCIES = dict(image_num_frequencies=4, image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log")


def _distance(a, b):   # (tests/test_gpu_tolerant.py)
    scale = np.nanmax(np.abs(b), axis=-1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / scale
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def _params(polarized=False, **over):
    fx, params, mock_args = gu.load_case("sim_polarized" if polarized else "sim_dp_interp")
    params = dict(params, simulation_interp="true", camera_resolution=12 if polarized else 16)
    params.update(CAMERA)
    params.update(over)
    if int(params["image_num_frequencies"]) > 1:
        params.pop("image_frequency", None)
    return params


@functools.lru_cache(maxsize=None)
def _single_block(n_r, blocks=None):
    from blacklight_amd import mock
    grid = mock.generate(n_r=n_r, n_th=8, n_ph=8)
    return gu.split_grid(grid, *blocks) if blocks else gu.single_block_table(grid)


@functools.lru_cache(maxsize=None)
def _mesh(block, split):
    from blacklight_amd import mock
    bi, bj, bk = block
    grid = mock.generate(n_r=4 * bi, n_th=4 * bj, n_ph=4 * bk)
    # (a fine block that this camera's rays sample goes last in the file, so that the upper end of every per-block table is read)
    return gu.subdivide_blocks(gu.refined_grid(grid, last=(1, 1, 1, 1), block=block), split)


_oracle_cache = {}


def _oracle(params, grid, key):
    """The CPU oracle's render, once per (parameters, grid)"""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    key = (json.dumps(params, sort_keys=True), key)
    if key not in _oracle_cache:
        p = bl.Params.from_dict(params)
        res = int(params["camera_resolution"])
        _oracle_cache[key] = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=res * res,
                                               max_steps=int(p.get("ray_max_steps")), n_freq=int(p.get("image_num_frequencies")))
    return _oracle_cache[key]


def _words(line):
    return dict(word.split("=", 1) if "=" in word else (word, "") for word in line.split())


def _stage(text):
    """A stage of the `tables:` line: where, bytes staged, lanes, workgroups of the first (and last) launch, 256-lane workgroups asked for"""
    text, _, last = text.partition(",@")
    place, _, shape = text.partition("x")
    where, _, nbytes = place.partition(":")
    out = dict(where=where, bytes=int(nbytes) if nbytes else 0)
    if shape:
        lanes, _, counts = shape.partition("@")
        blocks, _, grid = counts.partition("/")
        out.update(lanes=int(lanes), blocks=int(blocks), grid=int(grid))
    if last:
        out.update(last_blocks=int(last.split("/")[0]), last_grid=int(last.split("/")[1]))
    return out


def _render(ctx, capfd):
    """One render with its `kernels:` stages and its `tables:` stages"""
    capfd.readouterr()
    out = ctx.render()
    err = capfd.readouterr().err.splitlines()
    kernels = [line for line in err if line.startswith("kernels: ")]
    tables = [line for line in err if line.startswith("tables: ")]
    assert len(kernels) == 1 and len(tables) == 1, err
    out["kernels"] = _words(kernels[0][len("kernels: "):])
    out["tables"] = {name: _stage(text) for name, text in _words(tables[0][len("tables: "):]).items()}
    out["tables_line"] = tables[0]
    print(kernels[0], "|", tables[0])
    return out


def _context(monkeypatch, params, grid, undefined_policy=None):
    import blacklight_amd as bl
    monkeypatch.setenv("BLACKLIGHT_AMD_DEBUG_COUNTERS", "1")   # (read when the context is created)
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_geodesic_reuse(False)   # (every render runs every stage: a second render of a camera would shade the first one's located samples)
    if undefined_policy:
        ctx.set_undefined_policy(undefined_policy)
    ctx.set_grid(grid)
    return ctx


def _family(got):
    return got["kernels"]["shade"].split("<")[0]


def _check_exact(got, want):
    assert np.array_equal(got["sample_num"], want["sample_num"])
    assert np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["stats"].n_samples == want["n_samples"] and got["stats"].n_gathers == want["n_gathers"]
    same = gu.same_bits(got["image"], want["image"])
    assert same.all(), f"{(~same).sum()} of {same.size} values differ from the oracle"
    image = got["image"]
    assert np.isfinite(image).all() and (image[0] > 0.0).sum() > image.shape[1] // 2


def _check_tolerant(tol, exact, polarized=False):
    assert tol["stats"].arithmetic == 1
    assert np.array_equal(tol["sample_num"], exact["sample_num"]) and np.array_equal(tol["sample_flags"], exact["sample_flags"])
    assert np.array_equal(np.isnan(tol["image"]), np.isnan(exact["image"]))
    d = _distance(tol["image"], exact["image"])
    print(f"tolerant vs exact {d:.2e}")
    assert d < (EXPECTED_POLARIZED if polarized else EXPECTED)


def _inside(got, nbytes, lanes=256):
    """The coefficient kernel has the locate step inside, over `nbytes` of tables in LDS, and no locate kernel runs"""
    t = got["tables"]
    assert t["locate"]["where"] == "none" and got["kernels"]["locate"] == "none", got["tables_line"]
    assert (t["fused"]["where"], t["fused"]["bytes"], t["fused"]["lanes"]) == ("lds", nbytes, lanes), got["tables_line"]


def _outside(got, where, nbytes=0, lanes=256):
    """A locate kernel runs, on tables in `where`, and the coefficient kernel reads what it left"""
    t = got["tables"]
    assert t["fused"]["where"] == "none", got["tables_line"]
    assert (t["locate"]["where"], t["locate"]["bytes"], t["locate"]["lanes"]) == (where, nbytes, lanes), got["tables_line"]
    assert t["redo"]["where"] in ("none", "located"), got["tables_line"]


# ---- one block: the fused kernels' limit -------------------------------------------------------------------------------------------
N_FUSED_FITS = 1002   # 64 (1002 + 16) + 384 = 65 536
assert 64 * (N_FUSED_FITS + 16) + 384 == 64 * KIB


def _lds_table_bytes(n):
    """bl_grid.cpp: faces and centres as doubles, max(512, 8 n) 16-bit buckets per axis; rounded up to 16 where it is staged"""
    return sum((2 * m + 1) * 8 + max(512, 8 * m) * 2 for m in n)


@pytest.mark.parametrize("frequencies", [1, 4])
@pytest.mark.parametrize("spin", [0.0, 0.9])
@pytest.mark.parametrize("n_r", [N_FUSED_FITS, N_FUSED_FITS + 1])
def test_fused_kernels_single_block_limit(n_r, spin, frequencies, capfd, monkeypatch, built_library):
    """1018 cells summed over the axes fill the fused kernels' 64 KiB to the byte; one more and the render goes through
    bl_locate_plain_kernel and bl_shade_fast_kernel / bl_shade_exact_kernel. Both tiers, one frequency and four."""
    fits = n_r == N_FUSED_FITS
    params = _params(simulation_a=spin, **(FOUR_FREQUENCIES if frequencies == 4 else {}))
    grid = _single_block(n_r)
    want = _oracle(params, grid, n_r)
    staged = (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    z = int(spin == 0.0)
    if fits and frequencies == 1:
        assert exact["kernels"]["shade"] == f"exact2<{z}>"
        _inside(exact, 64 * KIB - 384)
    else:   # (the exact tier's kernel with the locate step inside takes one frequency only)
        assert exact["kernels"]["shade"] == f"exact<{z}>" and exact["kernels"]["locate"] == f"plain<{z}>"
        _outside(exact, "lds", staged)
    if fits:
        # (spin known at compile time or not; per-sample factors with four frequencies; one block)
        assert tol["kernels"]["shade"] in (f"fused2<{z},0,{int(frequencies == 4)},0>", f"fused2<{z},1,{int(frequencies == 4)},0>")
        _inside(tol, 64 * KIB)
        assert tol["tables"]["redo"]["where"] == "hbm"
    else:
        assert tol["kernels"]["shade"] == f"fast<{z},0>" and tol["kernels"]["locate"] == f"plain<{z}>"
        _outside(tol, "lds", staged)
        assert tol["tables"]["redo"]["where"] == "located"
    _check_exact(exact, want)
    _check_tolerant(tol, exact)


@pytest.mark.parametrize("spin", [0.0, 0.9])
@pytest.mark.parametrize("n_r", [N_FUSED_FITS, N_FUSED_FITS + 1])
def test_polarized_kernel_single_block_limit(n_r, spin, capfd, monkeypatch, built_library):
    params = _params(polarized=True, simulation_a=spin)
    grid = _single_block(n_r)
    want = _oracle(params, grid, n_r)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    for got in (exact, tol):
        if n_r == N_FUSED_FITS:
            assert _family(got) == "polarized2"
            _inside(got, 64 * KIB - 384)
        else:
            assert _family(got) == "shade" and got["kernels"]["locate"] == f"plain<{int(spin == 0.0)}>"
            _outside(got, "lds", (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16)
    _check_exact(exact, want)
    _check_tolerant(tol, exact, polarized=True)


# ---- one block: the locate kernels' 60 KiB -----------------------------------------------------------------------------------------
N_STAGED = max(n for n in range(1000, 3000) if _lds_table_bytes((n, 8, 8)) <= 60 * KIB)   # 32 n + 2 328 <= 61 440
assert N_STAGED == 1847 and _lds_table_bytes((N_STAGED + 1, 8, 8)) > 60 * KIB


@pytest.mark.parametrize("interp", ["true", "false"])
@pytest.mark.parametrize("spin", [0.0, 0.9])
@pytest.mark.parametrize("n_r", [N_STAGED, N_STAGED + 1])
def test_locate_tables_60_kib_limit(n_r, spin, interp, capfd, monkeypatch, built_library):
    """The last grid whose tables the locate kernels stage and the first that bl_locate_kernel<false, false, false, true> searches
    in HBM through flat pointers; trilinear and nearest sampling, both tiers."""
    params = _params(simulation_a=spin, simulation_interp=interp)
    grid = _single_block(n_r)
    want = _oracle(params, grid, n_r)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    z = int(spin == 0.0)
    for got in (exact, tol):
        if n_r == N_STAGED and interp == "true":
            assert got["kernels"]["locate"] == f"plain<{z}>"
            _outside(got, "lds", (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16)
        elif n_r == N_STAGED:   # (nearest sampling: the general kernel)
            assert got["kernels"]["locate"] == "general<0,0,0,0>"
            _outside(got, "lds", (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16)
        else:
            assert got["kernels"]["locate"] == "general<0,0,0,1>"
            _outside(got, "hbm")
    assert _family(exact) in ("exact", "shade") and _family(tol) == "fast"
    _check_exact(exact, want)
    _check_tolerant(tol, exact)


@pytest.mark.parametrize("variant", ["cut", "tau"])
@pytest.mark.parametrize("n_r", [N_STAGED, N_STAGED + 1])
def test_locate_tables_60_kib_limit_general_and_plain_kernel(n_r, variant, capfd, monkeypatch, built_library):
    """Below the limit a geometric cut takes the general locate kernel and an optical-depth image the plain one; above it both
    take the kernel that searches in HBM."""
    over = dict(cut_omit_near="true") if variant == "cut" else dict(image_tau="true")
    params = _params(simulation_a=0.9, **over)
    grid = _single_block(n_r)
    want = _oracle(params, grid, n_r)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    for got in (exact, tol):
        if n_r == N_STAGED:
            assert got["kernels"]["locate"] == ("general<0,0,0,0>" if variant == "cut" else "plain<0>")
            _outside(got, "lds", (_lds_table_bytes((n_r, 8, 8)) + 15) // 16 * 16)
        else:
            assert got["kernels"]["locate"] == "general<0,0,0,1>"
            _outside(got, "hbm")
    assert _family(tol) == "fast"
    _check_exact(exact, want)
    _check_tolerant(tol, exact)


def test_polarized_above_the_60_kib_limit(capfd, monkeypatch, built_library):
    params = _params(polarized=True, simulation_a=0.9)
    grid = _single_block(N_STAGED + 1)
    want = _oracle(params, grid, N_STAGED + 1)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    for got in (exact, tol):
        assert _family(got) == "shade" and got["kernels"]["locate"] == "general<0,0,0,1>"
        _outside(got, "hbm")
    _check_exact(exact, want)
    _check_tolerant(tol, exact, polarized=True)


def test_slow_light_above_the_60_kib_limit_is_refused(built_library):
    import blacklight_amd as bl
    fx, params, _ = gu.load_case("slow_interp")
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_grid_slice(0, _single_block(N_STAGED), 0.0)   # (the last grid that fits is taken)
        with pytest.raises(bl.BlacklightError, match="Slow light on a grid whose coordinate tables exceed the 60 KiB LDS budget is not built."):
            ctx.set_grid_slice(0, _single_block(N_STAGED + 1), 0.0)


@pytest.mark.parametrize("interp", ["false", "true"])
@pytest.mark.parametrize("spin", [0.0, 0.9])
def test_same_tables_as_equal_blocks(spin, interp, capfd, monkeypatch, built_library):
    """The grid above the limit as 2 x 2 x 2 equal blocks - the merged-grid path that split_grid() feeds: the same tables in HBM. With
    nearest sampling the same cells are read, so the render has the single block's bits. With trilinear sampling it has not, and must
    not: the reference interpolates within a MeshBlock (the oracle's two renders differ in 251 of 256 pixels); there the eight blocks
    are held to the oracle's render of the eight blocks."""
    params = _params(simulation_a=spin, simulation_interp=interp)
    n_r = N_STAGED + 1
    grids = dict(one=_single_block(n_r), eight=_single_block(n_r, (2, 2, 2)))
    out = {}
    for name, grid in grids.items():
        with _context(monkeypatch, params, grid) as ctx:
            for tier in ("exact", "tolerant"):
                ctx.set_arithmetic(tier)
                out[name, tier] = _render(ctx, capfd)
                assert out[name, tier]["kernels"]["locate"] == "general<0,0,0,1>"
                _outside(out[name, tier], "hbm")
    for tier in ("exact", "tolerant"):
        one, eight = out["one", tier], out["eight", tier]
        assert np.array_equal(one["sample_num"], eight["sample_num"]) and np.array_equal(one["sample_flags"], eight["sample_flags"])
        assert one["stats"].n_gathers == eight["stats"].n_gathers
        if interp == "false":
            assert gu.same_bits(one["image"], eight["image"]).all()
    _check_exact(out["eight", "exact"], _oracle(params, grids["eight"], (n_r, "eight")))
    _check_tolerant(out["eight", "tolerant"], out["eight", "exact"])


# ---- meshes with refinement --------------------------------------------------------------------------------------------------------
# (the camera inside the grid's outer edge, r_max = 52.2: from outside it the renders skip the empty shell's steps, and the fused kernel
# has no instantiation over a mesh for that)
MESH_CAMERA = dict(camera_r=50.0)

def _mesh_bytes(block, split, block_interp=False):
    """BlGridDevice::refined_lds_bytes and ::fused_lds_bytes of _mesh(block, split) as BuildLatticeTables (bl_grid.cpp) computes them: the
    two-level mesh has 36 blocks on a 4 x 4 x 4 lattice of fine boxes and six distinct coordinate rows per axis, each times the split.
    (0: beyond BL_LOCATE_REFINED_LDS / not a mesh for the fused kernel)"""
    nb = [b // s for b, s in zip(block, split)]
    pieces = split[0] * split[1] * split[2]
    n_b, n_boxes = 36 * pieces, 64 * pieces
    doubles = sum(4 * s + 1 + 6 * s * (2 * n + 4) + n_b for s, n in zip(split, nb))
    ints = n_boxes + 3 * n_b
    if block_interp:
        slots = 16
        while slots < 2 * n_b:
            slots *= 2
        doubles += slots
        ints += 4 * n_b + slots
    refined = doubles * 8 + (ints + 3) // 4 * 4 * 4
    fused = 384 + sum(6 * s * (16 + 64 * n) for s, n in zip(split, nb)) + 16 * n_boxes
    return (refined if refined <= 136 * KIB else 0), (fused if min(nb) >= 2 and fused <= 150 * KIB else 0)


# id: (cells per block of the two-level mesh, split of every block, refined_lds_bytes, fused_lds_bytes)
#                                                                      blocks   refined_lds_bytes          fused_lds_bytes
MESHES = {
    "36k_64k": ((8, 6, 8), (2, 2, 2), 15896, 17600),           #     288   (0, 36 KiB]                (0, 64 KiB]
    "48k_64k": ((20, 6, 8), (10, 1, 2), 37240, 35168),         #     720   (36, 48 KiB]               (0, 64 KiB]
    "136k_76k": ((10, 6, 8), (5, 3, 4), 98136, 72192),         #   2 160   (48, 136 KiB]              (64, 76 KiB]
    "136k_150k": ((16, 6, 8), (8, 2, 4), 105368, 78784),       #   2 304   (48, 136 KiB]              (76, 150 KiB]
    "hbm_150k": ((16, 6, 8), (8, 3, 4), 0, 111648),            #   3 456   beyond 136 KiB (155 256)   (76, 150 KiB]
    "hbm_none": ((24, 6, 8), (12, 3, 4), 0, 0),                #   5 184   beyond 136 KiB (231 416)   not applicable (164 256)
}


def _locate_shape(refined):
    """bl_launch_locate over a mesh: (where, bytes, lanes, whether the dynamic LDS attribute has to be raised)"""
    if refined == 0:
        return "hbm", 0, 256
    return "lds", refined, (256 if refined <= 36 * KIB else 1024)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_refined_mesh_budgets(name, capfd, monkeypatch, built_library):
    """Tolerant tier with the fused kernel, tolerant tier through the locate kernel and bl_shade_fast_kernel, exact tier, polarized:
    each in the regime the mesh was chosen for, each against the oracle / the exact tier."""
    block, split, refined, fused = MESHES[name]
    assert _mesh_bytes(block, split) == (refined, fused)
    grid = _mesh(block, split)
    params = _params(**MESH_CAMERA)
    want = _oracle(params, grid, name)
    where, staged, lanes = _locate_shape(refined)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
        ctx.debug_set_switches("NO_FUSED_LOCATE")
        outside = _render(ctx, capfd)
    # the fused kernel: 256 lanes two to a unit up to 76 KiB, 512 lanes and an eighth of the workgroups beyond, none without fused_lds_bytes
    if fused:
        assert tol["kernels"]["shade"] == "fused2<1,1,0,1>"   # (a mesh: composed maps only)
        _inside(tol, fused, 256 if fused <= 76 * KIB else 512)
        f = tol["tables"]["fused"]
        assert f["blocks"] == (f["grid"] if fused <= 76 * KIB else f["grid"] // 8) and f["grid"] >= 8
        assert tol["tables"]["redo"]["where"] == "hbm"
    else:
        assert tol["kernels"]["shade"] == "fast<1,0>" and tol["kernels"]["locate"] == "general<1,0,0,0>"
        _outside(tol, where, staged, lanes)
    # the exact tier's kernel with the locate step inside: up to 76 KiB, without the tolerant kernel's 384 bytes of thresholds
    if fused and fused <= 76 * KIB:
        assert exact["kernels"]["shade"] == "exact2<1>"
        _inside(exact, fused - 384)
    else:
        assert exact["kernels"]["shade"] == "exact<1>" and exact["kernels"]["locate"] == "general<1,0,0,0>"
        _outside(exact, where, staged, lanes)
    # the locate kernel: 256 lanes up to 36 KiB, 1 024 lanes and a sixteenth of the workgroups up to 136 KiB, HBM beyond
    assert outside["kernels"]["shade"] == "fast<1,0>" and outside["kernels"]["locate"] == "general<1,0,0,0>"
    _outside(outside, where, staged, lanes)
    loc = outside["tables"]["locate"]
    assert loc["grid"] >= 1024 and loc["blocks"] == (loc["grid"] // 16 if lanes == 1024 else loc["grid"])
    _check_exact(exact, want)
    for got in (tol, outside):
        _check_tolerant(got, exact)
        assert got["stats"].n_gathers == exact["stats"].n_gathers


@pytest.mark.parametrize("name", sorted(MESHES))
def test_refined_mesh_budgets_polarized(name, capfd, monkeypatch, built_library):
    block, split, refined, fused = MESHES[name]
    grid = _mesh(block, split)
    params = _params(polarized=True, **MESH_CAMERA)
    want = _oracle(params, grid, name)
    where, staged, lanes = _locate_shape(refined)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
    for got in (exact, tol):
        if fused and fused <= 76 * KIB:   # (bl_polarized2_refined_applicable; the attribute is raised beyond 64 KiB)
            assert _family(got) == "polarized2"
            _inside(got, fused - 384)
        else:
            assert _family(got) == "shade" and got["kernels"]["locate"] == "general<1,0,0,0>"
            _outside(got, where, staged, lanes)
    _check_exact(exact, want)
    _check_tolerant(tol, exact, polarized=True)


# (cells per block, split, refined_lds_bytes with the MeshBlock table and its hash, the second pass's tables)
BLOCK_INTERP = {
    "1024_lanes": ((8, 6, 8), (4, 2, 2), 62552, "located"),     # 576 blocks of 2 x 3 x 4 cells: locate kernel + bl_shade_fast_kernel<., 2>
    "fused_redo_lds": ((24, 12, 12), (2, 1, 1), 12856, "lds"),   # 72 blocks of 12^3 cells: the fused kernel, second pass on tables in LDS
}


@pytest.mark.parametrize("name", sorted(BLOCK_INTERP))
def test_refined_mesh_budgets_block_interpolation(name, capfd, monkeypatch, built_library):
    """simulation_block_interp = true: the MeshBlock table and its hash count towards the locate kernel's bytes (1 024 lanes at 576
    blocks, where the tables alone would take 256), and the exact second pass behind the fused kernel stages the mesh's tables
    (BL_REDO_TABLES_LDS). Against the same library with the tables searched in HBM (the oracle refuses the reads that the `edge`
    policy defines)."""
    block, split, refined, redo = BLOCK_INTERP[name]
    assert _mesh_bytes(block, split, True)[0] == refined
    assert _mesh_bytes(block, split, False)[0] <= 36 * KIB < refined or redo == "lds"
    grid = _mesh(block, split)
    params = _params(simulation_block_interp="true", **MESH_CAMERA)
    with _context(monkeypatch, params, grid, undefined_policy="edge") as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
        ctx.debug_set_switches("GENERAL_LOCATE", "NO_FUSED_LOCATE")
        tol_hbm = _render(ctx, capfd)
        ctx.set_arithmetic("exact")
        exact_hbm = _render(ctx, capfd)
    where, staged, lanes = _locate_shape(refined)
    _outside(exact, where, staged, lanes)
    if redo == "lds":
        assert tol["kernels"]["shade"] == "fused2<1,1,0,1>"
        _inside(tol, _mesh_bytes(block, split)[1])
        assert (tol["tables"]["redo"]["where"], tol["tables"]["redo"]["bytes"]) == ("lds", refined)
    else:
        assert tol["kernels"]["shade"] == "fast<0,2>"
        _outside(tol, where, staged, lanes)
        assert tol["tables"]["locate"]["blocks"] == tol["tables"]["locate"]["grid"] // 16
    for got in (tol_hbm, exact_hbm):
        _outside(got, "hbm")
    assert gu.same_bits(exact["image"], exact_hbm["image"]).all() and np.array_equal(exact["sample_num"], exact_hbm["sample_num"])
    assert exact["stats"].n_gathers == exact_hbm["stats"].n_gathers
    assert np.isfinite(exact["image"]).all() and (exact["image"][0] > 0.0).sum() > exact["image"].shape[1] // 2
    for got in (tol, tol_hbm):
        _check_tolerant(got, exact)
        assert got["stats"].n_gathers == exact["stats"].n_gathers


def test_large_workgroup_counts_on_a_frame_of_several_chunks(capfd, monkeypatch, built_library):
    """192^2 rays over the mesh of 1 024-lane locate workgroups and 512-lane fused ones: alone the locate kernel launches a sixteenth
    of its 256-lane count, beside the next chunk's geodesic kernel (overlapping chunks) a quarter of the smaller count, the fused kernel
    an eighth. Against the exact tier and against the same library with every table in HBM."""
    block, split, refined, fused = MESHES["136k_150k"]
    grid = _mesh(block, split)
    params = _params(camera_resolution=192, **MESH_CAMERA)
    with _context(monkeypatch, params, grid) as ctx:
        ctx.set_arithmetic("exact")
        exact = _render(ctx, capfd)
        ctx.set_arithmetic("tolerant")
        tol = _render(ctx, capfd)
        ctx.set_scratch_limit(1 << 28)   # (a few thousand rays' records per scratch set: several chunks)
        ctx.set_overlap(True)
        ctx.debug_set_switches("NO_FUSED_LOCATE")
        chunks = _render(ctx, capfd)
        ctx.debug_set_switches("GENERAL_LOCATE", "NO_FUSED_LOCATE")
        hbm = _render(ctx, capfd)
    _outside(exact, "lds", refined, 1024)
    loc = exact["tables"]["locate"]
    assert loc["grid"] >= 1024 and loc["blocks"] == loc["grid"] // 16
    _inside(tol, fused, 512)
    assert tol["tables"]["fused"]["grid"] >= 8 and tol["tables"]["fused"]["blocks"] == tol["tables"]["fused"]["grid"] // 8
    assert chunks["stats"].n_chunks >= 2
    _outside(chunks, "lds", refined, 1024)
    loc = chunks["tables"]["locate"]   # (the first chunk beside the second one's geodesic kernel, the last chunk alone)
    assert 4 <= loc["grid"] < 1024 and loc["blocks"] == loc["grid"] // 4
    assert loc["last_grid"] >= 1024 and loc["last_blocks"] == loc["last_grid"] // 16
    _outside(hbm, "hbm")
    assert np.isfinite(exact["image"]).all() and (exact["image"][0] > 0.0).sum() > exact["image"].shape[1] // 2
    for got in (tol, chunks, hbm):
        _check_tolerant(got, exact)
        assert got["stats"].n_gathers == exact["stats"].n_gathers
