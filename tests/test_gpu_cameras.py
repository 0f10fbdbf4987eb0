"""Several cameras in one render (bl_set_cameras) on the GPU: the slice [:, c res^2 : (c + 1) res^2] of every output against what a
context renders that bl_init made with camera c's angles in its parameter block - never against bl_set_cameras(1, ...). Bit for
bit in the exact tier and under bl_set_reproducible, whatever the chunking; with composed maps (the tolerant default) integer
outputs and NaN masks equal and every finite pixel within 1e-10 relative (the tier's own per-pixel bound,
tests/test_gpu_window_1024.py). Shapes: 16^2 (a multiple of 64 pixels per camera: the camera index is uniform over a wave of the
ray-start kernel; the swizzled tile order) and 12^2 (camera boundaries inside a wave: each lane loads its own frame; the
unswizzled order). Cameras: the pole (0, 0), (60, 30) and (163, 275).
Fresh comparison renders are made once per (case, size, camera, tier) and shared by the tests of this module."""
import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

CAMERAS = [(0.0, 0.0), (60.0, 30.0), (163.0, 275.0)]
OTHER_CAMERAS = [(120.0, 200.0), (17.0, 5.0)]
SCRATCH = 1 << 30
OUTPUTS = ("image", "sample_num", "sample_flags", "camera_pos", "camera_dir", "rendering")
BL_E_UNSUPPORTED, BL_E_ARG = 3, 5
BL_TAIL_WIDE = 1

_fresh_cache = {}
_grids = {}


def _case(name, res, **overrides):
    fx, params, mock_args = gu.load_case(name)
    params = dict(params, **overrides)
    if res is not None:
        params["camera_resolution"] = res
    if mock_args is None:
        return params, None
    key = repr(sorted(mock_args.items()))
    if key not in _grids:
        _grids[key] = gu.golden_grid(mock_args)
    return params, _grids[key]


def _context(params, grid, tier="exact", reproducible=False, scratch=SCRATCH):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_arithmetic(tier)
    ctx.set_reproducible(reproducible)
    ctx.set_scratch_limit(scratch)
    if grid is not None:
        ctx.set_grid(grid)
    return ctx


def _fresh(name, res, camera, tier="exact", reproducible=False, **overrides):
    """The render of a context made by bl_init with that camera's angles in its block."""
    key = (name, res, camera, tier, reproducible, repr(sorted(overrides.items())))
    if key not in _fresh_cache:
        params, grid = _case(name, res, camera_th=camera[0], camera_ph=camera[1], **overrides)
        with _context(params, grid, tier, reproducible) as ctx:
            out = ctx.render(want_camera=True)
            out["warnings"] = ctx.warnings
        for value in out.values():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
        _fresh_cache[key] = out
    return _fresh_cache[key]


def _slice(out, name, where):
    return out[name][..., where] if name in ("image", "rendering") else out[name][where]


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    if got.dtype == np.float64:
        same = gu.same_bits(got, want)
        assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ"
    else:
        assert np.array_equal(got, want), what


def _assert_cameras_equal_fresh(got, ctx, name, res, cameras, tier="exact", reproducible=False, bits=True, **overrides):
    n_flagged = 0
    for c, camera in enumerate(cameras):
        want = _fresh(name, res, camera, tier, reproducible, **overrides)
        where = ctx.camera_slice(c)
        n_flagged += int(want["sample_flags"].sum())
        for output in OUTPUTS:
            if want[output] is None:
                assert got[output] is None
                continue
            mine = _slice(got, output, where)
            if bits or output != "image":   # integer outputs, camera rows (a function of the pixel) and - exact arithmetic - renderings: always equal
                _assert_bits(mine, want[output], (name, res, c, output))
            else:
                assert np.array_equal(np.isnan(mine), np.isnan(want[output])), (name, res, c, "NaN mask")
                rel, above, used, same_support = gu.per_pixel_relative(mine, want[output])
                print(f"{name} {res}^2 camera {c}: per-pixel relative {rel:.3e} over {used} pixels")
                assert rel <= 1.0e-10 and same_support, (name, res, c, rel)
    return n_flagged


# ---------------------------------------------------------------------------------------------------------------- exact tier: bits
EXACT_CASES = [(case, res) for case in ("sim_dp_interp", "sim_spin_fallback", "sim_rk4", "sim_pinhole_camera_norm", "sim_polarized") for res in (16, 12)] \
    + [("formula_64", 16), ("formula_64", 12)]


@pytest.mark.parametrize("case,res", EXACT_CASES)
def test_exact_tier_every_output_bit_equal_per_camera(case, res, built_library):
    """All three ray-start instantiations (Dormand-Prince without and with spin, fixed step), both camera types, the polarized
    transfer's camera projection, formula mode."""
    params, grid = _case(case, res)
    with _context(params, grid) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        assert ctx.level_pixels(0) == 3 * res * res
        got = ctx.render(want_camera=True)
        warnings = ctx.warnings
        st = got["stats"]
        assert got["image"].shape == (ctx.num_quantities, 3 * res * res)
        assert (st.n_cameras, st.n_rays, st.xcd_order) == (3, 3 * res * res, 0)
        assert st.launches_geodesic == st.n_chunks == 1
        n_flagged = _assert_cameras_equal_fresh(got, ctx, case, res, CAMERAS)
    # the reference's warning once per render, with the totals over all cameras
    assert warnings.count("geodesics terminate unexpectedly") == (1 if n_flagged else 0)
    if n_flagged:
        assert f"Warning: {n_flagged} out of {3 * res * res} geodesics terminate unexpectedly." in warnings


@pytest.mark.parametrize("res", [16, 12])
def test_each_camera_bit_equal_to_the_cpu_oracle(res, built_library):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    params, grid = _case("sim_dp_interp", res)
    with _context(params, grid) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        got = ctx.render(want_camera=True)
        frames = [ctx.camera_frame_of(c) for c in range(3)]
        slices = [ctx.camera_slice(c) for c in range(3)]
    for c, (th, ph) in enumerate(CAMERAS):
        p = bl.Params.from_dict(dict(params, camera_th=th, camera_ph=ph))
        want = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=res * res, max_steps=int(p.get("ray_max_steps")),
                                 want_camera=True)
        for key in gu.FRAME_KEYS:
            assert gu.same_bits(np.array(getattr(frames[c], key)), np.array(getattr(want["frame"], key))).all(), (c, key)
        assert np.array_equal(got["sample_num"][slices[c]], want["sample_num"])
        assert np.array_equal(got["sample_flags"][slices[c]], want["sample_flags"])
        for output in ("image", "camera_pos", "camera_dir"):
            _assert_bits(_slice(got, output, slices[c]), want[output], (res, c, output))


# ---------------------------------------------------------------------------------------------------------------- tolerant tier
@pytest.mark.parametrize("res", [16, 12])
def test_tolerant_default_within_the_tiers_bound_and_bits_when_reproducible(res, built_library):
    params, grid = _case("sim_dp_interp", res)
    for reproducible in (False, True):
        with _context(params, grid, "tolerant", reproducible) as ctx:
            ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
            got = ctx.render(want_camera=True)
            st = got["stats"]
            assert st.arithmetic == 1 and st.n_cameras == 3 and st.launches_geodesic == st.n_chunks
            if reproducible:
                assert st.composed_maps == 0
            _assert_cameras_equal_fresh(got, ctx, "sim_dp_interp", res, CAMERAS, "tolerant", reproducible, bits=reproducible)


# ---------------------------------------------------------------------------------------------------------------- chunking, pixel maps, variants
@pytest.mark.parametrize("case,res", [("sim_dp_interp", 16), ("sim_dp_interp", 12), ("sim_polarized", 12)])
def test_several_chunks_same_bits(case, res, built_library):
    params, grid = _case(case, res)
    # (a budget of a few rays' worst case: 600 bytes per possible sample of one ray; a polarized run's scratch set holds a list of
    # 2^24 record indices - 128 MiB - whatever the frame, and 12 MiB beside it are some tens of thousands of its larger records)
    scratch = (1 << 27) + (12 << 20) if case == "sim_polarized" else max(1 << 20, int(params["ray_max_steps"]) * 600)
    with _context(params, grid, scratch=scratch) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        got = ctx.render(want_camera=True)
        st = got["stats"]
        print(f"{case} {res}^2: {st.n_chunks} chunks")
        assert st.n_chunks >= 2 and st.launches_geodesic == st.n_chunks and st.n_cameras == 3
        _assert_cameras_equal_fresh(got, ctx, case, res, CAMERAS)


@pytest.mark.parametrize("case,res", [("sim_dp_interp", 16), ("sim_polarized", 12)])
def test_pixel_map_of_virtual_pixels(case, res, built_library):
    """About a hundred virtual pixels drawn across all cameras: equal to the same pixels of the full render (which the test above
    and test_exact_tier_... hold against fresh contexts). Entries outside 0 .. C res^2 - 1 are refused."""
    import blacklight_amd as bl
    params, grid = _case(case, res)
    rng = np.random.default_rng(20261019)
    with _context(params, grid) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        full = ctx.render(want_camera=True)
        picks = rng.choice(3 * res * res, size=100, replace=False).astype(np.int32)
        assert len({int(v) // (res * res) for v in picks}) == 3
        part = ctx.render(pixel_map=picks, want_camera=True)
        assert part["stats"].n_rays == 100
        for output in OUTPUTS:
            if full[output] is not None:
                _assert_bits(_slice(part, output, slice(None)), _slice(full, output, picks), (case, output))
        for bad in (3 * res * res, -1):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.render(pixel_map=np.array([0, bad, 5], dtype=np.int32))
            assert err.value.code == BL_E_ARG and f"outside 0 .. {3 * res * res - 1}" in str(err.value)
        from blacklight_amd import _capi   # n_rays against the level's C res^2 pixels: one ray more is refused, host buffers that would hold it
        import ctypes as C
        d = _capi.RenderDesc()
        image = np.empty((ctx.num_quantities, 3 * res * res + 1))
        d.n_rays, d.image = 3 * res * res + 1, image.ctypes.data_as(C.c_void_p)
        assert ctx._lib.bl_render(ctx._ctx, C.byref(d)) == BL_E_ARG
        assert "n_rays exceeds the pixels of this level." in ctx._lib.bl_last_error(ctx._ctx).decode()
        whole = np.empty((ctx.num_quantities, 3 * res * res))   # (and exactly C res^2 is the full frame)
        d.n_rays, d.image = 3 * res * res, whole.ctypes.data_as(C.c_void_p)
        assert ctx._lib.bl_render(ctx._ctx, C.byref(d)) == 0
        _assert_bits(whole, full["image"], "full frame through the C interface")


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_two_electron_models_times_two_cameras(tier, built_library):
    """Rows stay variant-major: image row m n_q + q at [c res^2, (c + 1) res^2) is model m seen by camera c. The tolerant tier renders
    the models in one pass (one shading launch per chunk): held as the tolerant default is; the exact tier: bits."""
    res, cameras, pairs = 16, CAMERAS[1:], [(10.0, 1.0), (160.0, 2.0)]
    params, grid = _case("sim_dp_interp", res)
    with _context(params, grid, tier) as ctx:
        ctx.set_cameras([th for th, _ in cameras], [ph for _, ph in cameras])
        ctx.set_electron_models([h for h, _ in pairs], rat_low=[lo for _, lo in pairs])
        got = ctx.render(want_camera=True)
        st = got["stats"]
        assert got["image"].shape == (ctx.num_quantities, 2 * res * res) and st.n_cameras == 2
        if tier == "tolerant":
            assert st.launches_shade == st.n_chunks   # one pass
        n_q = ctx.num_quantities // 2
        for m, (high, low) in enumerate(pairs):
            rows = dict(got, image=got["image"][m * n_q:(m + 1) * n_q])
            _assert_cameras_equal_fresh(rows, ctx, "sim_dp_interp", res, cameras, tier, bits=tier == "exact", plasma_rat_high=high, plasma_rat_low=low)


# ---------------------------------------------------------------------------------------------------------------- series
def test_series_reuses_the_geodesics_of_all_cameras(built_library):
    res = 16
    params, grid = _case("sim_dp_interp", res)
    with _context(params, grid) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        first = ctx.render(want_camera=True)
        assert first["stats"].geodesics_reused == 0
        ctx.set_grid(grid)
        again = ctx.render(want_camera=True)
        assert again["stats"].geodesics_reused == 1 and again["stats"].launches_geodesic == 0 and again["stats"].n_cameras == 3
        for output in OUTPUTS:
            if first[output] is not None:
                _assert_bits(again[output], first[output], output)
        _assert_cameras_equal_fresh(again, ctx, "sim_dp_interp", res, CAMERAS)
        # another list: the resident records go, the new list's images come
        others = [CAMERAS[0]] + OTHER_CAMERAS
        ctx.set_cameras([th for th, _ in others], [ph for _, ph in others])
        ctx.set_grid(grid)
        changed = ctx.render(want_camera=True)
        assert changed["stats"].geodesics_reused == 0 and changed["stats"].launches_geodesic == changed["stats"].n_chunks
        _assert_cameras_equal_fresh(changed, ctx, "sim_dp_interp", res, others)
        ctx.set_cameras([th for th, _ in others[:2]], [ph for _, ph in others[:2]])   # a shorter list is another list too
        fewer = ctx.render(want_camera=True)
        assert fewer["stats"].geodesics_reused == 0 and fewer["stats"].n_rays == 2 * res * res
        _assert_cameras_equal_fresh(fewer, ctx, "sim_dp_interp", res, others[:2])


# ---------------------------------------------------------------------------------------------------------------- one camera, none, policies
@pytest.mark.parametrize("res", [16, 12])
def test_one_camera_is_the_fresh_context_and_none_is_the_blocks_own(res, built_library):
    params, grid = _case("sim_dp_interp", res)
    own = (float(params["camera_th"]), float(params["camera_ph"]))
    with _context(params, grid) as ctx:
        ctx.set_cameras(*CAMERAS[2])
        one = ctx.render(want_camera=True)
        assert one["stats"].n_cameras == 1 and one["stats"].n_rays == res * res
        _assert_cameras_equal_fresh(one, ctx, "sim_dp_interp", res, [CAMERAS[2]])
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        ctx.render()
        ctx.set_cameras([])
        none = ctx.render(want_camera=True)
        assert none["stats"].n_cameras == 1 and none["stats"].geodesics_reused == 0
        _assert_cameras_equal_fresh(none, ctx, "sim_dp_interp", res, [own])


def test_split_tail_policy_resolves_to_wide(built_library):
    """BL_TAIL_SPLIT asked for by name: with two cameras or more the render runs BL_TAIL_WIDE and says so; the bits are the same."""
    res = 16
    params, grid = _case("sim_dp_interp", res)
    with _context(params, grid) as ctx:
        ctx.set_tail_policy("split")
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        got = ctx.render(want_camera=True)
        assert got["stats"].tail_policy == BL_TAIL_WIDE and got["stats"].xcd_order == 0
        _assert_cameras_equal_fresh(got, ctx, "sim_dp_interp", res, CAMERAS)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_context(built_library, tmp_path):
    import blacklight_amd as bl
    res = 16
    two = ([17.0, 60.0], [0.0, 90.0])

    def refused(name, fragment, n=2, own_size=False, **overrides):
        if name.startswith("slow_"):
            import json
            import os
            params = json.loads(str(np.load(os.path.join(gu.GOLDEN_DIR, f"{name}.npz"), allow_pickle=False)["params"]))
        else:
            params, grid = _case(name, None if own_size else res, **overrides)
        with _context(params, None) as ctx:
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_cameras(two[0][:n], two[1][:n])
            assert err.value.code == BL_E_UNSUPPORTED and fragment in str(err.value), str(err.value)
            assert ctx.num_cameras == 0 and ctx.level_pixels(0) == ctx.resolution ** 2   # a refused call changes nothing

    refused("sim_adaptive", "adaptive refinement reads one image", own_size=True)
    refused("slow_interp", "slow light renders one camera")
    refused("sim_dp_interp", "a geodesic checkpoint holds one camera", checkpoint_geodesic_save="true", checkpoint_geodesic_file=str(tmp_path / "geo.bin"))
    refused("sim_dp_interp", "a geodesic checkpoint carries its own camera", n=1, checkpoint_geodesic_load="true",
            checkpoint_geodesic_file=str(tmp_path / "geo.bin"))
    refused("sim_dp_interp", "a sample checkpoint holds one camera", checkpoint_sample_save="true", checkpoint_sample_file=str(tmp_path / "samples.bin"))
    refused("sim_dp_interp", "cut_omit_near and cut_omit_far compare with one camera position", cut_omit_near="true")
    refused("sim_dp_interp", "image_crossings counts crossings of one camera's plane", image_crossings="true")
    params, grid = _case("sim_dp_interp", res, adaptive_block_size=8, output_file=str(tmp_path / "out.npz"))
    with _context(params, grid) as ctx:
        ctx.set_cameras(*two)
        got = ctx.render()
        for kwargs in ({}, {"variant": 0}):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([dict(got, block_locs=None)], **kwargs)
            assert err.value.code == BL_E_UNSUPPORTED and "the reference's file holds one camera" in str(err.value)
        with pytest.raises(bl.BlacklightError) as err:
            ctx.adaptive_refine(0, got["image"])
        assert err.value.code == BL_E_UNSUPPORTED and "two or more cameras" in str(err.value)
        ctx.write_output([dict(got, block_locs=None)], camera=1)   # the call that does write it
        assert (tmp_path / "out.c01.npz").exists()
