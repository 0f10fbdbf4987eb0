"""GPU: geodesics once per series for root-level frames of more than one chunk (bl_set_geodesic_reuse, the kept layout).

A frame whose rays do not fit one chunk used to integrate every ray for every snapshot. Now the render after the first one of a camera
integrates into the kept layout - a record store for the whole frame beside shading arrays for one chunk - and the renders after that
shade the kept chunks one after another without the stepper. Each case forces several chunks with bl_set_scratch_limit: the cap lets the
frame's records fit, but not the records together with shading arrays for all of them. What must hold: reuse from the third frame on,
several chunks on every frame, the images of fresh renders (bit for bit in the exact tier and under bl_set_reproducible at one
frequency; to 1e-13 relative for the tolerant tier's several frequencies and composed maps), and every change of camera, cap or
setting integrates again."""
import dataclasses

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

RECORD_BYTES = 64   # a sample record: position + id | momentum + length


def _snapshots(grid, count):
    """`count` snapshots on one geometry: density and pressure scaled, the rest kept"""
    out = []
    for n in range(count):
        prim = grid.prim.copy()
        prim[0:2] *= np.float32(1.0 + 0.11 * n)
        out.append(dataclasses.replace(grid, prim=prim))
    return out


def _context(params, tier, reproducible=False, reuse=True, cap=None, overlap=False):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_arithmetic(tier)
    ctx.set_reproducible(reproducible)
    ctx.set_geodesic_reuse(reuse)
    if cap is not None:
        ctx.set_scratch_limit(int(cap))
    if overlap:
        ctx.set_overlap(True)
    return ctx


def _shading_bytes(stats, n_nu, polarized):
    """What the one-chunk arrays beside the records cost per record on the path the stats name (bl_render.hip: PlanScratch)"""
    if polarized:
        return 128 + 64 + 64 * n_nu + (96 if stats.arithmetic == 1 else 0) + 1
    located = 40 if stats.fused_variant == 0 else 0
    if stats.arithmetic == 1:   # tolerant: per-sample factors from four frequencies on, else transfer records (+ composed maps)
        return located + (64 if n_nu >= 4 else 16 * n_nu + 16 * stats.composed_maps)
    return located + 16 * n_nu + (64 if n_nu >= 4 else 0)


def _cap(one_chunk, n_nu=1, polarized=False, max_steps=2000):
    """A scratch cap from a one-chunk render of the frame: the store as the library sizes it (the records, the
    reservations of a stepper grid held to a sixteenth of them, a block per wave and chunk, the unused end of each segment) and shading arrays for about half the
    records beside it - two to four chunks. The whole frame's records and shading arrays at once would need more."""
    st = one_chunk["stats"]
    records = st.n_samples_emitted
    grid = max(1, min((st.n_rays + 127) // 128, records // 16 // (64 * max_steps)))
    # (1.02: the partly filled blocks of the first render's chunks; the in-flight reservations once for the last chunk and once per
    # segment - the record arrays and the tails of the shading arrays - whose end a chunk cannot use)
    if polarized:
        tails = 4 if st.arithmetic == 1 else 3
    else:
        tails = (2 if st.fused_variant == 0 else 0) + 1 + (st.composed_maps if st.arithmetic == 1 and n_nu < 4 else 0) \
            + (1 if st.arithmetic == 0 and n_nu >= 4 else 0)
    segments = 1 + tails
    store = 1.02 * records + (1 + segments) * grid * 64 * max_steps + 24 * grid * 1024
    return int(RECORD_BYTES * store + 0.45 * records * _shading_bytes(st, n_nu, polarized))


def _same_frame(got, want, bitwise=True, tolerance=1.0e-13):
    assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
    if bitwise:
        assert gu.same_bits(got["image"], want["image"]).all()
    else:
        assert np.array_equal(np.isnan(got["image"]), np.isnan(want["image"]))
        with np.errstate(invalid="ignore"):
            assert np.nanmax(np.abs(got["image"] - want["image"])) <= tolerance * np.nanmax(np.abs(want["image"]))
    assert got["stats"].n_samples == want["stats"].n_samples and got["stats"].n_gathers == want["stats"].n_gathers


def _series(params, snaps, tier, cap, reproducible=False, **render_args):
    with _context(params, tier, reproducible, cap=cap) as ctx:
        frames = []
        for grid in snaps:
            ctx.set_grid(grid)
            frames.append(ctx.render(**render_args))
    return frames


def _fresh(params, grid, tier, cap, reproducible=False, **render_args):
    with _context(params, tier, reproducible, reuse=False, cap=cap) as ctx:
        ctx.set_grid(grid)
        out = ctx.render(**render_args)
    assert out["stats"].geodesics_reused == 0 and out["stats"].launches_geodesic == out["stats"].n_chunks
    return out


def _one_chunk(params, grid, tier, reproducible=False):
    with _context(params, tier, reproducible, reuse=False) as ctx:
        ctx.set_grid(grid)
        out = ctx.render()
    assert out["stats"].n_chunks == 1
    return out


def _reuse_flags(frames):
    flags = [f["stats"].geodesics_reused for f in frames]
    assert flags in ([0, 0] + [1] * (len(frames) - 2), [0] + [1] * (len(frames) - 1)), flags
    for f in frames:
        st = f["stats"]
        assert st.n_chunks > 1, [g["stats"].n_chunks for g in frames]
        if st.geodesics_reused:
            assert st.launches_geodesic == 0 and st.ms_geodesic == 0.0 and st.sampling_reused == 0
            assert st.n_chunks == frames[1]["stats"].n_chunks
        else:
            assert st.launches_geodesic == st.n_chunks and st.ms_geodesic > 0.0


def _bench_params(resolution, **extra):
    import bench
    return dict(bench.WORKLOAD, camera_resolution=resolution, **extra)


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_unpolarized_series_reuses_from_the_third_frame(tier):
    """The benchmark's path at 128^2, in three or so chunks: frames 3 and 4 shade the kept chunks"""
    from blacklight_amd import mock
    params = _bench_params(128)
    snaps = _snapshots(mock.generate(n_r=48, n_th=48, n_ph=48), 4)
    cap = _cap(_one_chunk(params, snaps[0], tier, reproducible=True))
    frames = _series(params, snaps, tier, cap, reproducible=True, want_camera=True)
    _reuse_flags(frames)
    for frame, grid in zip(frames, snaps):
        want = _fresh(params, grid, tier, cap, reproducible=True, want_camera=True)
        _same_frame(frame, want)
        assert gu.same_bits(frame["camera_pos"], want["camera_pos"]).all() and gu.same_bits(frame["camera_dir"], want["camera_dir"]).all()
    assert not gu.same_bits(frames[2]["image"], frames[3]["image"]).all()   # (the snapshots do differ)
    if tier == "tolerant":
        # composed maps (the tolerant tier's default): the same frames to rounding
        composed = _one_chunk(params, snaps[0], tier)
        cap = _cap(composed)
        frames = _series(params, snaps, tier, cap)
        _reuse_flags(frames)
        assert all(f["stats"].composed_maps == 1 for f in frames)
        for frame, grid in zip(frames, snaps):
            _same_frame(frame, _fresh(params, grid, tier, cap), bitwise=False)


def test_polarized_series_reuses_from_the_third_frame():
    """Full-Stokes transfer with an optical-depth row (configuration 4's physics) at 96^2, exact tier: bit for bit"""
    from blacklight_amd import mock
    params = _bench_params(96, image_polarization=True, image_tau=True)
    snaps = _snapshots(mock.generate(n_r=48, n_th=48, n_ph=48), 4)
    cap = _cap(_one_chunk(params, snaps[0], "exact"), polarized=True)
    frames = _series(params, snaps, "exact", cap)
    _reuse_flags(frames)
    for frame, grid in zip(frames, snaps):
        _same_frame(frame, _fresh(params, grid, "exact", cap))


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_several_frequencies(tier):
    """Eight frequencies: the exact tier bit for bit, the tolerant tier's many-frequency kernel to 1e-13 (its last bit wobbles from
    run to run)"""
    from blacklight_amd import mock
    params = _bench_params(96, image_num_frequencies=8, image_frequency_start=1.5e11, image_frequency_end=3.3e11, image_frequency_spacing="lin_wave")
    snaps = _snapshots(mock.generate(n_r=48, n_th=48, n_ph=48), 4)
    cap = _cap(_one_chunk(params, snaps[0], tier), n_nu=8)
    frames = _series(params, snaps, tier, cap)
    _reuse_flags(frames)
    for frame, grid in zip(frames, snaps):
        _same_frame(frame, _fresh(params, grid, tier, cap), bitwise=tier == "exact")


def test_adaptive_root_level_of_several_chunks():
    """The adaptive loop with a root level of several chunks: snapshot 3's root level shades the kept chunks, its refined levels
    integrate in buffers of their own, and every level is the fresh run's"""
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case("sim_adaptive")
    snaps = _snapshots(gu.golden_grid(mock_args), 4)
    root = _one_chunk(params, snaps[0], "exact")
    cap = _cap(root)
    series = []
    with _context(params, "exact", cap=cap) as ctx:
        for grid in snaps:
            ctx.set_grid(grid)
            series.append(ctx.render_adaptive())
    assert len(series[0]) > 1   # (the case does refine)
    _reuse_flags([run[0] for run in series])
    for run in series:
        assert all(lv["stats"].geodesics_reused == 0 for lv in run[1:])
    for grid, run in zip(snaps, series):
        with _context(params, "exact", reuse=False, cap=cap) as ctx:
            ctx.set_grid(grid)
            want = ctx.render_adaptive()
        assert len(want) == len(run)
        for a, b in zip(run, want):
            assert np.array_equal(a["block_locs"], b["block_locs"]) if a["block_locs"] is not None else b["block_locs"] is None
            assert gu.same_bits(a["image"], b["image"]).all() and np.array_equal(a["sample_num"], b["sample_num"])


def test_what_invalidates_the_kept_chunks():
    from blacklight_amd import distributed as bd
    from blacklight_amd import mock
    params = _bench_params(128)
    snaps = _snapshots(mock.generate(n_r=48, n_th=48, n_ph=48), 2)
    cap = _cap(_one_chunk(params, snaps[0], "exact"))
    fresh = [_fresh(params, grid, "exact", cap) for grid in snaps]

    def flags(ctx, count, **render_args):
        got = []
        for n in range(count):
            ctx.set_grid(snaps[n % 2])
            got.append(ctx.render(**render_args))
        return [g["stats"].geodesics_reused for g in got], got

    with _context(params, "exact", cap=cap) as ctx:
        assert flags(ctx, 3)[0] == [0, 0, 1]
        # another camera (a share of the pixels): integrated, then kept; the whole frame again: integrated again
        pixels = bd.tile_pixels(128, 1, 2, 64)
        seen, got = flags(ctx, 3, pixel_map=pixels)
        assert seen[0] == 0 and seen[-1] == 1 and gu.same_bits(got[-1]["image"], fresh[0]["image"][:, pixels]).all()
        seen, got = flags(ctx, 3)
        assert seen == [0, 0, 1] and gu.same_bits(got[-1]["image"], fresh[0]["image"]).all()
        # another cap: integrated again
        ctx.set_scratch_limit(cap + (256 << 20))
        assert flags(ctx, 1)[0] == [0]
        ctx.set_scratch_limit(cap)
        # switched off: every render integrates
        ctx.set_geodesic_reuse(False)
        seen, got = flags(ctx, 3)
        assert seen == [0, 0, 0] and all(g["stats"].launches_geodesic == g["stats"].n_chunks > 1 for g in got)
        ctx.set_geodesic_reuse(True)
        seen, got = flags(ctx, 4)
        assert seen == [0, 0, 1, 1] and gu.same_bits(got[3]["image"], fresh[1]["image"]).all()
    # a cap too small for the store beside a shading set: never kept, the fresh render's bits
    small = int(RECORD_BYTES * 0.9 * _one_chunk(params, snaps[0], "exact")["stats"].n_samples_emitted)
    with _context(params, "exact", cap=small) as ctx:
        seen, got = flags(ctx, 4)
        assert seen == [0, 0, 0, 0] and all(g["stats"].n_chunks > 1 for g in got)
        for n, g in enumerate(got):
            _same_frame(g, _fresh(params, snaps[n % 2], "exact", small))
    # two scratch sets: nothing kept
    with _context(params, "exact", cap=cap, overlap=True) as ctx:
        seen, got = flags(ctx, 4)
        assert seen == [0, 0, 0, 0]
        for n, g in enumerate(got):
            _same_frame(g, fresh[n % 2])


def test_kept_chunks_download_chunk_by_chunk():
    """Host outputs of a quarter of a GiB in many rows go chunk by chunk (RenderJob::raster): a reused multi-chunk frame into pageable
    memory and into pinned buffers is the integrating render's frame (128 frequencies, tolerant tier: to 1e-13)"""
    from blacklight_amd import mock
    params = _bench_params(512, image_num_frequencies=128, image_frequency_start=1.5e11, image_frequency_end=3.3e11, image_frequency_spacing="lin_wave")
    snaps = _snapshots(mock.generate(n_r=48, n_th=48, n_ph=48), 2)
    cap = _cap(_one_chunk(params, snaps[0], "tolerant"), n_nu=128)
    want = _fresh(params, snaps[1], "tolerant", cap)
    want_even = _fresh(params, snaps[0], "tolerant", cap)
    with _context(params, "tolerant", cap=cap) as ctx:
        n_q, n_rays = ctx.num_quantities, ctx.level_pixels()
        assert n_q * n_rays * 8 >= (256 << 20)
        pinned = dict(image=ctx.pinned_array((n_q, n_rays)), sample_num=ctx.pinned_array(n_rays, np.int32),
                      sample_flags=ctx.pinned_array(n_rays, np.uint8))
        got = []
        for n in range(4):
            ctx.set_grid(snaps[n % 2])
            got.append(ctx.render(out=pinned if n == 3 else None))
            if n == 3:
                got[-1] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got[-1].items()}
        assert [g["stats"].geodesics_reused for g in got][2:] == [1, 1] and all(g["stats"].n_chunks > 1 for g in got)
        _same_frame(got[2], want_even, bitwise=False)   # (reused, pageable)
        _same_frame(got[3], want, bitwise=False)        # (reused, pinned)
        _same_frame(got[1], want, bitwise=False)
        _same_frame(got[3], got[1], bitwise=False)
