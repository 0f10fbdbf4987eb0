"""An explicit list of observing frequencies (bl_set_frequencies) on the GPU: row l of a list render against what a FRESH context renders
that bl_init made with image_num_frequencies = 1 and image_frequency = L[l] in its block - never against a list of one. Bit for bit
in the exact tier; in the tolerant tier identical NaN masks and every finite pixel within 1e-10 relative of the exact tier's row (the
tier's own per-pixel bound, golden_util.per_pixel_relative), polarized rows within the bound tests/test_gpu_polarized_variants.py uses.
The list L = [345, 86, 230, 230, 1000] GHz is unordered, holds a duplicate and is taken at lengths 1 to 5: both sides of the plan's
n_nu >= 4 switch to per-sample factors (freq_split, coef_split). All frequencies lie between 4e10 and 2e12 Hz, where no accumulator
reaches the bottom of the normal range. Fresh one-frequency renders are made once per (case, frequency, tier) and shared."""
import json
import os

import numpy as np
import pytest

import frequency_util as fu
import golden_util as gu

pytestmark = pytest.mark.gpu

L = fu.L
OTHER = [1.5e11, 6.9e11, 4.3e10]
SCRATCH = 1 << 30

_fresh_cache = {}
_list_cache = {}
_grids = {}


def _case(name, **overrides):
    if name in gu.SLOW_CASES:
        fx = np.load(os.path.join(gu.GOLDEN_DIR, f"{name}.npz"), allow_pickle=False)
        return dict(json.loads(str(fx["params"])), **overrides), ("slow", name)
    fx, params, mock_args = gu.load_case(name)
    if name == "sim_dp_interp":
        params["camera_resolution"] = 16
    params = dict(params, **overrides)
    if mock_args is None:
        return params, None
    key = repr(sorted(mock_args.items()))
    if key not in _grids:
        _grids[key] = gu.golden_grid(mock_args)
    return params, _grids[key]


def _slow_slices(name):
    if ("slow", name) not in _grids:
        fx = np.load(os.path.join(gu.GOLDEN_DIR, f"{name}.npz"), allow_pickle=False)
        params = json.loads(str(fx["params"]))
        grids = gu.slow_light_grids(fx)
        file_times = [float(t) for t in fx["file_times"]]
        t_cam, files = gu.slow_light_windows(params, file_times)[0]
        _grids["slow", name] = [(grids[f], file_times[f]) for f in files]
    return _grids["slow", name]


def _context(params, grid, tier):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    ctx.set_arithmetic(tier)
    ctx.set_scratch_limit(SCRATCH)
    if isinstance(grid, tuple):   # slow light: the window of the first image
        for n, (slice_grid, time) in enumerate(_slow_slices(grid[1])):
            ctx.set_grid_slice(n, slice_grid, time)
        ctx.set_snapshot(0)
    elif grid is not None:
        ctx.set_grid(grid)
    return ctx


def _frozen(out):
    for value in out.values():
        if isinstance(value, np.ndarray):
            value.setflags(write=False)
    return out


def _fresh(name, hz, tier, **overrides):
    """The render of a context made by bl_init with that one frequency in its block."""
    key = (name, float(hz), tier, repr(sorted(overrides.items())))
    if key not in _fresh_cache:
        params, grid = _case(name, **overrides)
        with _context(fu.one_frequency(params, hz), grid, tier) as ctx:
            assert ctx.num_frequencies == 0 and ctx.frequencies.tolist() == [float(hz)]
            _fresh_cache[key] = _frozen(ctx.render())
    return _fresh_cache[key]


def _list_render(name, n, tier):
    key = (name, n, tier)
    if key not in _list_cache:
        params, grid = _case(name)
        with _context(params, grid, tier) as ctx:
            ctx.set_frequencies(L[:n])
            assert ctx.num_quantities == len(fu.labels(params, n))
            _list_cache[key] = _frozen(ctx.render())
    return _list_cache[key]


def _assert_bits(got, want, what):
    assert got.shape == want.shape, what
    same = gu.same_bits(got, want)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ"


def _distance(a, b):   # (tests/test_gpu_polarized_variants.py)
    scale = np.nanmax(np.abs(b), axis=-1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / scale
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def _assert_within_tier(got, want, polarized, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN mask")
    if polarized:
        distance = _distance(got, want)
        print(f"{what}: distance {distance:.3e}")
        assert distance < 1.0e-9, (what, distance)
    else:
        rel, above, used, same_support = gu.per_pixel_relative(got, want)
        print(f"{what}: per-pixel relative {rel:.3e} over {used} pixels")
        assert rel <= 1.0e-10 and same_support, (what, rel)


def _assert_rows_equal_fresh(name, n, tier="exact"):
    """Every row of every frequency of the list render at its offset, sample_num and sample_flags."""
    params, grid = _case(name)
    got = _list_render(name, n, tier)
    for l in range(n):
        want = _fresh(name, L[l], tier)
        rows = fu.rows_of(params, n, l)
        assert len(rows) == want["image"].shape[0]
        _assert_bits(got["image"][rows], want["image"], (name, n, l, tier))
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"]), (name, n, l)
    return got


# ---------------------------------------------------------------------------------------------------------------- exact tier: bits
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_exact_rows_have_the_bits_of_fresh_contexts_and_of_the_oracle(n, built_library):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    got = _assert_rows_equal_fresh("sim_dp_interp", n)
    st = got["stats"]
    assert st.arithmetic == 0 and st.n_chunks == 1
    params, grid = _case("sim_dp_interp")
    for l in range(n):
        p = bl.Params.from_dict(fu.one_frequency(params, L[l]))
        want = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=16 * 16, max_steps=int(p.get("ray_max_steps")))
        assert want["frequencies"][0] == L[l]
        _assert_bits(got["image"][l], want["image"][0], ("oracle", n, l))
        assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])
    if n >= 4:   # the duplicate's two rows
        _assert_bits(got["image"][2], got["image"][3], ("duplicate", n))


EXACT_CASES = [(case, n) for case in ("sim_aux_images", "sim_polarized", "sim_polarized_kappa_mix", "sim_powerlaw", "formula_flat", "sim_refined")
               for n in (1, 2, 3, 4, 5)] + [("slow_interp", 2), ("slow_interp", 4)]


@pytest.mark.parametrize("case,n", EXACT_CASES)
def test_exact_rows_of_every_kind_at_their_offsets(case, n, built_library):
    """Auxiliary rows (every row at its offset), Stokes rows 4 l + (I, Q, U, V) and tau, power-law electrons, formula mode, slow light,
    a mesh with refinement."""
    got = _assert_rows_equal_fresh(case, n)
    params, grid = _case(case)
    if n >= 4:
        _assert_bits(got["image"][fu.rows_of(params, n, 2)], got["image"][fu.rows_of(params, n, 3)], (case, "duplicate"))


# ---------------------------------------------------------------------------------------------------------------- tolerant tier
TOLERANT_CASES = [("sim_dp_interp", n) for n in (1, 2, 3, 4, 5)] + EXACT_CASES


@pytest.mark.parametrize("case,n", TOLERANT_CASES)
def test_tolerant_rows_within_the_tiers_bound_of_the_exact_rows(case, n, built_library):
    params, grid = _case(case)
    got, exact = _list_render(case, n, "tolerant"), _list_render(case, n, "exact")
    polarized = str(params.get("image_polarization", "false")).lower() == "true" and params["model_type"] == "simulation"
    assert np.array_equal(got["sample_num"], exact["sample_num"]) and np.array_equal(got["sample_flags"], exact["sample_flags"])
    for l in range(n):
        rows = fu.rows_of(params, n, l)
        _assert_within_tier(got["image"][rows], exact["image"][rows], polarized, (case, n, l))


# ---------------------------------------------------------------------------------------------------------------- with variants
PAIRS = [(1.0, 10.0), (1.0, 40.0), (2.0, 160.0)]   # (R_low, R_high)
UNITS = [1.0e-16, 3.0e-16]


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_models_x_units_x_frequencies(tier, built_library):
    """Three electron models x two units x L[:3]: in the tolerant tier one pass over the shared samples, each (model, unit, frequency)
    row within the bound of its fresh render; in the exact tier the same rows bit for bit."""
    params, grid = _case("sim_dp_interp")
    with _context(params, grid, tier) as ctx:
        ctx.set_electron_models([high for _, high in PAIRS], [low for low, _ in PAIRS])
        ctx.set_density_units(UNITS)
        ctx.set_frequencies(L[:3])
        assert ctx.num_quantities == 3 * 2 * 3
        got = ctx.render()
    st = got["stats"]
    if tier == "tolerant":
        assert st.arithmetic == 1 and st.launches_shade == st.n_chunks
    rows = got["image"].reshape(3, 2, 3, -1)
    for m, (low, high) in enumerate(PAIRS):
        for u, unit in enumerate(UNITS):
            for l in range(3):
                overrides = dict(plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=repr(unit))
                if tier == "exact":
                    _assert_bits(rows[m, u, l], _fresh("sim_dp_interp", L[l], "exact", **overrides)["image"][0], (m, u, l))
                else:
                    _assert_within_tier(rows[m, u, l], _fresh("sim_dp_interp", L[l], "exact", **overrides)["image"][0], False, (m, u, l))


def test_polarized_triples_x_frequencies(built_library):
    """Two polarized triples x L[:2], exact tier: rows v * n_q + 4 l + (I, Q, U, V) bit for bit."""
    params, grid = _case("sim_polarized")
    triples = [(1.0, 40.0, 3.0e-17), (2.0, 160.0, 3.0e-16)]   # (R_low, R_high, unit)
    with _context(params, grid, "exact") as ctx:
        ctx.set_polarized_variants([high for _, high, _ in triples], [unit for _, _, unit in triples], rat_low=[low for low, _, _ in triples])
        ctx.set_frequencies(L[:2])
        got = ctx.render()
    n_q = len(fu.labels(params, 2))
    assert got["image"].shape[0] == 2 * n_q
    for v, (low, high, unit) in enumerate(triples):
        for l in range(2):
            want = _fresh("sim_polarized", L[l], "exact", plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=repr(unit))
            rows = [v * n_q + q for q in fu.rows_of(params, 2, l)]
            _assert_bits(got["image"][rows], want["image"], (v, l))


# ---------------------------------------------------------------------------------------------------------------- with cameras
CAMERAS = [(60.0, 30.0), (163.0, 275.0)]


@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_two_cameras_x_three_frequencies(tier, built_library):
    params, grid = _case("sim_dp_interp")
    with _context(params, grid, tier) as ctx:
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        ctx.set_frequencies(L[:3])
        got = ctx.render()
        slices = [ctx.camera_slice(c) for c in range(2)]
    assert got["image"].shape == (3, 2 * 16 * 16)
    for c, (th, ph) in enumerate(CAMERAS):
        for l in range(3):
            want = _fresh("sim_dp_interp", L[l], "exact", camera_th=th, camera_ph=ph)
            assert np.array_equal(got["sample_num"][slices[c]], want["sample_num"]) and np.array_equal(got["sample_flags"][slices[c]], want["sample_flags"])
            if tier == "exact":
                _assert_bits(got["image"][l, slices[c]], want["image"][0], (c, l))
            else:
                _assert_within_tier(got["image"][l, slices[c]], want["image"][0], False, (c, l))


# ---------------------------------------------------------------------------------------------------------------- reuse
@pytest.mark.parametrize("tier", ["exact", "tolerant"])
def test_other_values_of_the_same_length_shade_the_resident_records(tier, built_library):
    params, grid = _case("sim_dp_interp")
    with _context(params, grid, tier) as ctx:
        ctx.set_reproducible(True)   # (tolerant tier: bits, so that the reused render can be held to a fresh context's)
        ctx.set_frequencies(L[:3])
        first = ctx.render()
        assert first["stats"].geodesics_reused == 0 and first["stats"].launches_geodesic >= 1
        ctx.set_frequencies(OTHER)
        second = ctx.render()
        assert second["stats"].geodesics_reused == 1 and second["stats"].launches_geodesic == 0
        # exact tier: the bits of a fresh context with that one frequency in its block. Tolerant tier (three frequencies and one take
        # different kernels there): the bits of a fresh context with the same list, and every pixel within the tier's bound of the exact row
        with _context(params, grid, tier) as fresh:
            fresh.set_reproducible(True)
            fresh.set_frequencies(OTHER)
            same_list = fresh.render()
        assert same_list["stats"].geodesics_reused == 0
        _assert_bits(second["image"], same_list["image"], (tier, "the same list, fresh"))
        for l, hz in enumerate(OTHER):
            want = _fresh("sim_dp_interp", hz, "exact")
            assert np.array_equal(second["sample_num"], want["sample_num"]) and np.array_equal(second["sample_flags"], want["sample_flags"])
            if tier == "exact":
                _assert_bits(second["image"][l], want["image"][0], (tier, l))
            else:
                _assert_within_tier(second["image"][l], want["image"][0], False, (tier, l))
        # a list of another length: reused wherever the plan chooses the same record layout, integrated again where it does not -
        # the rows are a fresh context's either way
        ctx.set_frequencies(L)
        third = ctx.render()
        for l, hz in enumerate(L):
            want = _fresh("sim_dp_interp", hz, "exact")
            if tier == "exact":
                _assert_bits(third["image"][l], want["image"][0], (tier, "five", l))
            else:
                _assert_within_tier(third["image"][l], want["image"][0], False, (tier, "five", l))


@pytest.mark.parametrize("case", ["sim_dp_interp", "sim_multifreq"])
def test_length_0_after_a_list_is_a_context_that_never_had_one(case, built_library):
    params, grid = _case(case)
    with _context(params, grid, "exact") as never:
        want = never.render()
    with _context(params, grid, "exact") as ctx:
        ctx.set_frequencies(L)
        ctx.render()
        ctx.set_frequencies([])
        got = ctx.render()
    _assert_bits(got["image"], want["image"], case)
    assert np.array_equal(got["sample_num"], want["sample_num"]) and np.array_equal(got["sample_flags"], want["sample_flags"])


def test_a_frame_of_several_chunks_kept_and_reused(built_library):
    """The kept layout of a frame of more than one chunk holds part of its record store in the tails of the per-frequency shading
    arrays: other values of the same length shade the kept chunks, a list of another length integrates again - the rows are a fresh
    context's both ways. The benchmark's path at 96^2 in a few chunks, as tests/test_gpu_series_chunked.py forces them."""
    import test_gpu_series_chunked as chunked
    from blacklight_amd import mock
    params = chunked._bench_params(96)
    grid = mock.generate(n_r=48, n_th=48, n_ph=48)
    cap = chunked._cap(chunked._one_chunk(params, grid, "exact"))

    def fresh(hz):
        return chunked._fresh(fu.one_frequency(params, hz), grid, "exact", cap)

    with chunked._context(params, "exact", cap=cap) as ctx:
        ctx.set_grid(grid)
        frames = [ctx.render() for _ in range(3)]   # several chunks, nothing kept; integrated in the kept layout; the kept chunks shaded
        chunked._reuse_flags(frames)
        ctx.set_frequencies([OTHER[0]])
        same_length = ctx.render()
        assert same_length["stats"].geodesics_reused == 1 and same_length["stats"].launches_geodesic == 0
        ctx.set_frequencies(L[:3])
        longer = ctx.render()
        assert longer["stats"].geodesics_reused == 0 and longer["stats"].n_chunks > 1
    _assert_bits(same_length["image"][0], fresh(OTHER[0])["image"][0], "kept, same length")
    for l in range(3):
        _assert_bits(longer["image"][l], fresh(L[l])["image"][0], ("kept, another length", l))


def test_a_saved_geodesic_checkpoint_carries_the_list(built_library, tmp_path):
    """... and a context that loads it - a block with as many frequencies, whatever their spacing - renders the list's rows."""
    path = str(tmp_path / "geodesics.ckpt")
    params, grid = _case("sim_dp_interp", checkpoint_geodesic_file=path)
    with _context(dict(params, checkpoint_geodesic_save="true"), grid, "exact") as ctx:
        ctx.set_frequencies(L[:3])
        saved = ctx.render()
    for l in range(3):
        _assert_bits(saved["image"][l], _fresh("sim_dp_interp", L[l], "exact")["image"][0], ("saving", l))
    loading = dict(params, checkpoint_geodesic_load="true", image_num_frequencies=3, image_frequency_start=1.0e11, image_frequency_end=3.0e11,
                   image_frequency_spacing="log")
    with _context(loading, grid, "exact") as ctx:
        got = ctx.render()
        assert got["stats"].ms_geodesic == 0.0 and ctx.frequencies.tolist() == L[:3]
    _assert_bits(got["image"], saved["image"], "loaded")
