"""Sigma cuts (bl_set_sigma_cuts, sweep_cut_sigma_max) on host-only contexts (no GPU): the C interface's symbols and struct sizes, the
key of the .input grammar (accepted forms and every error text, through the entry points that keep the list and through those that drop
it), the setter's argument errors and refusals, the row and file-name rule mMMuUUsSS of M x U x S variants, and
bl_write_output_variant: from fabricated rows, byte for byte the file a context with that cut_sigma_max in its block writes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import golden_util as gu
import sweep_util as su

BL_DEVICE_NONE = -2
BL_E_INPUT, BL_E_UNSUPPORTED, BL_E_ARG = 1, 3, 5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUTS = [0.01, 0.1, 1.0, 10.0, -1.0]
PAIRS_LOW, PAIRS_HIGH = [1.0, 2.0], [10.0, 160.0]
UNITS = [1.0e-16, 3.0e-16]


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return dict(params, **overrides)


# ---------------------------------------------------------------------------------------------------------------- exported symbols
def test_symbols_exported_and_declared(bl):
    from blacklight_amd import _capi
    lib = C.CDLL(bl.LIB_PATH)
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_set_sigma_cuts", "bl_num_sigma_cuts", "bl_params_set_line_sweeps", "bl_params_read_file_sweeps", "bl_apply_sweeps"):
        assert hasattr(lib, name), name
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_SIGMA_CUTS\s+16\b", header)
    assert re.search(r"typedef\s+struct\s+bl_sweep_cuts\s*\{\s*int32_t\s+n_sigma_max,\s*reserved;\s*double\s+sigma_max\[BL_MAX_SWEEP\];\s*\}\s*bl_sweep_cuts;", header)
    assert C.sizeof(_capi.Sweep) == 16 + 3 * 16 * 8          # bl_sweep is what it was
    assert C.sizeof(_capi.SweepCuts) == 8 + 16 * 8
    _capi.lib().bl_num_sigma_cuts.restype = C.c_int
    assert _capi.lib().bl_num_sigma_cuts(None) == -1          # no context


# ---------------------------------------------------------------------------------------------------------------- grammar
def test_accepted_forms(bl):
    p = bl.Params.from_text("""
        sweep_cut_sigma_max = 1, 3 ,1e1, -1     # the last one: the cut off
    """)
    assert p.has_sweep and p.sweep_cut_sigma_max == [1.0, 3.0, 10.0, -1.0]
    assert p.sweep_rat_low == [] and p.sweep_rho_cgs == []
    assert p.resolved_sweep() == (False, [], [], [])          # the 4-tuple of the three older lists stays what it was
    q = p.copy()
    p.set_line("sweep_cut_sigma_max = 0")                     # a later line replaces the list
    assert p.sweep_cut_sigma_max == [0.0] and q.sweep_cut_sigma_max == [1.0, 3.0, 10.0, -1.0]
    both = bl.Params.from_text("sweep_rho_cgs = 1e-16,2e-16\nsweep_cut_sigma_max = 0.5")
    assert both.sweep_rho_cgs == [1e-16, 2e-16] and both.sweep_cut_sigma_max == [0.5]
    sixteen = bl.Params.from_text("sweep_cut_sigma_max = " + ",".join(str(k) for k in range(16)))
    assert sixteen.sweep_cut_sigma_max == [float(k) for k in range(16)]
    plain = bl.Params.from_text("cut_sigma_max = 2")
    assert not plain.has_sweep and plain.sweep_cut_sigma_max == []


LINE_ERRORS = [
    ("sweep_cut_sigma_max = 1,,3", "Error: Empty entry in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max = 1,3,", "Error: Empty entry in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max =", "Error: Empty entry in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max = 1,three", "Error: Invalid number (three) in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max = 1x", "Error: Invalid number (1x) in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max = 1;3", "Error: Invalid number (1;3) in list (sweep_cut_sigma_max) in input file.\n"),
    ("sweep_cut_sigma_max = 1,nan", "Error: Invalid sigma cut (nan) in list (sweep_cut_sigma_max) in input file: must be finite.\n"),
    ("sweep_cut_sigma_max = inf", "Error: Invalid sigma cut (inf) in list (sweep_cut_sigma_max) in input file: must be finite.\n"),
    ("sweep_cut_sigma_max = 1,-inf", "Error: Invalid sigma cut (-inf) in list (sweep_cut_sigma_max) in input file: must be finite.\n"),
    ("sweep_cut_sigma_max = " + ",".join(["1"] * 17), "Error: Too many entries in list (sweep_cut_sigma_max) in input file: at most 16 for this build.\n"),
    ("sweep_cut_sigma_min = 1", "Error: Unknown key (sweep_cut_sigma_min) in input file.\n"),
]


@pytest.mark.parametrize("line,message", LINE_ERRORS)
def test_line_error_texts(bl, line, message):
    """... through the entry point that keeps the list and through the two that drop it (bl_params_set_line, bl_params_set_line_sweep)."""
    from blacklight_amd import _capi
    p = bl.Params()
    with pytest.raises(bl.BlacklightError) as err:
        p.set_line(line)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    text = C.create_string_buffer(1024)
    assert _capi.lib().bl_params_set_line(p.ptr, line.encode(), text, len(text)) == BL_E_INPUT
    assert text.value.decode() == message
    text = C.create_string_buffer(1024)
    sweep = _capi.Sweep()
    assert _capi.lib().bl_params_set_line_sweep(p.ptr, C.byref(sweep), line.encode(), text, len(text)) == BL_E_INPUT
    assert text.value.decode() == message


def test_the_older_entry_points_accept_the_key_and_drop_it(bl, tmp_path):
    from blacklight_amd import _capi
    L = _capi.lib()
    size = L.bl_params_sizeof()
    params = _case("sim_multifreq")
    plain = su.write_input(tmp_path / "plain.input", params)
    swept = su.write_input(tmp_path / "swept.input", dict(params, sweep_cut_sigma_max="1,3,-1", sweep_rho_cgs="2e-16"))
    bad = su.write_input(tmp_path / "bad.input", dict(params, sweep_cut_sigma_max="1,nan"))
    want = bl.Params.from_file(plain)
    kept = bl.Params.from_file(swept)
    assert kept.sweep_cut_sigma_max == [1.0, 3.0, -1.0] and kept.sweep_rho_cgs == [2e-16] and not want.has_sweep
    assert C.string_at(kept.ptr, size) == C.string_at(want.ptr, size)   # the key never enters the block
    text, runs = C.create_string_buffer(1024), C.c_int(0)
    old = bl.Params()
    assert L.bl_params_read_file(old.ptr, swept.encode(), C.byref(runs), text, len(text)) == 0, text.value
    assert C.string_at(old.ptr, size) == C.string_at(want.ptr, size) and runs.value == want.num_runs
    older, sweep = bl.Params(), _capi.Sweep()
    assert L.bl_params_read_file_sweep(older.ptr, C.byref(sweep), swept.encode(), C.byref(runs), text, len(text)) == 0, text.value
    assert C.string_at(older.ptr, size) == C.string_at(want.ptr, size) and (sweep.n_rho_cgs, sweep.n_rat_low) == (1, 0)
    message = "Error: Invalid sigma cut (nan) in list (sweep_cut_sigma_max) in input file: must be finite.\n"
    for call, extra in ((L.bl_params_read_file, ()), (L.bl_params_read_file_sweep, (C.byref(sweep),))):
        text = C.create_string_buffer(1024)
        assert call(bl.Params().ptr, *extra, bad.encode(), None, text, len(text)) == BL_E_INPUT
        assert text.value.decode() == message
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_file(bad)
    assert str(err.value) + "\n" == message
    by_line = bl.Params.from_dict(params)
    before = C.string_at(by_line.ptr, size)
    by_line.set_line("sweep_cut_sigma_max = 1,10")
    assert C.string_at(by_line.ptr, size) == before


# ---------------------------------------------------------------------------------------------------------------- the setter
def test_setter_arguments_and_counts(bl):
    with bl.Context(bl.Params.from_dict(_case("sim_multifreq")), device=BL_DEVICE_NONE) as ctx:
        n_q = ctx.num_quantities
        assert (ctx.num_sigma_cuts, ctx.sigma_cuts, ctx.num_variants) == (0, [], 1)
        ctx.set_sigma_cuts(CUTS)
        assert (ctx.num_sigma_cuts, ctx.sigma_cuts, ctx.num_variants, ctx.num_quantities) == (5, CUTS, 5, 5 * n_q)
        for bad in ([1.0, math.nan], [math.inf], [-math.inf, 1.0]):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_sigma_cuts(bad)
            assert err.value.code == BL_E_ARG and "is not finite" in str(err.value)
            assert ctx.num_sigma_cuts == 5          # a failed call changes nothing
        with pytest.raises(bl.BlacklightError) as err:
            ctx.set_sigma_cuts([1.0] * 17)
        assert err.value.code == BL_E_ARG and "0 <= n <= 16" in str(err.value)
        assert ctx._lib.bl_set_sigma_cuts(ctx._ctx, 2, None) == BL_E_ARG and ctx.num_sigma_cuts == 5
        ctx.set_sigma_cuts(3.0)                     # a scalar: one cut, in place of the block's
        assert (ctx.num_sigma_cuts, ctx.num_variants, ctx.num_quantities) == (1, 1, n_q)
        ctx.set_sigma_cuts([1.0] * 16)
        assert ctx.num_variants == 16
        ctx.set_electron_models(PAIRS_HIGH, rat_low=PAIRS_LOW)
        ctx.set_density_units(UNITS)
        assert (ctx.num_variants, ctx.num_quantities) == (2 * 2 * 16, 64 * n_q)
        ctx.set_sigma_cuts([])
        assert (ctx.num_sigma_cuts, ctx.num_variants) == (0, 4)


REFUSALS = [
    ("formula_flat", {}, 1, "Error: Sigma cuts: formula mode has no magnetisation (model_type = formula)."),
    ("sim_polarized", {}, 1, "Error: Sigma cuts: the polarized axis is not built yet; polarized runs render one sigma cut (image_polarization = true)."),
    ("sim_adaptive", {}, 2, "Error: Sigma cuts: adaptive refinement reads one image; n >= 2 cuts need adaptive_max_level = 0."),
    ("sim_render", {}, 2, "Error: Sigma cuts: a cut cell drops out of a rendering, and renderings come out once; n >= 2 cuts need render_num_images = 0."),
]


@pytest.mark.parametrize("case,overrides,least,message", REFUSALS)
def test_refusals(bl, case, overrides, least, message):
    """BL_E_UNSUPPORTED in the refusal's words, from the setter and - through the sweep key - from bl_apply_sweeps, which leaves no list."""
    params = _case(case, **overrides)
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        if least == 2:
            ctx.set_sigma_cuts([3.0])               # one cut is a single image: allowed
            assert ctx.num_sigma_cuts == 1
            ctx.set_sigma_cuts([])
        with pytest.raises(bl.BlacklightError) as err:
            ctx.set_sigma_cuts([1.0, 3.0])
        assert str(err.value) == message and err.value.code == BL_E_UNSUPPORTED
        assert ctx.num_sigma_cuts == 0 and ctx.num_variants == 1
    p = bl.Params.from_dict(params)
    p.set_line("sweep_cut_sigma_max = 1,3")
    with pytest.raises(bl.BlacklightError) as swept:
        bl.Context(p, device=BL_DEVICE_NONE)
    assert str(swept.value) == message and swept.value.code == BL_E_UNSUPPORTED


def test_slow_light_is_refused(bl):
    with bl.Context(bl.Params.from_dict(_case("slow_interp")), device=BL_DEVICE_NONE) as ctx:
        with pytest.raises(bl.BlacklightError) as err:
            ctx.set_sigma_cuts([1.0])
        assert str(err.value) == "Error: Sigma cuts: slow light renders one sigma cut (slow_light_on = true)." and err.value.code == BL_E_UNSUPPORTED
        assert ctx.num_sigma_cuts == 0


def test_a_refused_cut_list_leaves_no_other_list(bl):
    from blacklight_amd import _capi
    with bl.Context(bl.Params.from_dict(_case("sim_render")), device=BL_DEVICE_NONE) as ctx:
        sweep, cuts = _capi.Sweep(), _capi.SweepCuts()
        sweep.n_rat_low = sweep.n_rat_high = 1                # one model: a single image, which renderings allow
        sweep.rat_low[0], sweep.rat_high[0] = 1.0, 40.0
        cuts.n_sigma_max = 2
        cuts.sigma_max[0], cuts.sigma_max[1] = 1.0, 3.0
        assert ctx._lib.bl_apply_sweeps(ctx._ctx, C.byref(sweep), C.byref(cuts)) == BL_E_UNSUPPORTED
        assert "Sigma cuts: a cut cell drops out of a rendering" in ctx._lib.bl_last_error(ctx._ctx).decode()
        assert (ctx.num_electron_models, ctx.num_sigma_cuts, ctx.num_variants) == (0, 0, 1)
        cuts.n_sigma_max = 1
        assert ctx._lib.bl_apply_sweeps(ctx._ctx, C.byref(sweep), C.byref(cuts)) == 0
        assert (ctx.num_electron_models, ctx.num_sigma_cuts, ctx.num_variants) == (1, 1, 1)
        assert ctx._lib.bl_apply_sweeps(ctx._ctx, C.byref(sweep), None) == 0   # no cuts: bl_apply_sweep
        cuts.n_sigma_max = 17
        assert ctx._lib.bl_apply_sweeps(ctx._ctx, C.byref(sweep), C.byref(cuts)) == BL_E_INPUT


def test_single_image_calls_refuse_two_cuts(bl, tmp_path):
    p = bl.Params.from_dict(_case("sim_multifreq", output_file=str(tmp_path / "a.npz")))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        ctx.set_sigma_cuts([1.0, 3.0])
        image = np.zeros((ctx.num_quantities, ctx.resolution ** 2))
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output([dict(image=image, block_locs=None)])
        assert err.value.code == BL_E_UNSUPPORTED and "the reference's file layout has no sigma-cut axis" in str(err.value)
        flags, count = np.zeros(4, dtype=np.uint8), C.c_int32(0)
        rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 4, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(count), None)
        assert rc == BL_E_UNSUPPORTED and "not with two or more sigma cuts (bl_set_sigma_cuts)" in ctx._lib.bl_last_error(ctx._ctx).decode()


# ---------------------------------------------------------------------------------------------------------------- rows, names, files
def _rows(rng, n_rows, n_pix):
    image = rng.standard_normal((n_rows, n_pix)) * 10.0 ** rng.integers(-30, 5, size=(n_rows, 1))
    image[rng.random(image.shape) < 0.02] = np.nan
    return np.ascontiguousarray(image)


def test_names_follow_the_row_rule(bl, tmp_path):
    """Variant (m U + u) S + s is named mMMuUUsSS; without cuts the names are what they were."""
    params = _case("sim_dp_interp", simulation_multiple="true", simulation_start=7, simulation_end=9, output_file=str(tmp_path / "out.d/img_{04d}.npz"))
    p = bl.Params.from_dict(params)
    p.set_line("sweep_rat_low = 1,1,1")
    p.set_line("sweep_rat_high = 10,40,160")
    p.set_line("sweep_rho_cgs = 1e-16,2e-16")
    p.set_line("sweep_cut_sigma_max = " + su.comma(CUTS))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert (ctx.num_electron_models, ctx.num_density_units, ctx.num_sigma_cuts, ctx.num_variants) == (3, 2, 5, 30)
        assert ctx.sigma_cuts == CUTS
        names = [ctx.variant_output_path(2, v) for v in range(30)]
        assert names == [str(tmp_path / f"out.d/img_0009.m{m:02d}u{u:02d}s{s:02d}.npz") for m in range(3) for u in range(2) for s in range(5)]
        assert names == sorted(names)
        ctx.set_sigma_cuts([])
        assert ctx.variant_output_path(2, 3) == str(tmp_path / "out.d/img_0009.m01u01.npz")
    q = bl.Params.from_dict(_case("sim_dp_interp", output_file="image.npz"))
    q.set_line("sweep_cut_sigma_max = 1,3,10")
    with bl.Context(q, device=BL_DEVICE_NONE) as ctx:       # cuts alone
        assert [ctx.variant_output_path(0, v) for v in range(3)] == ["image.m00u00s00.npz", "image.m00u00s01.npz", "image.m00u00s02.npz"]
        ctx.set_sigma_cuts([3.0])                           # one image: the plain name
        assert ctx.variant_output_path(0, 0) == "image.npz"


@pytest.mark.parametrize("fmt", ["npz", "npy", "raw"])
def test_variant_files_equal_single_runs(bl, tmp_path, fmt):
    """M x U x S = 2 x 2 x 3 with two frequencies, an auxiliary row and the camera record: each file is, byte for byte, what a context
    with that pair, unit and cut_sigma_max in its block writes from that variant's rows."""
    cuts = [0.1, 1.0, -1.0]
    params = _case("sim_multifreq", image_num_frequencies=2, image_tau="true", output_camera="true", output_format=fmt,
                   output_file=str(tmp_path / f"sweep.{fmt}"))
    p = bl.Params.from_dict(params)
    for line in (f"sweep_rat_low = {su.comma(PAIRS_LOW)}", f"sweep_rat_high = {su.comma(PAIRS_HIGH)}", f"sweep_rho_cgs = {su.comma(UNITS)}",
                 f"sweep_cut_sigma_max = {su.comma(cuts)}"):
        p.set_line(line)
    rng = np.random.default_rng(20261018)
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_variants == 12
        n_q, n_pix = ctx.num_quantities // 12, ctx.resolution ** 2
        image = _rows(rng, 12 * n_q, n_pix)
        level = dict(image=image, block_locs=None, camera_pos=rng.standard_normal((n_pix, 4)))
        names = []
        for v in range(12):
            ctx.write_output([level], variant=v)
            names.append(ctx.variant_output_path(0, v))
    assert [os.path.basename(n) for n in names] == [f"sweep.m{m:02d}u{u:02d}s{s:02d}.{fmt}" for m in range(2) for u in range(2) for s in range(3)]
    for m in range(2):
        for u in range(2):
            for s in range(3):
                v = (m * 2 + u) * 3 + s
                single = dict(params, plasma_rat_low=PAIRS_LOW[m], plasma_rat_high=PAIRS_HIGH[m], simulation_rho_cgs=UNITS[u], cut_sigma_max=cuts[s],
                              output_file=str(tmp_path / f"single_{v}.{fmt}"))
                with bl.Context(bl.Params.from_dict(single), device=BL_DEVICE_NONE) as plain:
                    assert plain.num_quantities == n_q
                    plain.write_output([dict(level, image=image[v * n_q:(v + 1) * n_q])])
                assert su.file_bytes(names[v]) == su.file_bytes(single["output_file"]), (fmt, m, u, s)
