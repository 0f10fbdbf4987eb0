"""Several cameras in one render, on host-only contexts (no GPU): the sweep_camera_th / sweep_camera_ph keys of the grammar (accepted
forms, every error text, the broadcast and absent rules, existing parser calls drop the keys), bl_set_cameras (each camera's frame is
bit for bit the frame of a context initialised with those angles in its block; argument errors and refusals change nothing), the
file names, and bl_write_output_camera: byte for byte the file a context with that camera's angles in its block writes from the
camera's slice of every row and record."""
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

CAMERAS = [(0.0, 0.0), (60.0, 30.0), (163.0, 275.0), (180.0, 45.0)]   # both poles among them


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return dict(params, **overrides)


def _frame_values(frame):
    """Every member of a bl_camera_frame, as its bytes: bit for bit, a NaN included."""
    return bytes(frame)


# ---------------------------------------------------------------------------------------------------------------- exported symbols
def test_camera_symbols_exported_and_declared(bl):
    lib = C.CDLL(bl.LIB_PATH)
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_set_cameras", "bl_num_cameras", "bl_camera_frame_get_camera", "bl_cameras_get", "bl_write_output_camera", "bl_camera_output_path",
                 "bl_params_set_line_sweeps_cameras", "bl_params_read_file_sweeps_cameras", "bl_sweep_cameras_resolve", "bl_apply_sweeps_cameras"):
        assert hasattr(lib, name), name
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_CAMERAS\s+16\b", header)
    from blacklight_amd import _capi
    assert C.sizeof(_capi.SweepCameras) == 8 + 2 * 16 * 8
    assert C.sizeof(_capi.Sweep) == 16 + 3 * 16 * 8 and C.sizeof(_capi.SweepCuts) == 8 + 16 * 8   # the two earlier structs are ABI
    assert _capi.Stats._fields_[-1] == ("n_cameras", C.c_int32)   # at the end of bl_stats
    assert re.search(r"int32_t\s+n_cameras;[^}]*\}\s*bl_stats;", header, re.S)


# ---------------------------------------------------------------------------------------------------------------- grammar
def test_accepted_forms_and_the_broadcast_and_absent_rules(bl):
    p = bl.Params.from_text("""
        sweep_camera_th = 17, 60 ,163     # degrees
        sweep_camera_ph = 0,0, 9.0e1
    """)
    assert p.has_sweep
    assert p.sweep_camera_th == [17.0, 60.0, 163.0] and p.sweep_camera_ph == [0.0, 0.0, 90.0]
    assert p.sweep_cameras == [(17.0, 0.0), (60.0, 0.0), (163.0, 90.0)]
    q = p.copy()
    p.set_line("sweep_camera_ph = 45")   # one entry: every th at that ph; a later line replaces the list
    assert p.sweep_cameras == [(17.0, 45.0), (60.0, 45.0), (163.0, 45.0)] and q.sweep_camera_ph == [0.0, 0.0, 90.0]
    only_th = bl.Params.from_text("sweep_camera_th = 0, 180")   # ph absent: the block's own (None here)
    assert only_th.sweep_cameras == [(0.0, None), (180.0, None)]
    only_ph = bl.Params.from_text("sweep_camera_ph = 0, 120, 240")   # ph without th: the block's camera_th at each ph
    assert only_ph.sweep_cameras == [(None, 0.0), (None, 120.0), (None, 240.0)]
    sixteen = bl.Params.from_text("sweep_camera_th = " + ",".join(str(10 * k + 5) for k in range(16)))
    assert len(sixteen.sweep_cameras) == 16
    negative = bl.Params.from_text("sweep_camera_th = -20.5\nsweep_camera_ph = 400")   # (what bl_init takes for camera_th, the list takes)
    assert negative.sweep_cameras == [(-20.5, 400.0)]
    plain = bl.Params.from_text("camera_r = 50")
    assert not plain.has_sweep and plain.sweep_cameras == []


LINE_ERRORS = [
    ("sweep_camera_th = 17,,60", "Error: Empty entry in list (sweep_camera_th) in input file.\n"),
    ("sweep_camera_ph = 0,90,", "Error: Empty entry in list (sweep_camera_ph) in input file.\n"),
    ("sweep_camera_th = ,1", "Error: Empty entry in list (sweep_camera_th) in input file.\n"),
    ("sweep_camera_th =", "Error: Empty entry in list (sweep_camera_th) in input file.\n"),
    ("sweep_camera_ph = 10,ninety", "Error: Invalid number (ninety) in list (sweep_camera_ph) in input file.\n"),
    ("sweep_camera_th = 60deg", "Error: Invalid number (60deg) in list (sweep_camera_th) in input file.\n"),
    ("sweep_camera_th = 17;60", "Error: Invalid number (17;60) in list (sweep_camera_th) in input file.\n"),
    ("sweep_camera_th = 17,nan", "Error: Invalid angle (nan) in list (sweep_camera_th) in input file: must be finite.\n"),
    ("sweep_camera_ph = inf", "Error: Invalid angle (inf) in list (sweep_camera_ph) in input file: must be finite.\n"),
    ("sweep_camera_th = " + ",".join(["60"] * 17), "Error: Too many entries in list (sweep_camera_th) in input file: at most 16 for this build.\n"),
    ("sweep_camera_ph = " + ",".join(["0"] * 17), "Error: Too many entries in list (sweep_camera_ph) in input file: at most 16 for this build.\n"),
    ("sweep_camera_psi = 1", "Error: Unknown key (sweep_camera_psi) in input file.\n"),
]


@pytest.mark.parametrize("line,message", LINE_ERRORS)
def test_line_error_texts(bl, line, message):
    """... through the entry point that keeps the lists and through every one that drops them."""
    from blacklight_amd import _capi
    L = _capi.lib()
    p = bl.Params()
    with pytest.raises(bl.BlacklightError) as err:
        p.set_line(line)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    text = C.create_string_buffer(1024)
    assert L.bl_params_set_line(p.ptr, line.encode(), text, len(text)) == BL_E_INPUT and text.value.decode() == message
    text = C.create_string_buffer(1024)
    assert L.bl_params_set_line_sweep(p.ptr, None, line.encode(), text, len(text)) == BL_E_INPUT and text.value.decode() == message
    text = C.create_string_buffer(1024)
    assert L.bl_params_set_line_sweeps(p.ptr, None, None, line.encode(), text, len(text)) == BL_E_INPUT and text.value.decode() == message


def test_lengths_that_do_not_fit_are_an_error_of_the_file(bl, tmp_path):
    from blacklight_amd import _capi
    message = "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (2 and 3) in input file.\n"
    path = su.write_input(tmp_path / "bad.input", dict(_case("sim_multifreq"), sweep_camera_th="17,60,163", sweep_camera_ph="0,90"))
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_file(path)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    for reader in ("bl_params_read_file", ):   # ... and of the entry points that keep no camera lists: the command-line contract
        block, text = bl.Params(), C.create_string_buffer(1024)
        assert getattr(_capi.lib(), reader)(block.ptr, path.encode(), None, text, len(text)) == BL_E_INPUT
        assert text.value.decode() == message
    block, text = bl.Params(), C.create_string_buffer(1024)
    assert _capi.lib().bl_params_read_file_sweeps(block.ptr, None, None, path.encode(), None, text, len(text)) == BL_E_INPUT
    assert text.value.decode() == message
    # line by line there is no end of file: the lists are held against each other when they are resolved or applied
    p = bl.Params.from_dict(_case("sim_multifreq"))
    p.set_line("sweep_camera_th = 17,60,163")
    p.set_line("sweep_camera_ph = 0,90")
    with pytest.raises(bl.BlacklightError) as err:
        p.sweep_cameras
    assert str(err.value) + "\n" == message
    with pytest.raises(bl.BlacklightError) as err:
        bl.Context(p, device=BL_DEVICE_NONE)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    four_to_one = bl.Params.from_text("sweep_camera_th = 60\nsweep_camera_ph = 0,90,180,270")   # (ph longer than th fits no rule either)
    with pytest.raises(bl.BlacklightError) as err:
        four_to_one.sweep_cameras
    assert str(err.value) == "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (4 and 1) in input file."


def test_existing_parser_calls_accept_the_keys_and_drop_them(bl, tmp_path):
    """The block of a file with the camera keys is, byte for byte, the block of the file without them - through every reader - and the
    readers that know only the earlier lists fill those as ever."""
    from blacklight_amd import _capi
    L = _capi.lib()
    size = L.bl_params_sizeof()
    for case in ("sim_dp_interp", "sim_polarized", "formula_64"):
        params = _case(case)
        plain = su.write_input(tmp_path / f"{case}.input", params)
        keyed = su.write_input(tmp_path / f"{case}_cameras.input", dict(params, sweep_camera_th="17,60,163", sweep_camera_ph="0,0,90"))
        old, text, runs = bl.Params(), C.create_string_buffer(1024), C.c_int(0)
        assert L.bl_params_read_file(old.ptr, plain.encode(), C.byref(runs), text, len(text)) == 0, text.value
        want = C.string_at(old.ptr, size)
        for path in (plain, keyed):
            block = bl.Params()
            assert L.bl_params_read_file(block.ptr, path.encode(), None, text, len(text)) == 0, text.value
            assert C.string_at(block.ptr, size) == want
            sweep, cuts = _capi.Sweep(), _capi.SweepCuts()
            assert L.bl_params_read_file_sweep(block.ptr, C.byref(sweep), path.encode(), None, text, len(text)) == 0
            assert C.string_at(block.ptr, size) == want and sweep.n_rat_low == 0 and sweep.n_rho_cgs == 0
            assert L.bl_params_read_file_sweeps(block.ptr, C.byref(sweep), C.byref(cuts), path.encode(), None, text, len(text)) == 0
            assert C.string_at(block.ptr, size) == want and cuts.n_sigma_max == 0
        with_keys = bl.Params.from_file(keyed)
        assert C.string_at(with_keys.ptr, size) == want and with_keys.num_runs == runs.value
        assert with_keys.sweep_cameras == [(17.0, 0.0), (60.0, 0.0), (163.0, 90.0)] and not bl.Params.from_file(plain).has_sweep
        by_line = bl.Params.from_dict(params)
        before = C.string_at(by_line.ptr, size)
        by_line.set_line("sweep_camera_th = 0,180")
        assert C.string_at(by_line.ptr, size) == before


# ---------------------------------------------------------------------------------------------------------------- the setter
@pytest.mark.parametrize("case", ["sim_dp_interp", "sim_spin_fallback", "sim_pinhole_camera_norm", "formula_64", "formula_flat"])
def test_each_cameras_frame_is_a_fresh_contexts(bl, case):
    """... bit for bit, every member of bl_camera_frame - the pole branch (th = 0, th = 180), a spinning hole, a flat spacetime."""
    params = _case(case)
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        own = _frame_values(ctx.camera_frame)
        assert ctx.num_cameras == 0 and ctx.cameras == [] and _frame_values(ctx.camera_frame_of(0)) == own
        ctx.set_cameras([th for th, _ in CAMERAS], [ph for _, ph in CAMERAS])
        assert ctx.num_cameras == len(CAMERAS) and ctx.cameras == CAMERAS
        assert ctx.level_pixels(0) == len(CAMERAS) * ctx.resolution ** 2
        assert ctx.camera_slice(2) == slice(2 * ctx.resolution ** 2, 3 * ctx.resolution ** 2)
        assert _frame_values(ctx.camera_frame) == own   # (bl_camera_frame_get: the block's own while the list holds several)
        for c, (th, ph) in enumerate(CAMERAS):
            with bl.Context(bl.Params.from_dict(dict(params, camera_th=th, camera_ph=ph)), device=BL_DEVICE_NONE) as fresh:
                want = _frame_values(fresh.camera_frame)
            assert _frame_values(ctx.camera_frame_of(c)) == want, (case, c)
        with pytest.raises(IndexError):
            ctx.camera_frame_of(len(CAMERAS))
        with pytest.raises(IndexError):
            ctx.camera_slice(-1)
        ctx.set_cameras(163.0, 275.0)   # a list of one: that camera is the context's
        with bl.Context(bl.Params.from_dict(dict(params, camera_th=163.0, camera_ph=275.0)), device=BL_DEVICE_NONE) as fresh:
            assert _frame_values(ctx.camera_frame) == _frame_values(fresh.camera_frame) == _frame_values(ctx.camera_frame_of(0))
        assert ctx.level_pixels(0) == ctx.resolution ** 2
        ctx.set_cameras([])             # n = 0 restores the block's own camera
        assert ctx.num_cameras == 0 and _frame_values(ctx.camera_frame) == own


def test_the_pole_is_the_written_value_not_the_angle(bl):
    """camera_pole is set for a written value of exactly 0 or 180, as the parser sets it - 360 is not a pole, nor is 1e-300."""
    params = _case("sim_dp_interp")
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_cameras([360.0, 1.0e-300, -0.0], [10.0, 10.0, 10.0])
        for c, th in enumerate(("360.0", "1e-300", "-0.0")):
            with bl.Context(bl.Params.from_dict(dict(params, camera_th=th, camera_ph=10.0)), device=BL_DEVICE_NONE) as fresh:
                assert _frame_values(ctx.camera_frame_of(c)) == _frame_values(fresh.camera_frame), th


def test_sweep_keys_end_in_the_setter_with_the_blocks_own_angles_to_the_bit(bl, tmp_path):
    """An absent list means the block's radians themselves: 33.3 degrees is a value whose radians no round trip through degrees need hit."""
    params = _case("sim_dp_interp", camera_th=33.3, camera_ph=211.7)
    path = su.write_input(tmp_path / "th.input", dict(params, sweep_camera_th="17,60"))
    with bl.Context.from_input(path, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_cameras == 2 and [th for th, _ in ctx.cameras] == [17.0, 60.0]
        for c, th in enumerate((17.0, 60.0)):
            with bl.Context(bl.Params.from_dict(dict(params, camera_th=th)), device=BL_DEVICE_NONE) as fresh:
                assert _frame_values(ctx.camera_frame_of(c)) == _frame_values(fresh.camera_frame)
    path = su.write_input(tmp_path / "ph.input", dict(params, sweep_camera_ph="0,120,240"))
    with bl.Context.from_input(path, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_cameras == 3
        for c, ph in enumerate((0.0, 120.0, 240.0)):
            with bl.Context(bl.Params.from_dict(dict(params, camera_ph=ph)), device=BL_DEVICE_NONE) as fresh:
                assert _frame_values(ctx.camera_frame_of(c)) == _frame_values(fresh.camera_frame)
    both = su.write_input(tmp_path / "both.input", dict(params, sweep_camera_th="0,60,163", sweep_camera_ph="0,30,275", sweep_rat_low="1,1",
                                                      sweep_rat_high="10,40"))
    with bl.Context.from_input(both, device=BL_DEVICE_NONE) as ctx:
        assert ctx.cameras == CAMERAS[:3] and ctx.num_electron_models == 2 and ctx.num_variants == 2
        assert ctx.num_quantities == 2   # cameras multiply rays, not rows
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_cameras([10.0, 20.0])
        ctx.apply_sweep()   # an empty sweep makes no call
        assert ctx.num_cameras == 2


def test_argument_errors_change_nothing(bl):
    params = _case("sim_dp_interp")
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_cameras([17.0, 60.0], [0.0, 90.0])
        held = [_frame_values(ctx.camera_frame_of(c)) for c in range(2)]
        L, handle = ctx._lib, ctx._ctx
        th, ph = (C.c_double * 17)(*([60.0] * 17)), (C.c_double * 17)(*([0.0] * 17))
        for n, a, b in ((-1, th, ph), (17, th, ph), (2, None, ph), (2, th, None)):
            assert L.bl_set_cameras(handle, n, a, b) == BL_E_ARG
            assert "bl_set_cameras needs 0 <= n <= 16 and both arrays of angles." in L.bl_last_error(handle).decode()
        for bad, which in ((math.nan, "th"), (math.inf, "ph"), (-math.inf, "th")):
            angles = {"th": [17.0, 60.0, 163.0], "ph": [0.0, 0.0, 0.0]}
            angles[which][2] = bad
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_cameras(angles["th"], angles["ph"])
            assert err.value.code == BL_E_ARG and str(err.value) == "Error: bl_set_cameras: camera 2 has an angle that is not finite."
        assert L.bl_set_cameras(None, 0, None, None) == BL_E_ARG and L.bl_num_cameras(None) == -1
        assert ctx.num_cameras == 2 and ctx.cameras == [(17.0, 0.0), (60.0, 90.0)]
        assert [_frame_values(ctx.camera_frame_of(c)) for c in range(2)] == held
        assert L.bl_set_cameras(handle, 0, None, None) == 0 and ctx.num_cameras == 0   # n = 0 needs no arrays


REFUSALS = [
    ("sim_adaptive", {}, 2, "Error: Cameras: adaptive refinement reads one image; n >= 2 cameras need adaptive_max_level = 0."),
    ("slow_interp", {}, 2, "Error: Cameras: slow light renders one camera (slow_light_on = true)."),
    ("sim_dp_interp", dict(checkpoint_geodesic_save="true", checkpoint_geodesic_file="geo.bin"), 2,
     "Error: Cameras: a geodesic checkpoint holds one camera; n >= 2 cameras need checkpoint_geodesic_save = false."),
    ("sim_dp_interp", dict(checkpoint_geodesic_load="true", checkpoint_geodesic_file="geo.bin"), 1,
     "Error: Cameras: a geodesic checkpoint carries its own camera (checkpoint_geodesic_load = true)."),
    ("sim_dp_interp", dict(checkpoint_sample_save="true", checkpoint_sample_file="samples.bin"), 2,
     "Error: Cameras: a sample checkpoint holds one camera; n >= 2 cameras need checkpoint_sample_save = false."),
    ("sim_dp_interp", dict(cut_omit_near="true"), 2, "Error: Cameras: cut_omit_near and cut_omit_far compare with one camera position; n >= 2 cameras need both off."),
    ("sim_dp_interp", dict(cut_omit_far="true"), 2, "Error: Cameras: cut_omit_near and cut_omit_far compare with one camera position; n >= 2 cameras need both off."),
    ("sim_dp_interp", dict(image_crossings="true"), 2, "Error: Cameras: image_crossings counts crossings of one camera's plane; n >= 2 cameras need image_crossings = false."),
]


@pytest.mark.parametrize("case,overrides,smallest,message", REFUSALS)
def test_refusals_come_in_one_sentence_and_change_nothing(bl, tmp_path, case, overrides, smallest, message):
    if case.startswith("slow_"):
        params = json_params(case)
    else:
        params = _case(case, **overrides)
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        own = _frame_values(ctx.camera_frame)
        if smallest == 2:
            ctx.set_cameras(60.0, 30.0)   # one camera is a render of its own: accepted
            ctx.set_cameras([])
        with pytest.raises(bl.BlacklightError) as err:
            ctx.set_cameras([17.0, 60.0][:smallest], [0.0, 90.0][:smallest])
        assert err.value.code == BL_E_UNSUPPORTED and str(err.value) == message
        assert ctx.num_cameras == 0 and _frame_values(ctx.camera_frame) == own
    p = bl.Params.from_dict(params)   # ... and from the .input keys, in the same words
    p.set_line("sweep_camera_th = 17,60")
    with pytest.raises(bl.BlacklightError) as err:
        bl.Context(p, device=BL_DEVICE_NONE)
    assert err.value.code == BL_E_UNSUPPORTED and str(err.value) == message


def json_params(case):
    import json
    fx = np.load(os.path.join(gu.GOLDEN_DIR, f"{case}.npz"), allow_pickle=False)
    return json.loads(str(fx["params"]))


def test_a_refused_sweep_leaves_no_cameras_behind(bl):
    """The cameras are accepted, the electron models after them are not (formula mode): the call leaves neither."""
    p = bl.Params.from_dict(_case("formula_64"))
    p.set_line("sweep_camera_th = 17,60")
    p.set_line("sweep_rat_low = 1,1")
    p.set_line("sweep_rat_high = 10,40")
    with bl.Context(bl.Params.from_dict(_case("formula_64")), device=BL_DEVICE_NONE) as ctx:
        with pytest.raises(bl.BlacklightError) as err:
            ctx.apply_sweep(p)
        assert err.value.code == BL_E_UNSUPPORTED and "formula" in str(err.value)
        assert ctx.num_cameras == 0 and ctx.num_electron_models == 0


def test_host_steps_refuse_several_cameras(bl, tmp_path):
    """bl_write_output and bl_write_output_variant (the reference's file holds one camera) and bl_adaptive_refine; Python's flux fits
    and distributed renders raise ValueError."""
    params = _case("sim_dp_interp", camera_resolution=8, adaptive_block_size=8, output_file=str(tmp_path / "out.npz"))
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_cameras([17.0, 60.0], [0.0, 0.0])
        image = np.zeros((ctx.num_quantities, ctx.level_pixels(0)))
        level = dict(image=image, block_locs=None)
        for kwargs in ({}, {"variant": 0}):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([level], **kwargs)
            assert err.value.code == BL_E_UNSUPPORTED and "the reference's file holds one camera" in str(err.value)
        with pytest.raises(bl.BlacklightError) as err:
            ctx.adaptive_refine(0, image[:, :64])
        assert err.value.code == BL_E_UNSUPPORTED and "not with two or more cameras (bl_set_cameras)" in str(err.value)
        with pytest.raises(ValueError, match="two or more cameras"):
            ctx.fit_density_unit(1.0, 1.0e7, 1e-18, 1e-14)
        with pytest.raises(ValueError, match="two or more cameras"):
            ctx.fit_density_units_polarized([(10.0, 1.0)], 1.0, 1.0e7, 1e-18, 1e-14)
        from blacklight_amd import distributed

        class Comm:
            rank, world = 0, 1
        for call in (lambda: distributed.render_level(ctx, Comm()), lambda: distributed.render_tiled(ctx, Comm()),
                     lambda: distributed.render_adaptive(ctx, Comm())):
            with pytest.raises(ValueError, match="two or more cameras"):
                call()
        for bad in ((-1, 0), (2, 0), (0, 1), (0, -1)):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([level], camera=bad[0], variant=bad[1])
            assert err.value.code == BL_E_ARG
            with pytest.raises(bl.BlacklightError) as err:
                ctx.variant_output_path(0, bad[1], camera=bad[0])
            assert err.value.code == BL_E_ARG
        levels = [level, dict(image=image[:, :16], block_locs=np.zeros((1, 2), dtype=np.int32))]
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output(levels, camera=0)
        assert err.value.code == BL_E_ARG and "adaptive" in str(err.value)


# ---------------------------------------------------------------------------------------------------------------- names
def test_names_by_snapshot_camera_and_variant(bl, tmp_path):
    base = _case("sim_dp_interp", simulation_multiple="true", simulation_start=7, simulation_end=9, output_file=str(tmp_path / "out.d/img_{04d}.npz"))

    def context(*lines, case=None, **overrides):
        p = bl.Params.from_dict(dict(case or base, **overrides))
        for line in lines:
            p.set_line(line)
        return bl.Context(p, device=BL_DEVICE_NONE)

    three = "sweep_camera_th = 17,60,163"
    with context(three) as ctx:   # cameras alone: .cCC
        assert ctx.variant_output_path(2, 0, camera=1) == str(tmp_path / "out.d/img_0009.c01.npz")
    with context(three, "sweep_rat_low = 1,1,1", "sweep_rat_high = 10,40,160", "sweep_rho_cgs = 1e-16,2e-16,3e-16") as ctx:   # models x units
        assert ctx.variant_output_path(0, 0 * 3 + 2, camera=1) == str(tmp_path / "out.d/img_0007.c01m00u02.npz")
        names = [ctx.variant_output_path(1, v, camera=c) for c in range(3) for v in range(9)]
        assert names == sorted(names) and len(set(names)) == 27   # names sort in (camera, variant) order
    with context(three, "sweep_rho_cgs = 1e-16,2e-16,3e-16", "sweep_cut_sigma_max = 1,3,10,-1") as ctx:   # ... x cuts
        assert ctx.variant_output_path(0, 2 * 4 + 3, camera=1) == str(tmp_path / "out.d/img_0007.c01m00u02s03.npz")
    with context(three, "sweep_rho_cgs = 1e-16,2e-16,3e-16,4e-16", case=_case("sim_polarized", output_file="image.npz")) as ctx:   # polarized triples
        assert ctx.variant_output_path(0, 3, camera=1) == "image.c01v03.npz"
    with context("sweep_camera_th = 60", "sweep_rho_cgs = 1e-16,2e-16") as ctx:   # C = 1: no camera tag
        assert ctx.num_cameras == 1 and ctx.variant_output_path(0, 1, camera=0) == str(tmp_path / "out.d/img_0007.m00u01.npz")
        assert ctx.variant_output_path(0, 1) == ctx.variant_output_path(0, 1, camera=0)
    with context() as ctx:   # nothing set: the plain name
        assert ctx.variant_output_path(1, 0, camera=0) == str(tmp_path / "out.d/img_0008.npz")
    with context(three, output_file=str(tmp_path / "out.d/no_extension_{02d}")) as ctx:   # the '.' of a directory is not an extension
        assert ctx.variant_output_path(0, 0, camera=2) == str(tmp_path / "out.d/no_extension_07.c02")
        buf = C.create_string_buffer(8)
        assert ctx._lib.bl_camera_output_path(ctx._ctx, 0, 0, 0, buf, len(buf)) == BL_E_ARG   # a buffer too short for the name
    with context("sweep_camera_th = " + ",".join(str(10 * k + 5) for k in range(16))) as ctx:
        assert [os.path.basename(ctx.variant_output_path(0, 0, camera=c)) for c in (0, 9, 15)] == ["img_0007.c00.npz", "img_0007.c09.npz", "img_0007.c15.npz"]


# ---------------------------------------------------------------------------------------------------------------- the writer
def _rows(rng, n_rows, n_pix):
    image = rng.standard_normal((n_rows, n_pix)) * 10.0 ** rng.integers(-30, 5, size=(n_rows, 1))
    image[rng.random(image.shape) < 0.02] = np.nan
    return np.ascontiguousarray(image)


def _write_and_compare(bl, tmp_path, params, sweep_lines, cameras, variant_values, fmt, camera_key=None, rendering=False):
    """A context with several cameras (and variants) writes each (camera, variant) from synthetic rows; a plain context with that
    camera's angles (and that variant's values) in its block writes the slice."""
    params = dict(params, output_format=fmt, output_file=str(tmp_path / f"lib.{fmt}"))
    p = bl.Params.from_dict(params)
    p.set_line("sweep_camera_th = " + su.comma([th for th, _ in cameras]))
    p.set_line("sweep_camera_ph = " + su.comma([ph for _, ph in cameras]))
    for line in sweep_lines:
        p.set_line(line)
    rng = np.random.default_rng(20261019)
    names = {}
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        n_cameras, n_variants = ctx.num_cameras, ctx.num_variants
        assert n_cameras == len(cameras) and n_variants == len(variant_values)
        n_q = ctx.num_quantities // n_variants
        n_pix = ctx.resolution ** 2
        image = _rows(rng, n_variants * n_q, n_cameras * n_pix)
        level = dict(image=image, block_locs=None)
        if camera_key is not None:
            level[camera_key] = rng.standard_normal((n_cameras * n_pix, 4))
        if rendering:
            level["rendering"] = rng.random((ctx.num_render_images, 3, n_cameras * n_pix))
        for c in range(n_cameras):
            for v in range(n_variants):
                ctx.write_output([level], camera=c, variant=v)
                names[c, v] = ctx.variant_output_path(0, v, camera=c)
                assert os.path.exists(names[c, v]), names[c, v]
        slices = [ctx.camera_slice(c) for c in range(n_cameras)]
    ordered = [names[c, v] for c in range(len(cameras)) for v in range(len(variant_values))]
    assert ordered == sorted(ordered) and len(set(ordered)) == len(ordered)
    for c, (th, ph) in enumerate(cameras):
        for v, values in enumerate(variant_values):
            single = dict(params, camera_th=th, camera_ph=ph, output_file=str(tmp_path / f"single_{c}_{v}.{fmt}"), **values)
            part = dict(image=np.ascontiguousarray(image[v * n_q:(v + 1) * n_q, slices[c]]), block_locs=None)
            if camera_key is not None:
                part[camera_key] = np.ascontiguousarray(level[camera_key][slices[c]])
            if rendering:
                part["rendering"] = np.ascontiguousarray(level["rendering"][:, :, slices[c]])
            with bl.Context(bl.Params.from_dict(single), device=BL_DEVICE_NONE) as plain:
                assert plain.num_quantities == n_q
                plain.write_output([part])
            got, want = su.file_bytes(names[c, v]), su.file_bytes(single["output_file"])
            assert got == want, (fmt, c, v)
            if fmt == "raw":
                assert got == part["image"].tobytes()
    return names


@pytest.mark.parametrize("fmt", ["npz", "npy", "raw"])
def test_camera_files_equal_single_runs(bl, tmp_path, fmt):
    """Three cameras, two frequencies, an auxiliary row and the camera record (output_camera; written to npz only, as in a single run)."""
    params = _case("sim_multifreq", image_num_frequencies=2, image_tau="true", output_camera="true")
    names = _write_and_compare(bl, tmp_path, params, [], CAMERAS[:3], [{}], fmt, camera_key="camera_pos")
    assert [os.path.basename(names[c, 0]) for c in range(3)] == [f"lib.c{c:02d}.{fmt}" for c in range(3)]
    if fmt == "npz":
        assert np.load(names[1, 0])["positions"].shape == (16, 16, 4)


@pytest.mark.parametrize("fmt", ["npz", "npy", "raw"])
def test_camera_files_with_variants_equal_single_runs(bl, tmp_path, fmt):
    """Two cameras x (two models x two units): the camera's slice of the variant's rows."""
    params = _case("sim_multifreq", image_num_frequencies=2)
    lines = ["sweep_rat_low = 1,2", "sweep_rat_high = 10,160", "sweep_rho_cgs = 1e-16,3e-16"]
    values = [dict(plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=rho) for low, high in ((1.0, 10.0), (2.0, 160.0)) for rho in (1e-16, 3e-16)]
    names = _write_and_compare(bl, tmp_path, params, lines, CAMERAS[1:3], values, fmt)
    assert os.path.basename(names[1, 3]) == f"lib.c01m01u01.{fmt}"


def test_pinhole_directions_polarized_rows_and_renderings(bl, tmp_path):
    """A pinhole camera's record is "directions"; polarized rows are regrouped by Stokes parameter; renderings come by camera too."""
    pinhole = _case("sim_pinhole_camera_norm", output_camera="true")
    names = _write_and_compare(bl, tmp_path, pinhole, [], CAMERAS[1:3], [{}], "npz", camera_key="camera_dir")
    assert "directions" in np.load(names[0, 0]).files
    polarized = _case("sim_polarized", image_num_frequencies=2, image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log")
    values = [dict(plasma_rat_low=1.0, plasma_rat_high=10.0, simulation_rho_cgs=1e-16), dict(plasma_rat_low=1.0, plasma_rat_high=40.0, simulation_rho_cgs=2e-16)]
    sub = tmp_path / "pol"
    sub.mkdir()
    names = _write_and_compare(bl, sub, polarized, ["sweep_rat_low = 1,1", "sweep_rat_high = 10,40", "sweep_rho_cgs = 1e-16,2e-16"], CAMERAS[:2], values, "npz")
    assert os.path.basename(names[1, 1]) == "lib.c01v01.npz" and np.load(names[1, 1])["Q_nu"].shape == (2, 24, 24)
    render_case = next((c for c in gu.GPU_CASES if int(_case(c).get("render_num_images") or 0) > 0 and _case(c).get("model_type") == "simulation"), None)
    assert render_case is not None, "no golden case with renderings"
    sub = tmp_path / "render"
    sub.mkdir()
    names = _write_and_compare(bl, sub, _case(render_case), [], CAMERAS[1:3], [{}], "npz", rendering=True)
    assert np.load(names[1, 0])["rendering"].shape[-2:] == (int(_case(render_case)["camera_resolution"]),) * 2


def test_one_camera_is_the_variant_writer(bl, tmp_path):
    """C = 1 - no list, or a list of one: camera 0, the plain call's name and bytes."""
    params = _case("sim_multifreq", output_file=str(tmp_path / "one.npz"))
    rng = np.random.default_rng(7)
    for lines in ([], ["sweep_camera_th = 45", "sweep_camera_ph = 0"]):
        p = bl.Params.from_dict(params)
        for line in lines:
            p.set_line(line)
        with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
            level = dict(image=_rows(rng, ctx.num_quantities, ctx.resolution ** 2), block_locs=None)
            ctx.write_output([level])
            plain = su.file_bytes(params["output_file"])
            os.remove(params["output_file"])
            ctx.write_output([level], camera=0)
            assert su.file_bytes(params["output_file"]) == plain
            other = tmp_path / "elsewhere.npz"
            ctx.write_output([level], path=other, camera=0, variant=0)   # path_override wins
            assert su.file_bytes(other) == plain
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([level], camera=1)
            assert err.value.code == BL_E_ARG
