"""An explicit list of observing frequencies, on host-only contexts (no GPU): bl_set_frequencies (argument errors with the entry's
index, the two refusals, n = 0 restoring the block's list bit for bit, the row count of a block with image_num_frequencies = n),
the sweep_frequency key of the grammar (list forms, error texts, dropped by every older parser call, kept by the new ones), the
checked apply step (all or nothing), the file names with their fFF tag, and bl_write_output_frequency: byte for byte the file a
context with that one frequency in its block writes from the matching rows."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import frequency_util as fu
import golden_util as gu
import sweep_util as su

BL_DEVICE_NONE = -2
BL_E_INPUT, BL_E_UNSUPPORTED, BL_E_ARG = 1, 3, 5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L = fu.L   # unordered, with a duplicate
_labels = fu.labels


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return dict(params, **overrides)


def _spaced(params, n):
    """The block with image_num_frequencies = n: its one image_frequency, or n values between 8.6e10 and 3.45e11."""
    params = dict(params, image_num_frequencies=n)
    if n == 1:
        params.setdefault("image_frequency", 2.3e11)
        return params
    return dict(params, image_frequency_start=8.6e10, image_frequency_end=3.45e11, image_frequency_spacing="log")


def _bits(values):
    return np.asarray(values, dtype=np.float64).tobytes()


def _state(ctx):
    return ctx.num_frequencies, _bits(ctx.frequencies), ctx.num_quantities


# ---------------------------------------------------------------------------------------------------------------- exported symbols
def test_symbols_exported_and_declared(bl):
    lib = C.CDLL(bl.LIB_PATH)
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_set_frequencies", "bl_num_frequencies", "bl_write_output_frequency", "bl_frequency_output_path", "bl_params_set_line_sweep_all",
                 "bl_params_read_file_sweep_all", "bl_apply_sweep_all"):
        assert hasattr(lib, name), name
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_FREQUENCIES\s+1024\b", header)
    assert re.search(r"typedef\s+struct\s+bl_sweep_frequencies\s*\{\s*int32_t\s+n,\s*reserved;\s*double\s+hz\[BL_MAX_SWEEP\];\s*\}\s*bl_sweep_frequencies;", header)
    from blacklight_amd import _capi
    assert C.sizeof(_capi.SweepFrequencies) == 8 + 16 * 8 and C.sizeof(_capi.SweepAll) == 5 * C.sizeof(C.c_void_p)
    assert C.sizeof(_capi.SweepLists) == 4 * C.sizeof(C.c_void_p)   # the four-member struct stays as it is


# ---------------------------------------------------------------------------------------------------------------- the setter
def test_the_list_is_the_contexts_frequency_count(bl):
    with bl.Context(bl.Params.from_dict(_case("sim_dp_interp")), device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_frequencies == 0 and ctx.n_freq == 1 and ctx.num_quantities == 1
        for n in range(1, 6):
            ctx.set_frequencies(L[:n])
            assert ctx.num_frequencies == n == ctx.n_freq and _bits(ctx.frequencies) == _bits(L[:n]) and ctx.num_quantities == n
        ctx.set_frequencies(4.3e10)   # a scalar: a list of one
        assert ctx.num_frequencies == 1 and ctx.frequencies.tolist() == [4.3e10]
        ctx.set_electron_models([10.0, 40.0])   # rows stay variant-major: the list multiplies a variant's rows
        ctx.set_frequencies(L[:3])
        assert ctx.num_quantities == 2 * 3
    assert C.CDLL(bl.LIB_PATH).bl_num_frequencies(None) == -1


def test_argument_errors_name_the_entry_and_change_nothing(bl):
    with bl.Context(bl.Params.from_dict(_case("sim_aux_images")), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies(L[:3])
        held = _state(ctx)
        lib, handle = ctx._lib, ctx._ctx
        many = (C.c_double * 1025)(*([2.3e11] * 1025))
        for n, array in ((-1, many), (1025, many), (2, None)):
            assert lib.bl_set_frequencies(handle, n, array) == BL_E_ARG
            assert lib.bl_last_error(handle).decode() == "Error: bl_set_frequencies needs 0 <= n <= 1024 and the array of frequencies.\n"
            assert _state(ctx) == held
        for index, bad in ((0, 0.0), (1, -2.3e11), (2, math.nan), (3, math.inf), (4, -math.inf), (2, -0.0)):
            values = list(L)
            values[index] = bad
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_frequencies(values)
            assert err.value.code == BL_E_ARG and str(err.value) == f"Error: bl_set_frequencies: frequency {index} is not a finite value > 0."
            assert _state(ctx) == held
        assert lib.bl_set_frequencies(None, 0, None) == BL_E_ARG
        assert lib.bl_set_frequencies(handle, 1024, many) == 0 and ctx.num_frequencies == 1024   # the bound itself is taken
        assert lib.bl_set_frequencies(handle, 0, None) == 0 and ctx.num_frequencies == 0         # n = 0 needs no array


def test_adaptive_frequency_num_must_index_the_list(bl):
    message = "Error: Must choose adaptive_frequency_num from 1 to image_num_frequencies."
    two = _case("formula_adaptive_multifreq")   # two frequencies, adaptive_frequency_num = 2
    assert int(two["adaptive_frequency_num"]) == 2
    with bl.Context(bl.Params.from_dict(two), device=BL_DEVICE_NONE) as ctx:
        own = _state(ctx)
        for n in (2, 3, 5):
            ctx.set_frequencies(L[:n])   # 2 lies within 1 .. n
        ctx.set_frequencies(L[:1])       # n = 1: the index is 0 whatever the key says
        ctx.set_frequencies([])
        assert _state(ctx) == own
    for overrides, absent in ((dict(adaptive_frequency_num=3), False), (dict(adaptive_frequency_num=0), False), ({}, True)):
        one = dict(_spaced(two, 1), **overrides)
        if absent:
            one.pop("adaptive_frequency_num")
        with bl.Context(bl.Params.from_dict(one), device=BL_DEVICE_NONE) as ctx:
            held = _state(ctx)
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_frequencies(L[:2])
            assert err.value.code == BL_E_ARG and str(err.value) == message
            assert _state(ctx) == held
            ctx.set_frequencies(L[:1])   # one entry refines by its own image: accepted
            if overrides.get("adaptive_frequency_num") == 3:
                ctx.set_frequencies(L[:3])
                with pytest.raises(bl.BlacklightError):
                    ctx.set_frequencies(L[:2])
                assert ctx.num_frequencies == 3


def test_a_loaded_geodesic_checkpoint_refuses_the_list(bl):
    params = _case("sim_dp_interp", checkpoint_geodesic_load="true", checkpoint_geodesic_file="geo.bin")
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        held = _state(ctx)
        for n in (1, 3):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_frequencies(L[:n])
            assert err.value.code == BL_E_UNSUPPORTED
            assert str(err.value) == ("Error: Frequencies: a geodesic checkpoint carries its own frequency list, which replaces the context's "
                                      "(checkpoint_geodesic_load = true).")
            assert _state(ctx) == held
        ctx.set_frequencies([])   # n = 0 asks for nothing
        assert _state(ctx) == held
    saving = _case("sim_dp_interp", checkpoint_geodesic_save="true", checkpoint_geodesic_file="geo.bin")
    with bl.Context(bl.Params.from_dict(saving), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies(L)   # a checkpoint that is saved carries the list
        assert ctx.num_frequencies == 5


@pytest.mark.parametrize("case", ["sim_multifreq", "sim_true_color", "sim_dp_interp"])   # log, lin_wave, one frequency
def test_n_0_restores_the_blocks_list_bit_for_bit(bl, case):
    with bl.Context(bl.Params.from_dict(_case(case)), device=BL_DEVICE_NONE) as ctx:
        own = _state(ctx)
        assert own[0] == 0 and len(own[1]) == 8 * int(_case(case)["image_num_frequencies"])
        ctx.set_frequencies(L)
        assert _state(ctx) != own
        ctx.set_frequencies([])
        assert _state(ctx) == own
        ctx.set_frequencies([])   # twice: still the block's
        assert _state(ctx) == own


@pytest.mark.parametrize("case", ["sim_aux_images", "sim_polarized", "formula_flat"])
def test_row_count_is_that_of_a_block_with_n_frequencies(bl, case):
    params = _case(case)
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        for n in (1, 3, 5):
            ctx.set_frequencies(L[:n])
            with bl.Context(bl.Params.from_dict(_spaced(params, n)), device=BL_DEVICE_NONE) as block:
                assert ctx.num_quantities == block.num_quantities, (case, n)
    if case == "sim_aux_images":
        assert ctx.params.get("image_lambda_ave") and ctx.params.get("image_crossings")   # (the case with every kind of row)


# ---------------------------------------------------------------------------------------------------------------- grammar
def test_accepted_forms(bl):
    p = bl.Params.from_text("""
        sweep_frequency = 86e9, 230e9 ,3.45e11     # Hz
    """)
    assert p.has_sweep and p.sweep_frequency == [8.6e10, 2.3e11, 3.45e11]
    q = p.copy()
    p.set_line("sweep_frequency = 1e12")   # a later line replaces the list
    assert p.sweep_frequency == [1.0e12] and q.sweep_frequency == [8.6e10, 2.3e11, 3.45e11]
    sixteen = bl.Params.from_text("sweep_frequency = " + ",".join(f"{k + 1}e11" for k in range(16)))
    assert len(sixteen.sweep_frequency) == 16
    assert bl.Params.from_text("sweep_frequency = 2.3e11,2.3e11").sweep_frequency == [2.3e11, 2.3e11]   # duplicates are entries
    plain = bl.Params.from_text("camera_r = 50")
    assert not plain.has_sweep and plain.sweep_frequency == []


LINE_ERRORS = [
    ("sweep_frequency = 86e9,,230e9", "Error: Empty entry in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency = 86e9,", "Error: Empty entry in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency =", "Error: Empty entry in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency = 86e9,band7", "Error: Invalid number (band7) in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency = 230GHz", "Error: Invalid number (230GHz) in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency = 86e9;230e9", "Error: Invalid number (86e9;230e9) in list (sweep_frequency) in input file.\n"),
    ("sweep_frequency = 86e9,nan", "Error: Invalid frequency (nan) in list (sweep_frequency) in input file: must be finite and positive.\n"),
    ("sweep_frequency = inf", "Error: Invalid frequency (inf) in list (sweep_frequency) in input file: must be finite and positive.\n"),
    ("sweep_frequency = 86e9,0", "Error: Invalid frequency (0) in list (sweep_frequency) in input file: must be finite and positive.\n"),
    ("sweep_frequency = -230e9", "Error: Invalid frequency (-230e9) in list (sweep_frequency) in input file: must be finite and positive.\n"),
    ("sweep_frequency = " + ",".join(["230e9"] * 17), "Error: Too many entries in list (sweep_frequency) in input file: at most 16 for this build.\n"),
    ("sweep_frequencies = 1e11", "Error: Unknown key (sweep_frequencies) in input file.\n"),
]


@pytest.mark.parametrize("line,message", LINE_ERRORS)
def test_line_error_texts_through_every_parser_call(bl, line, message):
    """... the calls that keep the list and every one that drops it."""
    from blacklight_amd import _capi
    lib = _capi.lib()
    p = bl.Params()
    with pytest.raises(bl.BlacklightError) as err:
        p.set_line(line)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT

    def text_of(call, *args):
        text = C.create_string_buffer(1024)
        assert call(p.ptr, *args, line.encode(), text, len(text)) == BL_E_INPUT
        return text.value.decode()
    assert text_of(lib.bl_params_set_line) == message
    assert text_of(lib.bl_params_set_line_sweep, None) == message
    assert text_of(lib.bl_params_set_line_sweeps, None, None) == message
    assert text_of(lib.bl_params_set_line_sweeps_cameras, None, None, None) == message
    assert text_of(lib.bl_params_set_line_sweep_lists, None) == message
    assert text_of(lib.bl_params_set_line_sweep_all, None) == message


def test_older_parser_calls_drop_the_key_and_the_new_ones_keep_it(bl, tmp_path):
    """The block of a file with the key is, byte for byte, the block of the file without it - through every reader; the readers that
    know the earlier lists fill those as ever, bl_params_read_file_sweep_all fills the fifth struct."""
    from blacklight_amd import _capi
    lib = _capi.lib()
    size = lib.bl_params_sizeof()
    for case in ("sim_dp_interp", "sim_polarized", "formula_64"):
        params = _case(case)
        plain = su.write_input(tmp_path / f"{case}.input", params)
        keyed = su.write_input(tmp_path / f"{case}_f.input", dict(params, sweep_frequency="86e9,230e9,345e9", sweep_camera_th="17,60"))
        old, text, runs = bl.Params(), C.create_string_buffer(1024), C.c_int(0)
        assert lib.bl_params_read_file(old.ptr, plain.encode(), C.byref(runs), text, len(text)) == 0, text.value
        want = C.string_at(old.ptr, size)
        block = bl.Params()
        sweep, cuts, cameras, electrons, frequencies = _capi.Sweep(), _capi.SweepCuts(), _capi.SweepCameras(), _capi.SweepElectrons(), _capi.SweepFrequencies()
        assert lib.bl_params_read_file(block.ptr, keyed.encode(), None, text, len(text)) == 0, text.value
        assert C.string_at(block.ptr, size) == want
        assert lib.bl_params_read_file_sweep(block.ptr, C.byref(sweep), keyed.encode(), None, text, len(text)) == 0
        assert lib.bl_params_read_file_sweeps(block.ptr, C.byref(sweep), C.byref(cuts), keyed.encode(), None, text, len(text)) == 0
        assert lib.bl_params_read_file_sweeps_cameras(block.ptr, C.byref(sweep), C.byref(cuts), C.byref(cameras), keyed.encode(), None, text, len(text)) == 0
        assert C.string_at(block.ptr, size) == want and cameras.n_th == 2 and sweep.n_rat_low == 0 and cuts.n_sigma_max == 0
        four = _capi.SweepLists(C.pointer(sweep), C.pointer(cuts), C.pointer(cameras), C.pointer(electrons))
        assert lib.bl_params_read_file_sweep_lists(block.ptr, C.byref(four), keyed.encode(), None, text, len(text)) == 0
        assert C.string_at(block.ptr, size) == want and cameras.n_th == 2
        frequencies.n = 7   # (a reader clears the struct it fills)
        five = _capi.SweepAll(C.pointer(sweep), C.pointer(cuts), C.pointer(cameras), C.pointer(electrons), C.pointer(frequencies))
        for path, n in ((plain, 0), (keyed, 3)):
            assert lib.bl_params_read_file_sweep_all(block.ptr, C.byref(five), path.encode(), C.byref(runs), text, len(text)) == 0
            assert C.string_at(block.ptr, size) == want and frequencies.n == n
        assert list(frequencies.hz[:3]) == [8.6e10, 2.3e11, 3.45e11]
        only = _capi.SweepAll(None, None, None, None, C.pointer(frequencies))   # NULL members: validated and dropped
        assert lib.bl_params_read_file_sweep_all(block.ptr, C.byref(only), keyed.encode(), None, text, len(text)) == 0 and frequencies.n == 3
        assert lib.bl_params_read_file_sweep_all(block.ptr, None, keyed.encode(), None, text, len(text)) == 0
        with_key = bl.Params.from_file(keyed)
        assert C.string_at(with_key.ptr, size) == want and with_key.sweep_frequency == [8.6e10, 2.3e11, 3.45e11] and with_key.sweep_camera_th == [17.0, 60.0]
        assert not bl.Params.from_file(plain).has_sweep
        by_line = bl.Params.from_dict(params)
        before = C.string_at(by_line.ptr, size)
        by_line.set_line("sweep_frequency = 1e11,2e11")
        assert C.string_at(by_line.ptr, size) == before and by_line.has_sweep


# ---------------------------------------------------------------------------------------------------------------- the apply step
def _everything(ctx):
    return (_state(ctx), ctx.num_cameras, ctx.num_electron_models, ctx.num_density_units, ctx.num_sigma_cuts, ctx.num_polarized_variants, ctx.num_variants)


def test_the_key_ends_in_the_setter(bl, tmp_path):
    params = _case("sim_dp_interp")
    path = su.write_input(tmp_path / "f.input", dict(params, sweep_frequency=su.comma(L), sweep_rat_low="1,1", sweep_rat_high="10,40",
                                                     sweep_camera_th="17,60,163"))
    with bl.Context.from_input(path, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_frequencies == 5 and _bits(ctx.frequencies) == _bits(L)
        assert ctx.num_cameras == 3 and ctx.num_electron_models == 2 and ctx.num_quantities == 2 * 5
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies(L[:2])
        ctx.apply_sweep()   # an empty sweep makes no call
        other = bl.Params.from_text("sweep_rho_cgs = 1e-16,2e-16")
        ctx.apply_sweep(other)   # a list the call does not carry leaves its axis as it is
        assert ctx.num_frequencies == 2 and ctx.num_density_units == 2
        assert ctx._lib.bl_apply_sweep_all(ctx._ctx, None) == BL_E_ARG and ctx._lib.bl_apply_sweep_all(None, C.byref(other.sweep_all)) == BL_E_ARG
        assert ctx._lib.bl_apply_sweep_lists(ctx._ctx, C.byref(other.sweep_lists)) == 0   # the older call forwards, with no frequency list


def test_all_or_nothing(bl):
    from blacklight_amd import _capi
    params = _case("sim_dp_interp")
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies(L[:2])
        ctx.set_sigma_cuts([1.0, 3.0])
        held = _everything(ctx)
        # a bad frequency list beside good other lists (the parser refuses such an entry: the struct is filled by hand)
        good = bl.Params.from_text("sweep_rat_low = 1,1\nsweep_rat_high = 10,40\nsweep_camera_th = 17,60")
        for bad_value, n in ((math.nan, 3), (0.0, 3), (2.3e11, 17), (2.3e11, -1)):
            frequencies = _capi.SweepFrequencies()
            frequencies.n = n
            for k in range(16):
                frequencies.hz[k] = 2.3e11
            frequencies.hz[1] = bad_value
            lists = good.sweep_all
            lists.frequencies = C.pointer(frequencies)
            rc = ctx._lib.bl_apply_sweep_all(ctx._ctx, C.byref(lists))
            text = ctx._lib.bl_last_error(ctx._ctx).decode()
            if 0 < n <= 16:
                assert rc == BL_E_ARG and text == "Error: bl_set_frequencies: frequency 1 is not a finite value > 0.\n"
            else:
                assert rc == BL_E_INPUT and text == "Error: Too many entries in a sweep list: at most 16 for this build.\n"
            assert _everything(ctx) == held
        # a good frequency list beside a refused other list: kappa electrons need a polarized block
        refused = bl.Params.from_text("sweep_frequency = 86e9,230e9,345e9\nsweep_kappa_frac = 0.2,0.3")
        with pytest.raises(bl.BlacklightError) as err:
            ctx.apply_sweep(refused)
        assert err.value.code == BL_E_INPUT and "needs image_polarization = true" in str(err.value)
        assert _everything(ctx) == held
    with bl.Context(bl.Params.from_dict(_case("formula_64")), device=BL_DEVICE_NONE) as ctx:   # formula mode has no electron models
        held = _everything(ctx)
        with pytest.raises(bl.BlacklightError) as err:
            ctx.apply_sweep(bl.Params.from_text("sweep_frequency = 86e9,230e9\nsweep_rat_low = 1,1\nsweep_rat_high = 10,40"))
        assert err.value.code == BL_E_UNSUPPORTED and "formula" in str(err.value) and _everything(ctx) == held
        ctx.apply_sweep(bl.Params.from_text("sweep_frequency = 86e9,230e9"))   # formula mode takes the frequencies
        assert ctx.num_frequencies == 2


def test_a_sweep_of_several_frequencies_is_refused_on_an_adaptive_block(bl):
    message = "Error: Frequencies: adaptive refinement reads one image; a sweep of n >= 2 frequencies needs adaptive_max_level = 0."
    for case in ("sim_adaptive", "formula_adaptive_multifreq"):
        with bl.Context(bl.Params.from_dict(_case(case)), device=BL_DEVICE_NONE) as ctx:
            held = _everything(ctx)
            with pytest.raises(bl.BlacklightError) as err:
                ctx.apply_sweep(bl.Params.from_text("sweep_frequency = 86e9,230e9"))
            assert err.value.code == BL_E_UNSUPPORTED and str(err.value) == message
            assert _everything(ctx) == held
            ctx.apply_sweep(bl.Params.from_text("sweep_frequency = 86e9"))   # one entry: accepted
            assert ctx.num_frequencies == 1
        p = bl.Params.from_dict(_case(case))
        p.set_line("sweep_frequency = 86e9,230e9")
        with pytest.raises(bl.BlacklightError) as err:   # ... and when a context is made of such a file
            bl.Context(p, device=BL_DEVICE_NONE)
        assert err.value.code == BL_E_UNSUPPORTED and str(err.value) == message


# ---------------------------------------------------------------------------------------------------------------- names
def test_names_by_snapshot_frequency_camera_and_variant(bl, tmp_path):
    base = _case("sim_dp_interp", simulation_multiple="true", simulation_start=7, simulation_end=9, output_file=str(tmp_path / "out.d/img_{04d}.npz"))

    def context(*lines, case=None, **overrides):
        p = bl.Params.from_dict(dict(case or base, **overrides))
        for line in lines:
            p.set_line(line)
        return bl.Context(p, device=BL_DEVICE_NONE)

    three = "sweep_frequency = 86e9,230e9,345e9"
    with context(three, output_file="image.npz", simulation_multiple="false") as ctx:   # frequencies alone
        assert ctx.variant_output_path(frequency=2) == "image.f02.npz"
        assert ctx.variant_output_path() == "image.npz"   # the tag only where the frequency file is asked for
    with context(three, "sweep_camera_th = 17,60", "sweep_rat_low = 1,1", "sweep_rat_high = 10,40", "sweep_rho_cgs = 1e-16,2e-16") as ctx:
        assert ctx.variant_output_path(2, 0 * 2 + 1, camera=1, frequency=2) == str(tmp_path / "out.d/img_0009.c01f02m00u01.npz")
        assert ctx.variant_output_path(2, 1, camera=1) == str(tmp_path / "out.d/img_0009.c01m00u01.npz")   # the existing names stay
        names = [ctx.variant_output_path(0, v, camera=c, frequency=f) for c in range(2) for f in range(3) for v in range(4)]
        assert names == sorted(names) and len(set(names)) == 24   # names sort in (camera, frequency, variant) order
    with context(three, "sweep_cut_sigma_max = 1,3", "sweep_rho_cgs = 1e-16,2e-16") as ctx:
        assert ctx.variant_output_path(0, 3, frequency=0) == str(tmp_path / "out.d/img_0007.f00m00u01s01.npz")
    with context(three, "sweep_rho_cgs = 1e-16,2e-16,3e-16,4e-16", case=_case("sim_polarized", output_file="image.npz")) as ctx:   # polarized triples
        assert ctx.variant_output_path(0, 3, frequency=0) == "image.f00v03.npz"
        assert ctx.variant_output_path(0, 3) == "image.v03.npz"
    with context("sweep_frequency = 230e9") as ctx:   # a list of one: the sweep decides the names, not its length
        assert ctx.variant_output_path(1, frequency=0) == str(tmp_path / "out.d/img_0008.f00.npz")
        assert ctx.variant_output_path(1) == str(tmp_path / "out.d/img_0008.npz")
    with context(case=_case("sim_multifreq", output_file="image.npz")) as ctx:   # no list: an index into the block's own spaced list
        assert ctx.variant_output_path(frequency=1) == "image.f01.npz"
        for bad in (dict(frequency=3), dict(frequency=-1), dict(frequency=0, camera=1), dict(frequency=0, variant=1)):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.variant_output_path(**bad)
            assert err.value.code == BL_E_ARG
        buf = C.create_string_buffer(8)
        assert ctx._lib.bl_frequency_output_path(ctx._ctx, 0, 0, 0, 0, buf, len(buf)) == BL_E_ARG   # a buffer too short for the name
    with context(three, output_file=str(tmp_path / "out.d/no_extension_{02d}")) as ctx:   # the '.' of a directory is not an extension
        assert ctx.variant_output_path(0, frequency=1) == str(tmp_path / "out.d/no_extension_07.f01")


# ---------------------------------------------------------------------------------------------------------------- the writer
def _distinct_rows(n_rows, n_pix):
    """A distinct value in every row (and pixel), with a few NaNs."""
    image = (np.arange(n_rows, dtype=np.float64)[:, None] + 1.0) * 1.0e3 + np.arange(n_pix, dtype=np.float64)[None, :] / 7.0
    image[::3, 5::17] = np.nan
    return np.ascontiguousarray(image)


WRITER_CASES = [("sim_aux_images", {}), ("sim_polarized", dict(image_tau="true")), ("formula_flat", {})]


@pytest.mark.parametrize("fmt", ["npz", "npy"])
@pytest.mark.parametrize("case,overrides", WRITER_CASES)
def test_frequency_files_equal_a_one_frequency_contexts(bl, tmp_path, case, overrides, fmt):
    params = _case(case, output_format=fmt, output_file=str(tmp_path / f"lib.{fmt}"), **overrides)
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies(L)
        labels = _labels(params, 5)
        assert ctx.num_quantities == len(labels)
        n_pix = ctx.resolution ** 2
        image = _distinct_rows(len(labels), n_pix)
        level = dict(image=image, block_locs=None)
        for l in range(5):
            ctx.write_output([level], frequency=l)
            assert os.path.exists(ctx.variant_output_path(frequency=l))
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output([level], frequency=5)
        assert err.value.code == BL_E_ARG and "frequency 5 outside 0 .. 4" in str(err.value)
        levels = [level, dict(image=image[:, :16], block_locs=np.zeros((1, 2), dtype=np.int32))]
        with pytest.raises(bl.BlacklightError) as err:   # a one-frequency run refines by its own image
            ctx.write_output(levels, frequency=0)
        assert err.value.code == BL_E_ARG and "adaptive" in str(err.value)
    for l in range(5):
        single = _spaced(dict(params, output_file=str(tmp_path / f"single_{l}.{fmt}")), 1)
        single["image_frequency"] = repr(L[l])
        one = _labels(single, 1)
        picked = [labels.index((name, None if f is None else l, k)) for name, f, k in one]
        with bl.Context(bl.Params.from_dict(single), device=BL_DEVICE_NONE) as plain:
            assert plain.num_quantities == len(picked) and plain.frequencies.tolist() == [L[l]]
            plain.write_output([dict(image=np.ascontiguousarray(image[picked]), block_locs=None)])
        assert su.file_bytes(str(tmp_path / f"lib.f{l:02d}.{fmt}")) == su.file_bytes(single["output_file"]), (case, fmt, l)
    if fmt == "npz":
        third = np.load(str(tmp_path / "lib.f03.npz"))
        assert third["frequency"].tolist() == [L[3]] and third["I_nu"].shape == (ctx.resolution, ctx.resolution)


def test_frequency_files_by_camera_and_variant(bl, tmp_path):
    """Two cameras x two models x three frequencies: the camera's slice of the variant's rows of that frequency."""
    params = _case("sim_dp_interp", image_tau="true", output_file=str(tmp_path / "lib.npz"))
    cameras, pairs = [(17.0, 0.0), (60.0, 30.0)], [(1.0, 10.0), (2.0, 160.0)]
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_cameras([th for th, _ in cameras], [ph for _, ph in cameras])
        ctx.set_electron_models([high for _, high in pairs], [low for low, _ in pairs])
        ctx.set_frequencies(L[:3])
        labels = _labels(params, 3)
        n_q, n_pix = len(labels), ctx.resolution ** 2
        assert ctx.num_quantities == 2 * n_q
        image = _distinct_rows(2 * n_q, 2 * n_pix)
        for c in range(2):
            for l in range(3):
                for v in range(2):
                    ctx.write_output([dict(image=image, block_locs=None)], camera=c, variant=v, frequency=l)
    for c, (th, ph) in enumerate(cameras):
        for l in range(3):
            for v, (low, high) in enumerate(pairs):
                single = dict(params, camera_th=th, camera_ph=ph, plasma_rat_low=low, plasma_rat_high=high, image_frequency=repr(L[l]),
                              output_file=str(tmp_path / f"single_{c}_{l}_{v}.npz"))
                picked = [v * n_q + labels.index((name, None if f is None else l, k)) for name, f, k in _labels(single, 1)]
                with bl.Context(bl.Params.from_dict(single), device=BL_DEVICE_NONE) as plain:
                    plain.write_output([dict(image=np.ascontiguousarray(image[picked, c * n_pix:(c + 1) * n_pix]), block_locs=None)])
                assert su.file_bytes(str(tmp_path / f"lib.c{c:02d}f{l:02d}m{v:02d}u00.npz")) == su.file_bytes(single["output_file"]), (c, l, v)


def test_a_carried_list_writes_the_spaced_blocks_file(bl, tmp_path):
    """bl_write_output with a list set: one file with the reference's frequency axis - that of the spaced block whose list it carries."""
    for case, fmt in (("sim_multifreq", "npz"), ("sim_true_color", "npz"), ("sim_multifreq", "npy")):
        spaced = _case(case, image_tau="true", output_format=fmt, output_file=str(tmp_path / f"spaced.{fmt}"))
        with bl.Context(bl.Params.from_dict(spaced), device=BL_DEVICE_NONE) as block:
            values = block.frequencies
            image = _distinct_rows(block.num_quantities, block.resolution ** 2)
            block.write_output([dict(image=image, block_locs=None)])
            block.write_output([dict(image=image, block_locs=None)], frequency=1)   # (n = 0: an index into the block's own list)
        one = {k: v for k, v in spaced.items() if k not in ("image_frequency_start", "image_frequency_end", "image_frequency_spacing")}
        one = dict(one, image_num_frequencies=1, image_frequency=2.3e11, output_file=str(tmp_path / f"carried.{fmt}"))
        with bl.Context(bl.Params.from_dict(one), device=BL_DEVICE_NONE) as ctx:
            ctx.set_frequencies(values)
            assert ctx.num_quantities == image.shape[0]
            ctx.write_output([dict(image=image, block_locs=None)])
            ctx.write_output([dict(image=image, block_locs=None)], frequency=1)
        assert su.file_bytes(one["output_file"]) == su.file_bytes(spaced["output_file"]), (case, fmt)
        assert su.file_bytes(str(tmp_path / f"carried.f01.{fmt}")) == su.file_bytes(str(tmp_path / f"spaced.f01.{fmt}"))


def test_one_frequency_and_adaptive_levels(bl, tmp_path):
    """A list of one entry writes the f00 file with the bytes of the plain call - adaptive levels included."""
    params = _case("sim_adaptive", output_camera="false", output_file=str(tmp_path / "one.npz"))
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_frequencies([3.45e11])
        bs = int(params["adaptive_block_size"])
        level0 = dict(image=_distinct_rows(ctx.num_quantities, ctx.resolution ** 2), block_locs=None)
        level1 = dict(image=_distinct_rows(ctx.num_quantities, 2 * bs * bs), block_locs=np.array([[0, 0], [1, 1]], dtype=np.int32))
        ctx.write_output([level0, level1])
        ctx.write_output([level0, level1], frequency=0)
    assert su.file_bytes(str(tmp_path / "one.f00.npz")) == su.file_bytes(params["output_file"])
    assert np.load(params["output_file"])["frequency"].tolist() == [3.45e11]
