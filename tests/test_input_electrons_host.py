"""The seven electron lists of a .input file (sweep_power_frac ... sweep_w) on the host (no GPU): parsed and kept by the
bl_sweep_lists calls, validated and dropped by every earlier parser call, both list errors at the end of bl_params_read_file*, in
bl_sweep_electrons_resolve and in bl_apply_sweep_lists, one-entry lists, N from the electron lists alone, an unpolarized block, and
that a file without the keys parses as it always did."""
import ctypes as C
import os
import re

import pytest

import golden_util as gu
import sweep_util as su

BL_DEVICE_NONE = -2
BL_E_INPUT = 1
BL_E_ARG = 5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")
LISTS = dict(sweep_power_frac="0,0.3,0.2", sweep_p="2.5,2.5,3", sweep_gamma_min="2", sweep_gamma_max="1000,1000,500", sweep_kappa_frac="0.4,0,0.25",
             sweep_kappa="4,4,4.3", sweep_w="1.5")
WANT = dict(power_frac=[0.0, 0.3, 0.2], p=[2.5, 2.5, 3.0], gamma_min=[2.0], gamma_max=[1000.0, 1000.0, 500.0], kappa_frac=[0.4, 0.0, 0.25],
            kappa=[4.0, 4.0, 4.3], w=[1.5])
MIXES = [dict(power_frac=0.0, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.4, kappa=4.0, w=1.5),
         dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0, kappa=4.0, w=1.5),
         dict(power_frac=0.2, p=3.0, gamma_min=2.0, gamma_max=500.0, kappa_frac=0.25, kappa=4.3, w=1.5)]


def _lib():
    from blacklight_amd import _capi
    return _capi.lib()


def _params(case="sim_polarized_kappa", **overrides):
    fx, params, mock_args = gu.load_case(case)
    return dict(params, **overrides)


def _error(call, *args):
    err = C.create_string_buffer(1024)
    rc = call(*args, err, len(err))
    return rc, err.value.decode()


def _read_file(name, path):
    """One of the nine bl_params_read_file* calls on `path`: (rc, error text, what it kept of the electron lists - None: it keeps none)"""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    L, p, runs = _lib(), bl.Params(), C.c_int(0)
    sweep, cuts, cameras, electrons = _capi.Sweep(), _capi.SweepCuts(), _capi.SweepCameras(), _capi.SweepElectrons()
    path = str(path).encode()
    if name == "bl_params_read_file":
        rc, text = _error(L.bl_params_read_file, p._buf, path, C.byref(runs))
    elif name == "bl_params_read_file_sweep":
        rc, text = _error(L.bl_params_read_file_sweep, p._buf, C.byref(sweep), path, C.byref(runs))
    elif name == "bl_params_read_file_sweeps":
        rc, text = _error(L.bl_params_read_file_sweeps, p._buf, C.byref(sweep), C.byref(cuts), path, C.byref(runs))
    elif name == "bl_params_read_file_sweeps_cameras":
        rc, text = _error(L.bl_params_read_file_sweeps_cameras, p._buf, C.byref(sweep), C.byref(cuts), C.byref(cameras), path, C.byref(runs))
    elif name == "lists without electrons":
        lists = _capi.SweepLists(C.pointer(sweep), C.pointer(cuts), C.pointer(cameras), None)
        rc, text = _error(L.bl_params_read_file_sweep_lists, p._buf, C.byref(lists), path, C.byref(runs))
    elif name == "null lists":
        rc, text = _error(L.bl_params_read_file_sweep_lists, p._buf, None, path, C.byref(runs))
    else:
        lists = _capi.SweepLists(C.pointer(sweep), C.pointer(cuts), C.pointer(cameras), C.pointer(electrons))
        rc, text = _error(L.bl_params_read_file_sweep_lists, p._buf, C.byref(lists), path, C.byref(runs))
        return rc, text, {key: [float(x) for x in getattr(electrons, key)[:getattr(electrons, "n_" + key)]] for key in NAMES}
    return rc, text, None


READERS = ["bl_params_read_file", "bl_params_read_file_sweep", "bl_params_read_file_sweeps", "bl_params_read_file_sweeps_cameras", "lists without electrons",
           "null lists", "bl_params_read_file_sweep_lists"]


def _set_line(name, p, line):
    from blacklight_amd import _capi
    L = _lib()
    sweep, cuts, cameras = _capi.Sweep(), _capi.SweepCuts(), _capi.SweepCameras()
    line = line.encode()
    if name == "bl_params_set_line":
        return _error(L.bl_params_set_line, p._buf, line)
    if name == "bl_params_set_line_sweep":
        return _error(L.bl_params_set_line_sweep, p._buf, C.byref(sweep), line)
    if name == "bl_params_set_line_sweeps":
        return _error(L.bl_params_set_line_sweeps, p._buf, C.byref(sweep), C.byref(cuts), line)
    if name == "bl_params_set_line_sweeps_cameras":
        return _error(L.bl_params_set_line_sweeps_cameras, p._buf, C.byref(sweep), C.byref(cuts), C.byref(cameras), line)
    return _error(L.bl_params_set_line_sweep_lists, p._buf, None, line)


SETTERS = ["bl_params_set_line", "bl_params_set_line_sweep", "bl_params_set_line_sweeps", "bl_params_set_line_sweeps_cameras", "null lists"]


def test_symbols_exported_and_declared(built_library):
    from blacklight_amd import _capi
    import blacklight_amd as bl
    lib = C.CDLL(bl.LIB_PATH)
    for name in ("bl_params_set_line_sweep_lists", "bl_params_read_file_sweep_lists", "bl_sweep_electrons_resolve", "bl_apply_sweep_lists"):
        assert hasattr(lib, name), name
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+bl_sweep_lists\s*\{\s*bl_sweep\s*\*sweep;\s*bl_sweep_cuts\s*\*cuts;\s*bl_sweep_cameras\s*\*cameras;\s*"
                     r"bl_sweep_electrons\s*\*electrons;\s*\}\s*bl_sweep_lists;", header)
    assert "_sweeps_cameras_electrons" not in header   # one extensible set of calls, not a fourth generation
    # the three earlier structs are ABI and keep their sizes
    assert (C.sizeof(_capi.Sweep), C.sizeof(_capi.SweepCuts), C.sizeof(_capi.SweepCameras)) == (16 + 3 * 16 * 8, 8 + 16 * 8, 8 + 2 * 16 * 8)
    assert C.sizeof(_capi.SweepElectrons) == 32 + 7 * 16 * 8 and C.sizeof(_capi.SweepLists) == 4 * C.sizeof(C.c_void_p)


def test_the_seven_keys_are_parsed_and_kept(built_library, tmp_path):
    import blacklight_amd as bl
    p = bl.Params.from_dict(_params(**LISTS))
    assert p.sweep_electrons == WANT and p.has_sweep and p.has_sweep_electrons
    assert p.copy().sweep_electrons == WANT
    for key in LISTS:   # never in the parameter block
        with pytest.raises(KeyError):
            p.get(key)
    path = su.write_input(tmp_path / "lists.input", _params(**LISTS))
    rc, text, kept = _read_file("bl_params_read_file_sweep_lists", path)
    assert (rc, text, kept) == (0, "", WANT)
    q = bl.Params.from_file(path)
    assert q.sweep_electrons == WANT
    assert q.resolved_electrons() == ([1.0] * 3, [10.0] * 3, [1.0e-16] * 3, MIXES)   # the block's pair and unit at every mix


@pytest.mark.parametrize("name", READERS[:6])
def test_every_earlier_reader_validates_and_drops_them(name, built_library, tmp_path):
    import blacklight_amd as bl
    with_keys = su.write_input(tmp_path / "with.input", _params(**LISTS))
    without = su.write_input(tmp_path / "without.input", _params())
    assert _read_file(name, with_keys) == (0, "", None)
    plain, kept = bl.Params(), bl.Params()
    runs = C.c_int(0)
    assert _error(_lib().bl_params_read_file, plain._buf, without.encode(), C.byref(runs))[0] == 0
    assert _error(_lib().bl_params_read_file, kept._buf, with_keys.encode(), C.byref(runs))[0] == 0
    assert plain._buf.raw == kept._buf.raw   # the keys leave no trace in the block
    # ... validated all the same: per entry when the line is read, against each other at the end of the file
    bad = su.write_input(tmp_path / "bad.input", _params(**dict(LISTS, sweep_w="1.5,inf")))
    assert _read_file(name, bad) == (BL_E_INPUT, "Error: Invalid value (inf) in list (sweep_w) in input file: must be finite.\n", None)
    bad = su.write_input(tmp_path / "bad.input", _params(**dict(LISTS, sweep_kappa="4,4.3")))
    assert _read_file(name, bad) == (BL_E_INPUT, "Error: sweep_kappa must have one entry or as many as the other sweep lists (2 and 3) in input file.\n", None)
    bad = su.write_input(tmp_path / "bad.input", _params(image_polarization="false", sweep_p="2.5"))
    assert _read_file(name, bad) == (BL_E_INPUT, "Error: sweep_p needs image_polarization = true in input file.\n", None)


@pytest.mark.parametrize("name", SETTERS)
def test_every_earlier_line_setter_validates_and_drops_them(name, built_library):
    import blacklight_amd as bl
    p = bl.Params.from_dict(_params())
    before = p._buf.raw
    for key, value in LISTS.items():
        assert _set_line(name, p, f"{key} = {value}") == (0, "")
    assert p._buf.raw == before and not p.has_sweep
    entries = [("sweep_kappa = 4,,5", "Error: Empty entry in list (sweep_kappa) in input file.\n"),
               ("sweep_p = 2.5x", "Error: Invalid number (2.5x) in list (sweep_p) in input file.\n"),
               ("sweep_gamma_min = nan", "Error: Invalid value (nan) in list (sweep_gamma_min) in input file: must be finite.\n"),
               ("sweep_power_frac = -inf,0", "Error: Invalid value (-inf) in list (sweep_power_frac) in input file: must be finite.\n"),
               ("sweep_w = " + ",".join(["1"] * 17), "Error: Too many entries in list (sweep_w) in input file: at most 16 for this build.\n"),
               ("sweep_kapa = 4", "Error: Unknown key (sweep_kapa) in input file.\n")]
    for line, message in entries:
        assert _set_line(name, p, line) == (BL_E_INPUT, message)


CASES = [
    (dict(sweep_kappa="4,4.3", sweep_w="1.5,1,2"), "Error: sweep_kappa must have one entry or as many as the other sweep lists (2 and 3) in input file.\n"),
    (dict(sweep_rat_low="1,1", sweep_rat_high="10,40", sweep_kappa_frac="0.4,0,0.1"),
     "Error: sweep_kappa_frac must have one entry or as many as the other sweep lists (3 and 2) in input file.\n"),
    (dict(sweep_rho_cgs="1e-16,2e-16,3e-16,4e-16", sweep_power_frac="0.1", sweep_gamma_max="10,20"),
     "Error: sweep_gamma_max must have one entry or as many as the other sweep lists (2 and 4) in input file.\n"),
    (dict(image_polarization="false", sweep_w="1.5,2"), "Error: sweep_w needs image_polarization = true in input file.\n"),
    (dict(image_polarization="false", sweep_rat_low="1,1", sweep_rat_high="10,40", sweep_power_frac="0.1"),
     "Error: sweep_power_frac needs image_polarization = true in input file.\n"),
]


@pytest.mark.parametrize("keys, message", CASES)
def test_both_list_errors_at_all_three_places(keys, message, built_library, tmp_path):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    params = _params(**keys)
    # at the end of bl_params_read_file* (every one of them)
    path = su.write_input(tmp_path / "bad.input", params)
    for name in READERS:
        rc, text, kept = _read_file(name, path)
        assert (rc, text) == (BL_E_INPUT, message), name
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_file(path)
    assert err.value.code == BL_E_INPUT and str(err.value) == message.rstrip("\n")
    # in the resolve call: the lines alone are fine, the lists against each other are not
    p = bl.Params.from_dict(params)
    with pytest.raises(bl.BlacklightError) as err:
        p.resolved_electrons()
    assert err.value.code == BL_E_INPUT and str(err.value) == message.rstrip("\n")
    # in the apply call, which leaves the context as it was
    block = bl.Params.from_dict(_params(**{k: v for k, v in keys.items() if not k.startswith("sweep_")}))
    ctx = bl.Context(block, device=BL_DEVICE_NONE)
    assert ctx._lib.bl_apply_sweep_lists(ctx._ctx, C.byref(p.sweep_lists)) == BL_E_INPUT
    assert ctx._lib.bl_last_error(ctx._ctx).decode() == message
    assert ctx.num_variants == 1 and ctx.num_polarized_variants == 0 and ctx.num_cameras == 0
    ctx.close()
    with pytest.raises(bl.BlacklightError):
        bl.Context(p, device=BL_DEVICE_NONE)
    assert _lib().bl_apply_sweep_lists(None, C.byref(p.sweep_lists)) == BL_E_ARG


def test_one_entry_lists_are_every_variants_value(built_library):
    import blacklight_amd as bl
    p = bl.Params.from_dict(_params(sweep_rat_low="1,1,2", sweep_rat_high="10,40,160", sweep_rho_cgs="3e-16", sweep_kappa_frac="0.25", sweep_kappa="4.3,4,3.5",
                                    sweep_power_frac="0.2", sweep_p="3", sweep_gamma_min="3", sweep_gamma_max="500"))
    low, high, rho, mixes = p.resolved_electrons()
    assert (low, high, rho) == ([1.0, 1.0, 2.0], [10.0, 40.0, 160.0], [3.0e-16] * 3)
    assert mixes == [dict(power_frac=0.2, p=3.0, gamma_min=3.0, gamma_max=500.0, kappa_frac=0.25, kappa=kappa, w=1.5) for kappa in (4.3, 4.0, 3.5)]   # (w: the block's)
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_polarized_variants == 3 and ctx.polarized_variants == [(10.0, 1.0, 3.0e-16), (40.0, 1.0, 3.0e-16), (160.0, 2.0, 3.0e-16)]
        assert ctx.polarized_electrons == mixes and ctx.polarized_electrons_set and ctx.polarized_cuts is None
        assert ctx.variant_output_path(0, 2).endswith(".v02.npz")
        assert ctx._lib.bl_warnings(ctx._ctx).decode().count("Polarized transport will interpolate formulas based on kappa.") == 1


def test_the_number_of_tuples_from_the_electron_lists_alone(built_library):
    import blacklight_amd as bl
    p = bl.Params.from_dict(_params(sweep_w="1.5,2.5", sweep_kappa="4"))
    low, high, rho, mixes = p.resolved_electrons()
    assert (low, high, rho) == ([1.0, 1.0], [10.0, 10.0], [1.0e-16, 1.0e-16]) and [m["w"] for m in mixes] == [1.5, 2.5]
    assert [m["kappa_frac"] for m in mixes] == [0.4, 0.4]
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_polarized_variants == 2 and ctx.polarized_electrons == mixes
    # a single entry is a single variant: that tuple instead of the parameter block's
    one = bl.Params.from_dict(_params(sweep_kappa_frac="0"))
    assert one.resolved_electrons()[3] == [dict(power_frac=0.0, p=0.0, gamma_min=0.0, gamma_max=0.0, kappa_frac=0.0, kappa=4.0, w=1.5)]
    with bl.Context(one, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_polarized_variants == 1 and ctx.num_variants == 1 and ctx.polarized_electrons[0]["kappa_frac"] == 0.0
    # what the setter checks it checks, in its words: the context is not made
    with pytest.raises(bl.BlacklightError) as err:
        bl.Context(bl.Params.from_dict(_params(sweep_kappa="4,5.5")), device=BL_DEVICE_NONE)
    assert "variant 1: Polarized transport only supports kappa in [3.5, 5]." in str(err.value)


def test_an_unpolarized_block_keeps_its_sweeps_and_refuses_the_electron_keys(built_library):
    import blacklight_amd as bl
    keys = dict(sweep_rat_low="1,1", sweep_rat_high="10,40", sweep_rho_cgs="1e-16,2e-16")
    p = bl.Params.from_dict(_params("sim_dp_interp", **keys))
    assert p.resolved_electrons() == ([], [], [], [])   # no polarized variants: models x units, as ever
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_variants == 4 and ctx.num_polarized_variants == 0
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_dict(_params("sim_dp_interp", sweep_kappa="4", **keys)).resolved_electrons()
    assert str(err.value) == "Error: sweep_kappa needs image_polarization = true in input file."


def test_a_file_without_the_keys_is_what_it_was(built_library, tmp_path):
    import blacklight_amd as bl
    for case, keys in (("sim_polarized_kappa", {}), ("sim_polarized", dict(sweep_rat_low="1,1", sweep_rat_high="10,40")),
                       ("sim_dp_interp", dict(sweep_rho_cgs="1e-16,2e-16", sweep_cut_sigma_max="1,-1"))):
        path = su.write_input(tmp_path / f"{case}.input", _params(case, **keys))
        rc, text, kept = _read_file("bl_params_read_file_sweep_lists", path)
        assert (rc, text) == (0, "") and kept == {key: [] for key in NAMES}
        new = bl.Params.from_file(path)
        old, runs = bl.Params(), C.c_int(0)
        assert _error(_lib().bl_params_read_file, old._buf, path.encode(), C.byref(runs))[0] == 0
        assert new._buf.raw == old._buf.raw and new.num_runs == runs.value and not new.has_sweep_electrons
        assert new.has_sweep == bool(keys)
        with bl.Context(new, device=BL_DEVICE_NONE) as ctx:   # applied as before: through bl_apply_sweeps_cameras
            assert not ctx.polarized_electrons_set
            assert ctx.num_variants == (1 if not keys else (2 if case == "sim_polarized" else 4))
