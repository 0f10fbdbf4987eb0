"""Sweeps written in the .input file, on host-only contexts (no GPU): the sweep_rat_low / sweep_rat_high / sweep_rho_cgs keys of the
grammar (accepted forms, every error text, parameter blocks of sweep-free inputs untouched), bl_apply_sweep, and
bl_write_output_variant / bl_variant_output_path: one reference-layout file per variant of a render, byte for byte the file a
context with that variant in its parameter block writes from that variant's rows."""
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

PAIRS_LOW, PAIRS_HIGH = [1.0, 1.0, 2.0], [10.0, 40.0, 160.0]
UNITS = [1.0e-16, 3.0e-16]


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return dict(params, **overrides)


# ---------------------------------------------------------------------------------------------------------------- exported symbols
def test_sweep_symbols_exported_and_declared(bl):
    lib = C.CDLL(bl.LIB_PATH)
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_write_output_variant", "bl_variant_output_path", "bl_apply_sweep", "bl_params_read_file_sweep",
                 "bl_params_set_line_sweep", "bl_sweep_resolve", "bl_num_variants"):
        assert hasattr(lib, name), name
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_SWEEP\s+16\b", header)
    from blacklight_amd import _capi
    assert C.sizeof(_capi.Sweep) == 16 + 3 * 16 * 8


# ---------------------------------------------------------------------------------------------------------------- grammar
def test_accepted_forms(bl):
    p = bl.Params.from_text("""
        sweep_rat_low  = 1, 1 ,2        # pairs
        sweep_rat_high = 10,40, 1.6e2
        sweep_rho_cgs  = 1e-16 , 3.0E-16
    """)
    assert p.has_sweep
    assert p.sweep_rat_low == [1.0, 1.0, 2.0] and p.sweep_rat_high == [10.0, 40.0, 160.0] and p.sweep_rho_cgs == [1.0e-16, 3.0e-16]
    assert p.resolved_sweep() == (False, [1.0, 1.0, 2.0], [10.0, 40.0, 160.0], [1.0e-16, 3.0e-16])
    q = p.copy()
    assert q.sweep_rat_high == [10.0, 40.0, 160.0] and q.sweep_rho_cgs == [1.0e-16, 3.0e-16]
    p.set_line("sweep_rho_cgs = 5e-17")   # a later line replaces the list, as a later line replaces any value
    assert p.sweep_rho_cgs == [5.0e-17] and q.sweep_rho_cgs == [1.0e-16, 3.0e-16]
    only_units = bl.Params.from_text("sweep_rho_cgs = 1e-16")
    assert only_units.sweep_rat_low == [] and only_units.sweep_rat_high == [] and only_units.sweep_rho_cgs == [1.0e-16]
    only_pairs = bl.Params.from_text("sweep_rat_low = 1\nsweep_rat_high = -3.5")   # (a negative ratio is the setter's to judge)
    assert only_pairs.sweep_rho_cgs == [] and only_pairs.resolved_sweep() == (False, [1.0], [-3.5], [])
    sixteen = bl.Params.from_text("sweep_rho_cgs = " + ",".join(f"{k + 1}e-16" for k in range(16)))
    assert len(sixteen.sweep_rho_cgs) == 16
    assert not bl.Params.from_text("camera_r = 50").has_sweep


def test_polarized_lists_become_triples(bl):
    base = _case("sim_polarized", plasma_rat_low=3.0, plasma_rat_high=30.0, simulation_rho_cgs=7.0e-17)

    def resolved(**sweep):
        p = bl.Params.from_dict(base)
        for key, values in sweep.items():
            p.set_line(f"sweep_{key} = {su.comma(values)}")
        return p.resolved_sweep()

    assert resolved(rat_low=[1, 1, 2], rat_high=[10, 40, 160], rho_cgs=[1e-16, 2e-16, 3e-16]) == \
        (True, [1.0, 1.0, 2.0], [10.0, 40.0, 160.0], [1e-16, 2e-16, 3e-16])
    assert resolved(rat_low=[1, 1, 2], rat_high=[10, 40, 160], rho_cgs=[2e-16]) == (True, [1.0, 1.0, 2.0], [10.0, 40.0, 160.0], [2e-16] * 3)
    assert resolved(rat_low=[1, 1], rat_high=[10, 40]) == (True, [1.0, 1.0], [10.0, 40.0], [7.0e-17] * 2)
    assert resolved(rho_cgs=[1e-16, 2e-16]) == (True, [3.0, 3.0], [30.0, 30.0], [1e-16, 2e-16])
    assert resolved() == (True, [], [], [])
    with pytest.raises(bl.BlacklightError) as err:
        resolved(rat_low=[1, 1, 2], rat_high=[10, 40, 160], rho_cgs=[1e-16, 2e-16])
    assert str(err.value) == "Error: sweep_rho_cgs must have one entry or as many as sweep_rat_high (2 and 3) with image_polarization in input file."


LINE_ERRORS = [
    ("sweep_rho_cgs = 1e-16,,2e-16", "Error: Empty entry in list (sweep_rho_cgs) in input file.\n"),
    ("sweep_rat_high = 10,40,", "Error: Empty entry in list (sweep_rat_high) in input file.\n"),
    ("sweep_rat_low = ,1", "Error: Empty entry in list (sweep_rat_low) in input file.\n"),
    ("sweep_rat_low =", "Error: Empty entry in list (sweep_rat_low) in input file.\n"),
    ("sweep_rat_high = 10,forty", "Error: Invalid number (forty) in list (sweep_rat_high) in input file.\n"),
    ("sweep_rho_cgs = 1e-16g", "Error: Invalid number (1e-16g) in list (sweep_rho_cgs) in input file.\n"),
    ("sweep_rat_low = 1;2", "Error: Invalid number (1;2) in list (sweep_rat_low) in input file.\n"),
    ("sweep_rho_cgs = 1e-16,nan", "Error: Invalid density unit (nan) in list (sweep_rho_cgs) in input file: must be finite and positive.\n"),
    ("sweep_rho_cgs = inf", "Error: Invalid density unit (inf) in list (sweep_rho_cgs) in input file: must be finite and positive.\n"),
    ("sweep_rho_cgs = 0", "Error: Invalid density unit (0) in list (sweep_rho_cgs) in input file: must be finite and positive.\n"),
    ("sweep_rho_cgs = 1e-16,-1e-16", "Error: Invalid density unit (-1e-16) in list (sweep_rho_cgs) in input file: must be finite and positive.\n"),
    ("sweep_rho_cgs = " + ",".join(["1e-16"] * 17), "Error: Too many entries in list (sweep_rho_cgs) in input file: at most 16 for this build.\n"),
    ("sweep_rat_high = " + ",".join(["10"] * 17), "Error: Too many entries in list (sweep_rat_high) in input file: at most 16 for this build.\n"),
    ("sweep_rat_mid = 1", "Error: Unknown key (sweep_rat_mid) in input file.\n"),
]


@pytest.mark.parametrize("line,message", LINE_ERRORS)
def test_line_error_texts(bl, line, message):
    """... through the entry point that keeps the lists and through the one that drops them (what a caller of bl_params_set_line sees)."""
    from blacklight_amd import _capi
    p = bl.Params()
    with pytest.raises(bl.BlacklightError) as err:
        p.set_line(line)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    text = C.create_string_buffer(1024)
    assert _capi.lib().bl_params_set_line(p.ptr, line.encode(), text, len(text)) == BL_E_INPUT
    assert text.value.decode() == message


def test_unequal_pair_lists_are_an_error_of_the_file(bl, tmp_path):
    from blacklight_amd import _capi
    message = "Error: sweep_rat_low and sweep_rat_high must have the same number of entries (3 and 2) in input file.\n"
    path = su.write_input(tmp_path / "bad.input", dict(_case("sim_multifreq"), sweep_rat_low="1,1,1", sweep_rat_high="10,40"))
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_file(path)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT
    block = bl.Params()
    text = C.create_string_buffer(1024)   # ... and of the entry point that keeps no lists: the command-line contract
    assert _capi.lib().bl_params_read_file(block.ptr, path.encode(), None, text, len(text)) == BL_E_INPUT
    assert text.value.decode() == message
    only_high = su.write_input(tmp_path / "half.input", dict(_case("sim_multifreq"), sweep_rat_high="10,40"))
    with pytest.raises(bl.BlacklightError) as err:
        bl.Params.from_file(only_high)
    assert str(err.value) == "Error: sweep_rat_low and sweep_rat_high must have the same number of entries (0 and 2) in input file."
    # line by line there is no end of file: the lists are held against each other when they are applied
    p = bl.Params.from_dict(_case("sim_multifreq"))
    p.set_line("sweep_rat_low = 1,1,1")
    p.set_line("sweep_rat_high = 10,40")
    with pytest.raises(bl.BlacklightError) as err:
        bl.Context(p, device=BL_DEVICE_NONE)
    assert str(err.value) + "\n" == message and err.value.code == BL_E_INPUT


def test_sweep_free_inputs_parse_to_the_same_block(bl, tmp_path):
    """Every golden case's input, as a file: the entry point that knows of sweeps and the one that does not fill the block with the
    same bytes and the same run count, and sweep keys added to the file change no byte of it."""
    from blacklight_amd import _capi
    L = _capi.lib()
    size = L.bl_params_sizeof()
    for case in gu.GPU_CASES:
        params = _case(case)
        plain = su.write_input(tmp_path / f"{case}.input", params)
        swept = su.write_input(tmp_path / f"{case}_sweep.input", dict(params, sweep_rat_low="1,1", sweep_rat_high="10,40", sweep_rho_cgs="2e-16"))
        old = bl.Params()
        runs_old, text = C.c_int(0), C.create_string_buffer(1024)
        assert L.bl_params_read_file(old.ptr, plain.encode(), C.byref(runs_old), text, len(text)) == 0, text.value
        new, with_keys = bl.Params.from_file(plain), bl.Params.from_file(swept)
        assert not new.has_sweep and with_keys.has_sweep
        want = C.string_at(old.ptr, size)
        assert C.string_at(new.ptr, size) == want, case
        assert C.string_at(with_keys.ptr, size) == want, case
        assert new.num_runs == runs_old.value == with_keys.num_runs
        by_line = bl.Params.from_dict(params)   # and line by line
        before = C.string_at(by_line.ptr, size)
        by_line.set_line("sweep_rho_cgs = 1e-16,2e-16")
        assert C.string_at(by_line.ptr, size) == before


# ---------------------------------------------------------------------------------------------------------------- bl_apply_sweep
def test_apply_makes_the_setter_calls(bl, tmp_path):
    path = su.write_input(tmp_path / "sweep.input", dict(_case("sim_multifreq"), sweep_rat_low=su.comma(PAIRS_LOW), sweep_rat_high=su.comma(PAIRS_HIGH),
                                                        sweep_rho_cgs=su.comma(UNITS)))
    with bl.Context.from_input(path, device=BL_DEVICE_NONE) as ctx:
        assert (ctx.num_electron_models, ctx.num_density_units, ctx.num_polarized_variants, ctx.num_variants) == (3, 2, 0, 6)
        assert ctx.electron_models == list(zip(PAIRS_HIGH, PAIRS_LOW)) and ctx.density_units == UNITS
        assert ctx.num_quantities == 6 * 3
    p = bl.Params.from_dict(_case("sim_multifreq"))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:   # no sweep: nothing set, one variant
        assert (ctx.num_electron_models, ctx.num_density_units, ctx.num_variants) == (0, 0, 1)
        ctx.set_density_units([1e-16, 2e-16])
        ctx.apply_sweep()                               # an empty sweep makes no call
        assert ctx.num_density_units == 2
    p.set_line("sweep_rho_cgs = 1e-16,2e-16,3e-16")
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:   # units alone: the block's own pair
        assert (ctx.num_electron_models, ctx.num_density_units, ctx.num_variants) == (0, 3, 3)
    q = bl.Params.from_dict(_case("sim_polarized"))
    q.set_line("sweep_rat_low = 1,1,2")
    q.set_line("sweep_rat_high = 10,40,160")
    q.set_line("sweep_rho_cgs = 2e-16")
    with bl.Context(q, device=BL_DEVICE_NONE) as ctx:
        assert (ctx.num_electron_models, ctx.num_density_units, ctx.num_polarized_variants, ctx.num_variants) == (0, 0, 3, 3)
        assert ctx.polarized_variants == [(10.0, 1.0, 2e-16), (40.0, 1.0, 2e-16), (160.0, 2.0, 2e-16)]


@pytest.mark.parametrize("case", ["formula_flat", "sim_code_kappa", "sim_adaptive"])
def test_what_a_setter_refuses_comes_in_its_own_words(bl, case):
    """Formula mode, code_kappa with pairs, adaptive runs: the parser does not know these conditions."""
    params = _case(case)
    plain = bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE)
    with pytest.raises(bl.BlacklightError) as direct:
        plain.set_electron_models([10.0, 40.0], rat_low=[1.0, 1.0])
    p = bl.Params.from_dict(params)
    p.set_line("sweep_rat_low = 1,1")
    p.set_line("sweep_rat_high = 10,40")
    with pytest.raises(bl.BlacklightError) as swept:
        bl.Context(p, device=BL_DEVICE_NONE)
    assert str(swept.value) == str(direct.value) and swept.value.code == direct.value.code == BL_E_UNSUPPORTED


def test_a_refused_second_list_leaves_no_first_list(bl):
    """A ratio that is not finite is the setter's BL_E_ARG; units refused after the models were accepted take the models back."""
    from blacklight_amd import _capi
    p = bl.Params.from_dict(_case("sim_multifreq"))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        sweep = _capi.Sweep()
        sweep.n_rat_low = sweep.n_rat_high = 2
        sweep.rat_low[0] = sweep.rat_low[1] = 1.0
        sweep.rat_high[0], sweep.rat_high[1] = 10.0, math.inf
        assert ctx._lib.bl_apply_sweep(ctx._ctx, C.byref(sweep)) == BL_E_ARG
        assert "bl_set_electron_models" in ctx._lib.bl_last_error(ctx._ctx).decode() and ctx.num_electron_models == 0
        sweep.rat_high[1] = 40.0
        sweep.n_rho_cgs = 2
        sweep.rho_cgs[0], sweep.rho_cgs[1] = 1e-16, -1.0   # (not reachable through the parser, which refuses the unit itself)
        assert ctx._lib.bl_apply_sweep(ctx._ctx, C.byref(sweep)) == BL_E_ARG
        assert "bl_set_density_units: unit 1 is not a finite value > 0." in ctx._lib.bl_last_error(ctx._ctx).decode()
        assert ctx.num_electron_models == 0 and ctx.num_density_units == 0 and ctx.num_variants == 1


# ---------------------------------------------------------------------------------------------------------------- the writer
def _rows(rng, n_rows, n_pix):
    image = rng.standard_normal((n_rows, n_pix)) * 10.0 ** rng.integers(-30, 5, size=(n_rows, 1))
    image[rng.random(image.shape) < 0.02] = np.nan
    return np.ascontiguousarray(image)


def _write_and_compare(bl, tmp_path, params, sweep_lines, variant_values, fmt, levels_extra, monkeypatch=None):
    """A sweep context writes each variant; a plain context with the variant's values in its block writes that variant's rows."""
    params = dict(params, output_format=fmt, output_file=str(tmp_path / f"sweep.{fmt}"))
    p = bl.Params.from_dict(params)
    for line in sweep_lines:
        p.set_line(line)
    rng = np.random.default_rng(20261016)
    names = []
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        n_variants = ctx.num_variants
        assert n_variants == len(variant_values)
        n_q = ctx.num_quantities // n_variants
        n_pix = ctx.resolution ** 2
        image = _rows(rng, n_variants * n_q, n_pix)
        level = dict(image=image, block_locs=None, **levels_extra(n_pix, rng))
        with pytest.raises(bl.BlacklightError) as err:   # bl_write_output keeps refusing the sweep
            ctx.write_output([level], path=tmp_path / "refused")
        assert err.value.code == BL_E_UNSUPPORTED and "the reference's file layout has no" in str(err.value)
        for v in range(n_variants):
            ctx.write_output([level], variant=v)
            names.append(ctx.variant_output_path(0, v))
            assert os.path.exists(names[-1]), names[-1]
        for bad in (-1, n_variants):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([level], variant=bad)
            assert err.value.code == BL_E_ARG
            with pytest.raises(bl.BlacklightError) as err:
                ctx.variant_output_path(0, bad)
            assert err.value.code == BL_E_ARG
    assert names == sorted(names) and len(set(names)) == n_variants   # names sort in variant order
    for v, (low, high, rho) in enumerate(variant_values):
        single = dict(params, plasma_rat_low=low, plasma_rat_high=high, simulation_rho_cgs=rho, output_file=str(tmp_path / f"single_{v}.{fmt}"))
        with bl.Context(bl.Params.from_dict(single), device=BL_DEVICE_NONE) as plain:
            assert plain.num_quantities == n_q
            plain.write_output([dict(level, image=image[v * n_q:(v + 1) * n_q])])
        got, want = su.file_bytes(names[v]), su.file_bytes(single["output_file"])
        assert got == want, (fmt, v)
        if fmt == "raw":
            assert got == image[v * n_q:(v + 1) * n_q].tobytes()
    return names


@pytest.mark.parametrize("fmt", ["npz", "npy", "raw"])
def test_unpolarized_three_by_two_files_equal_single_runs(bl, tmp_path, fmt):
    """M x U = 3 x 2, two frequencies, an auxiliary row and the camera record: variant m * U + u."""
    params = _case("sim_multifreq", image_num_frequencies=2, image_tau="true", output_camera="true")
    values = [(PAIRS_LOW[m], PAIRS_HIGH[m], UNITS[u]) for m in range(3) for u in range(2)]
    lines = [f"sweep_rat_low = {su.comma(PAIRS_LOW)}", f"sweep_rat_high = {su.comma(PAIRS_HIGH)}", f"sweep_rho_cgs = {su.comma(UNITS)}"]
    names = _write_and_compare(bl, tmp_path, params, lines, values, fmt, lambda n_pix, rng: dict(camera_pos=rng.standard_normal((n_pix, 4))))
    assert [os.path.basename(n) for n in names] == [f"sweep.m{m:02d}u{u:02d}.{fmt}" for m in range(3) for u in range(2)]


@pytest.mark.parametrize("fmt", ["npz", "npy"])   # (raw: "Only npz or npy outputs support polarization.", as in the reference)
def test_polarized_triples_files_equal_single_runs(bl, tmp_path, fmt):
    params = _case("sim_polarized", image_num_frequencies=2, image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log")
    values = [(1.0, 10.0, 1.0e-16), (1.0, 40.0, 2.0e-16), (2.0, 160.0, 4.0e-16)]
    lines = ["sweep_rat_low = 1,1,2", "sweep_rat_high = 10,40,160", "sweep_rho_cgs = 1e-16,2e-16,4e-16"]
    names = _write_and_compare(bl, tmp_path, params, lines, values, fmt, lambda n_pix, rng: {})
    assert [os.path.basename(n) for n in names] == [f"sweep.v{v:02d}.{fmt}" for v in range(3)]


def test_polarized_raw_is_refused_as_in_a_single_run(bl, tmp_path):
    p = bl.Params.from_dict(_case("sim_polarized", output_format="raw", output_file=str(tmp_path / "pol.raw")))
    p.set_line("sweep_rho_cgs = 1e-16,2e-16")
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        image = np.zeros((ctx.num_quantities, ctx.resolution ** 2))
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output([dict(image=image, block_locs=None)], variant=1)
        assert str(err.value) == "Error: Only npz or npy outputs support polarization."


def test_zip64_rules_hold_per_variant(bl, tmp_path, monkeypatch):
    monkeypatch.setenv("BLACKLIGHT_AMD_ZIP64", "always")
    params = _case("sim_multifreq", image_num_frequencies=2)
    values = [(1.0, 10.0, u) for u in UNITS]
    names = _write_and_compare(bl, tmp_path, params, [f"sweep_rho_cgs = {su.comma(UNITS)}"], values, "npz", lambda n_pix, rng: {})
    assert b"PK\x06\x06" in open(names[1], "rb").read()[-200:]
    got = np.load(names[1])
    assert got["I_nu"].shape == (2, 16, 16)


def test_one_variant_is_bl_write_output(bl, tmp_path):
    """V = 1 - no sweep, or lists of one entry: variant 0, the plain call's name and bytes; no other variant."""
    params = _case("sim_multifreq", output_file=str(tmp_path / "one.npz"))
    rng = np.random.default_rng(7)
    for lines in ([], ["sweep_rat_low = 2", "sweep_rat_high = 20", "sweep_rho_cgs = 3e-16"]):
        p = bl.Params.from_dict(params)
        for line in lines:
            p.set_line(line)
        with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
            assert ctx.num_variants == 1
            level = dict(image=_rows(rng, ctx.num_quantities, ctx.resolution ** 2), block_locs=None)
            assert ctx.variant_output_path(0, 0) == params["output_file"]
            ctx.write_output([level])
            plain = su.file_bytes(params["output_file"])
            os.remove(params["output_file"])
            ctx.write_output([level], variant=0)
            assert su.file_bytes(params["output_file"]) == plain
            other = tmp_path / "elsewhere.npz"
            ctx.write_output([level], path=other, variant=0)   # path_override wins
            assert su.file_bytes(other) == plain
            with pytest.raises(bl.BlacklightError) as err:
                ctx.write_output([level], variant=1)
            assert err.value.code == BL_E_ARG


def test_names_by_snapshot_and_variant(bl, tmp_path):
    params = _case("sim_dp_interp", simulation_multiple="true", simulation_start=7, simulation_end=9, output_file=str(tmp_path / "out.d/img_{04d}.npz"))
    p = bl.Params.from_dict(params)
    p.set_line("sweep_rat_low = " + ",".join(["1"] * 16))
    p.set_line("sweep_rat_high = " + ",".join(str(10 * (k + 1)) for k in range(16)))
    p.set_line("sweep_rho_cgs = " + ",".join(f"{k + 1}e-16" for k in range(16)))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        assert ctx.num_variants == 256
        assert ctx.variant_output_path(2, 16 * 3 + 11) == str(tmp_path / "out.d/img_0009.m03u11.npz")
        names = [ctx.variant_output_path(1, v) for v in range(256)]
        assert names == sorted(names) and len(set(names)) == 256
        buf = C.create_string_buffer(8)
        assert ctx._lib.bl_variant_output_path(ctx._ctx, 0, 0, buf, len(buf)) == BL_E_ARG   # a buffer too short for the name
    q = bl.Params.from_dict(dict(params, output_file=str(tmp_path / "out.d/no_extension_{02d}")))
    q.set_line("sweep_rho_cgs = 1e-16,2e-16")
    with bl.Context(q, device=BL_DEVICE_NONE) as ctx:   # the '.' of a directory is not an extension
        assert ctx.variant_output_path(0, 1) == str(tmp_path / "out.d/no_extension_07.m00u01")
    r = bl.Params.from_dict(_case("sim_polarized", output_file="image.npz"))
    r.set_line("sweep_rho_cgs = " + ",".join(f"{k + 1}e-16" for k in range(16)))
    with bl.Context(r, device=BL_DEVICE_NONE) as ctx:
        assert [ctx.variant_output_path(0, v) for v in (0, 7, 15)] == ["image.v00.npz", "image.v07.npz", "image.v15.npz"]


def test_adaptive_levels_cannot_come_with_a_sweep(bl, tmp_path):
    p = bl.Params.from_dict(_case("sim_multifreq", output_file=str(tmp_path / "a.npz")))
    p.set_line("sweep_rho_cgs = 1e-16,2e-16")
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        image = np.zeros((ctx.num_quantities, ctx.resolution ** 2))
        levels = [dict(image=image, block_locs=None), dict(image=image[:, :16], block_locs=np.zeros((1, 2), dtype=np.int32))]
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output(levels, variant=0)
        assert err.value.code == BL_E_ARG and "adaptive" in str(err.value)
