"""Electron mixes of an unpolarized run (bl_set_electron_mixes) on host-only contexts (no GPU): the exported symbols and the grown
bl_stats against ctypes, every argument error and refusal with its text, the shape values that are not read, the reference's two
warnings (each once per call), the order of bl_variants_get's rows for E x M x U x S, what n = 0 restores, what a refused call leaves,
and the eEE tag of the output names."""
import ctypes as C
import math
import os
import re

import pytest

import golden_util as gu

BL_DEVICE_NONE = -2
BL_E_UNSUPPORTED, BL_E_ARG = 3, 5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")

THERMAL = dict(power_frac=0.0, p=3.0, gamma_min=4.0, gamma_max=1000.0)
MIXES = [THERMAL, dict(power_frac=0.3, p=2.5, gamma_min=1.0, gamma_max=1000.0), dict(power_frac=0.5, p=3.5, gamma_min=10.0, gamma_max=1.0e5),
         dict(power_frac=0.05, p=2.2, gamma_min=2.0, gamma_max=500.0)]
PAIRS_LOW, PAIRS_HIGH = [1.0, 2.0], [10.0, 160.0]
UNITS = [1.0e-16, 3.0e-16]
CUTS = [1.0, -1.0]
WARN_POWER = "Warning: Fraction of power-law electrons outside [0, 1].\n"
WARN_THERMAL = "Warning: Fraction of thermal electrons outside [0, 1].\n"


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _case(name, **overrides):
    fx, params, mock_args = gu.load_case(name)
    return dict(params, **overrides)


def _context(bl, name, **overrides):
    return bl.Context(bl.Params.from_dict(_case(name, **overrides)), device=BL_DEVICE_NONE)


def _array(mappings):
    from blacklight_amd import _capi
    array = (_capi.ElectronMix * max(1, len(mappings)))()
    for e, mapping in enumerate(mappings):
        for key in KEYS:
            setattr(array[e], key, mapping.get(key, 0.0))
    return array


def _set(ctx, mappings, n=None):
    return ctx._lib.bl_set_electron_mixes(ctx._ctx, len(mappings) if n is None else n, C.cast(_array(mappings), C.c_void_p))


def _last_error(ctx):
    return ctx._lib.bl_last_error(ctx._ctx).decode().rstrip("\n")


def _warnings(ctx):
    return ctx._lib.bl_warnings(ctx._ctx).decode()


def _state(ctx):
    n = ctx.num_variants
    return (ctx.num_electron_mixes, ctx.electron_mixes, n, ctx.num_quantities, ctx._variants(), [ctx.variant_output_path(0, v) for v in range(n)])


# ---------------------------------------------------------------------------------------------------------------- header against ctypes
def test_symbols_exported_and_declared(bl):
    from blacklight_amd import _capi
    lib = C.CDLL(bl.LIB_PATH)
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    for name in ("bl_set_electron_mixes", "bl_num_electron_mixes", "bl_electron_mix_get"):
        assert hasattr(lib, name), name
        assert re.search(r"BL_API\s+int\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BL_MAX_ELECTRON_MIXES\s+16\b", header)
    assert re.search(r"int\s+bl_set_electron_mixes\(bl_ctx\s*\*ctx,\s*int\s+n,\s*const\s+bl_electron_mix\s*\*mix\);", header)
    assert re.search(r"int\s+bl_electron_mix_get\(const\s+bl_ctx\s*\*ctx,\s*int\s+e,\s*bl_electron_mix\s*\*out\);", header)
    assert len(_capi.lib().bl_set_electron_mixes.argtypes) == 3 and len(_capi.lib().bl_electron_mix_get.argtypes) == 3
    _capi.lib().bl_num_electron_mixes.restype = C.c_int
    assert _capi.lib().bl_num_electron_mixes(None) == -1          # no context
    assert _capi.lib().bl_set_electron_mixes(None, 0, None) == BL_E_ARG


def test_stats_gain_n_mixes_at_the_end(bl):
    """The struct's last member, an int32 behind n_cameras in what was tail padding: no other member moves, the size stays."""
    from blacklight_amd import _capi
    header = open(os.path.join(REPO, "include", "blacklight_amd.h")).read()
    assert re.search(r"int32_t\s+n_cameras;[^}]*int32_t\s+n_mixes;[^};]*(/\*[^}]*\*/)?\s*\}\s*bl_stats;", header, re.S)
    assert _capi.Stats.N_MIXES_OFFSET == _capi.Stats.n_cameras.offset + 4 == 164
    assert C.sizeof(_capi.Stats) == 168                            # what it was: every older member where it was
    with _context(bl, "sim_powerlaw") as ctx:
        assert ctx.stats.n_mixes == 0 and ctx.stats.n_cameras == 0   # no render yet


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_counts_getter_and_clearing(bl):
    with _context(bl, "sim_powerlaw") as ctx:
        n_q = ctx.num_quantities
        own = ctx._block_electrons()
        assert (own["power_frac"], own["p"], own["gamma_min"], own["gamma_max"]) == (0.3, 2.5, 1.0, 1000.0)
        before = _state(ctx)
        assert (ctx.num_electron_mixes, ctx.electron_mixes, ctx.num_variants) == (0, [], 1)
        from blacklight_amd import _capi
        mix = _capi.ElectronMix()
        assert ctx._lib.bl_electron_mix_get(ctx._ctx, 0, C.byref(mix)) == 0 and mix.power_frac == 0.3   # no list: the block's own
        assert ctx._lib.bl_electron_mix_get(ctx._ctx, 1, C.byref(mix)) == BL_E_ARG
        assert ctx._lib.bl_electron_mix_get(ctx._ctx, 0, None) == BL_E_ARG
        ctx.set_electron_mixes(MIXES)
        assert (ctx.num_electron_mixes, ctx.num_variants, ctx.num_quantities) == (4, 4, 4 * n_q)
        got = ctx.electron_mixes
        for e, want in enumerate(MIXES):
            assert {k: got[e][k] for k in want} == want
            assert (got[e]["kappa_frac"], got[e]["kappa"], got[e]["w"]) == (own["kappa_frac"], own["kappa"], own["w"])   # a missing key: the block's
        assert ctx._lib.bl_electron_mix_get(ctx._ctx, 4, C.byref(mix)) == BL_E_ARG
        ctx.set_electron_mixes(dict(power_frac=0.1))                # one mapping: one mix, the other keys the block's
        assert (ctx.num_electron_mixes, ctx.num_variants, ctx.num_quantities) == (1, 1, n_q)
        assert ctx.electron_mixes[0]["p"] == 2.5
        ctx.set_electron_mixes([THERMAL] * 16)
        assert ctx.num_variants == 16
        ctx.set_electron_mixes([])                                  # n = 0 restores the context
        assert _state(ctx) == before
        with pytest.raises(ValueError):
            ctx.set_electron_mixes([dict(power=0.1)])


ARG_ERRORS = [
    (dict(power_frac=math.nan), "has a power_frac that is not finite."),
    (dict(power_frac=math.inf), "has a power_frac that is not finite."),
    (dict(power_frac=0.2, p=math.nan, gamma_min=1.0, gamma_max=10.0), "has a p that is not finite."),
    (dict(power_frac=0.2, p=2.5, gamma_min=-math.inf, gamma_max=10.0), "has a gamma_min that is not finite."),
    (dict(power_frac=0.2, p=2.5, gamma_min=1.0, gamma_max=math.inf), "has a gamma_max that is not finite."),
]


@pytest.mark.parametrize("bad,text", ARG_ERRORS)
def test_argument_errors_name_the_mix(bl, bad, text):
    with _context(bl, "sim_powerlaw") as ctx:
        assert _set(ctx, [MIXES[1], MIXES[2]]) == 0
        before = _state(ctx)
        assert _set(ctx, [MIXES[0], MIXES[1], bad]) == BL_E_ARG
        assert _last_error(ctx) == "Error: bl_set_electron_mixes: mix 2 " + text
        assert _state(ctx) == before                                # a failed call changes nothing


def test_count_and_pointer_errors(bl):
    with _context(bl, "sim_powerlaw") as ctx:
        text = "Error: bl_set_electron_mixes needs 0 <= n <= 16 and the array of mixes."
        assert _set(ctx, [THERMAL] * 17) == BL_E_ARG and _last_error(ctx) == text
        assert _set(ctx, [], n=-1) == BL_E_ARG and _last_error(ctx) == text
        assert ctx._lib.bl_set_electron_mixes(ctx._ctx, 2, None) == BL_E_ARG and _last_error(ctx) == text
        assert ctx.num_electron_mixes == 0
        assert ctx._lib.bl_set_electron_mixes(ctx._ctx, 0, None) == 0   # clearing needs no array


def test_values_not_read_are_returned_as_given(bl):
    """With power_frac == 0 the shape values are neither read nor checked."""
    odd = dict(power_frac=0.0, p=math.nan, gamma_min=math.inf, gamma_max=-1.0)
    with _context(bl, "sim_powerlaw") as ctx:
        assert _set(ctx, [odd, MIXES[1]]) == 0 and _warnings(ctx) == ""
        got = ctx.electron_mixes[0]
        assert math.isnan(got["p"]) and got["gamma_min"] == math.inf and got["gamma_max"] == -1.0 and got["power_frac"] == 0.0


def test_the_two_warnings_each_once_per_call(bl):
    with _context(bl, "sim_powerlaw") as ctx:
        assert _warnings(ctx) == ""
        assert _set(ctx, MIXES) == 0 and _warnings(ctx) == ""
        outside = dict(MIXES[1], power_frac=1.5)                    # the power law above 1, the thermal part below 0
        assert _set(ctx, [outside, outside, MIXES[0]]) == 0
        assert _warnings(ctx) == WARN_POWER + WARN_THERMAL
        assert _set(ctx, [dict(MIXES[1], power_frac=-0.25)]) == 0   # ... below 0, the thermal part above 1
        assert _warnings(ctx) == (WARN_POWER + WARN_THERMAL) * 2
        before = _warnings(ctx)
        assert _set(ctx, [outside, dict(power_frac=math.nan)]) == BL_E_ARG   # a failed call warns of nothing
        assert _warnings(ctx) == before


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSALS = [
    ("formula_flat", {}, 1, "Error: Electron mixes: formula mode has no electron distribution (model_type = formula)."),
    ("sim_polarized", {}, 1, "Error: Electron mixes: a polarized run takes its electron distributions with its variants (image_polarization = true): "
                             "bl_set_polarized_variants_electrons."),
    ("slow_interp", {}, 1, "Error: Electron mixes: slow light renders one electron mix (slow_light_on = true)."),
    ("sim_adaptive", {}, 2, "Error: Electron mixes: adaptive refinement reads one image; n >= 2 mixes need adaptive_max_level = 0."),
    ("sim_render", {}, 2, "Error: Electron mixes: renderings come out once; n >= 2 mixes need render_num_images = 0."),
    ("sim_dp_interp", dict(checkpoint_geodesic_save="true", checkpoint_geodesic_file="geo.bin"), 2,
     "Error: Electron mixes: a geodesic checkpoint is saved by a render of one image; n >= 2 mixes need checkpoint_geodesic_save = false."),
    ("sim_dp_interp", dict(checkpoint_sample_save="true", checkpoint_sample_file="samples.bin"), 2,
     "Error: Electron mixes: a sample checkpoint is saved by a render of one image; n >= 2 mixes need checkpoint_sample_save = false."),
]


@pytest.mark.parametrize("case,overrides,least,message", REFUSALS)
def test_refusals(bl, case, overrides, least, message):
    with _context(bl, case, **overrides) as ctx:
        before = _state(ctx)
        if least == 2:
            ctx.set_electron_mixes([MIXES[1]])                      # one mix is a single image: allowed
            assert ctx.num_electron_mixes == 1
            ctx.set_electron_mixes([])
        with pytest.raises(bl.BlacklightError) as err:
            ctx.set_electron_mixes(MIXES[:2])
        assert str(err.value) == message and err.value.code == BL_E_UNSUPPORTED
        assert _state(ctx) == before                                # a refused call leaves the context as it was


def test_kappa_electrons_are_refused(bl):
    message = ("Error: Electron mixes: kappa-distribution electrons (kappa_frac != 0) in an unpolarized run - the reference's absorptivity reads "
               "kappa_aa_high_i, which it only initialises for polarized runs: no defined result to reproduce.")
    with _context(bl, "sim_powerlaw") as ctx:
        ctx.set_electron_mixes(MIXES[:2])
        before = _state(ctx)
        for n, mixes in ((1, [dict(MIXES[1], kappa_frac=0.1, kappa=4.0, w=1.0)]), (2, [MIXES[0], dict(THERMAL, kappa_frac=0.2, kappa=4.0, w=1.0)])):
            with pytest.raises(bl.BlacklightError) as err:
                ctx.set_electron_mixes(mixes)
            assert str(err.value) == message and err.value.code == BL_E_UNSUPPORTED, n
            assert _state(ctx) == before


def test_single_image_calls_refuse_two_mixes(bl, tmp_path):
    import numpy as np
    p = bl.Params.from_dict(_case("sim_multifreq", output_file=str(tmp_path / "a.npz")))
    with bl.Context(p, device=BL_DEVICE_NONE) as ctx:
        ctx.set_electron_mixes(MIXES[:2])
        image = np.zeros((ctx.num_quantities, ctx.resolution ** 2))
        with pytest.raises(bl.BlacklightError) as err:
            ctx.write_output([dict(image=image, block_locs=None)])
        assert err.value.code == BL_E_UNSUPPORTED and "the reference's file layout has no electron-mix axis (bl_set_electron_mixes with n >= 2)" in str(err.value)
        flags, count = np.zeros(4, dtype=np.uint8), C.c_int32(0)
        rc = ctx._lib.bl_adaptive_refine(ctx._ctx, 0, 4, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(count), None)
        assert rc == BL_E_UNSUPPORTED and "not with two or more electron mixes (bl_set_electron_mixes)" in _last_error(ctx)


# ---------------------------------------------------------------------------------------------------------------- rows and names
def test_variant_rows_are_mix_major(bl):
    """bl_variants_get for E x M x U x S = 3 x 2 x 2 x 2: the rows of models x units x cuts, repeated per mix."""
    with _context(bl, "sim_multifreq") as ctx:
        n_q = ctx.num_quantities
        ctx.set_electron_models(PAIRS_HIGH, rat_low=PAIRS_LOW)
        ctx.set_density_units(UNITS)
        ctx.set_sigma_cuts(CUTS)
        inner, _ = ctx._variants()
        assert len(inner[0]) == 8
        ctx.set_electron_mixes(MIXES[:3])
        assert (ctx.num_variants, ctx.num_quantities) == (24, 24 * n_q)
        (low, high, rho, cut), flags = ctx._variants()
        assert flags == 0
        want = [(PAIRS_LOW[m], PAIRS_HIGH[m], UNITS[u], CUTS[s]) for e in range(3) for m in range(2) for u in range(2) for s in range(2)]
        assert list(zip(low, high, rho, cut)) == want
        assert [low, high, rho, cut] == [column * 3 for column in inner]
        assert ctx.electron_models == list(zip(PAIRS_HIGH, PAIRS_LOW)) and ctx.density_units == UNITS and ctx.sigma_cuts == CUTS
        ctx.set_sigma_cuts([])                                      # another list changes: the mixes stay
        assert (ctx.num_electron_mixes, ctx.num_variants) == (3, 12)


def test_every_row_of_the_product_has_its_tag_and_its_values(bl, tmp_path):
    """E x M x U x S = 3 x 2 x 2 x 2, all 24 rows: row v = ((e 2 + m) 2 + u) 2 + s is named eEEmMMuUUsSS and holds model m's pair,
    unit u's value and cut s's value."""
    params = _case("sim_multifreq", output_file=str(tmp_path / "image.npz"))
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_electron_mixes(MIXES[:3])
        ctx.set_electron_models(PAIRS_HIGH, rat_low=PAIRS_LOW)
        ctx.set_density_units(UNITS)
        ctx.set_sigma_cuts(CUTS)
        assert ctx.num_variants == 24
        (low, high, rho, cut), _ = ctx._variants()
        assert len(low) == len(high) == len(rho) == len(cut) == 24
        seen = set()
        for v in range(24):
            tag = re.fullmatch(r"image\.e(\d\d)m(\d\d)u(\d\d)s(\d\d)\.npz", os.path.basename(ctx.variant_output_path(0, v)))
            assert tag, (v, ctx.variant_output_path(0, v))
            e, m, u, s = (int(digits) for digits in tag.groups())
            assert e < 3 and m < 2 and u < 2 and s < 2 and v == ((e * 2 + m) * 2 + u) * 2 + s, (v, e, m, u, s)
            assert (low[v], high[v], rho[v], cut[v]) == (PAIRS_LOW[m], PAIRS_HIGH[m], UNITS[u], CUTS[s]), v
            seen.add((e, m, u, s))
        assert len(seen) == 24


def test_names_carry_the_mix_in_front(bl, tmp_path):
    params = _case("sim_dp_interp", output_file=str(tmp_path / "image.npz"))
    with bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE) as ctx:
        ctx.set_electron_models(PAIRS_HIGH, rat_low=PAIRS_LOW)
        ctx.set_density_units(UNITS)
        plain = [ctx.variant_output_path(0, v) for v in range(4)]
        assert plain == [str(tmp_path / f"image.m{m:02d}u{u:02d}.npz") for m in range(2) for u in range(2)]   # without the axis: as ever
        ctx.set_electron_mixes(MIXES[:3])
        names = [ctx.variant_output_path(0, v) for v in range(12)]
        assert names == [str(tmp_path / f"image.e{e:02d}m{m:02d}u{u:02d}.npz") for e in range(3) for m in range(2) for u in range(2)]
        assert names == sorted(names)
        ctx.set_sigma_cuts(CUTS)
        names = [ctx.variant_output_path(0, v) for v in range(24)]
        assert names == [str(tmp_path / f"image.e{e:02d}m{m:02d}u{u:02d}s{s:02d}.npz") for e in range(3) for m in range(2) for u in range(2) for s in range(2)]
        ctx.set_electron_models([])
        ctx.set_density_units([])
        ctx.set_sigma_cuts([])
        assert [ctx.variant_output_path(0, v) for v in range(3)] == [str(tmp_path / f"image.e{e:02d}m00u00.npz") for e in range(3)]   # mixes alone
        ctx.set_electron_mixes(MIXES[1])                            # one image: the plain name
        assert ctx.variant_output_path(0, 0) == str(tmp_path / "image.npz")
        ctx.set_cameras([30.0, 60.0])
        ctx.set_electron_mixes(MIXES[:2])
        assert ctx.variant_output_path(0, 1, camera=1) == str(tmp_path / "image.c01e01m00u00.npz")
        ctx.set_electron_mixes([])
        ctx.set_cameras([])
        assert ctx.variant_output_path(0, 0) == str(tmp_path / "image.npz")
