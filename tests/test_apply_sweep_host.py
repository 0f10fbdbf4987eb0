"""bl_apply_sweep_lists as one checked step, and the context as the only record of what it renders - on host-only contexts (no GPU):
a refused apply leaves a context that already held lists exactly as it was (every list, every camera frame, byte for byte), two
faults in one call report the one the earlier library reported, and Context's properties read the context (bl_variants_get), so they
are right after calls through the C interface, after a refusal and after the two flux fits."""
import ctypes as C
import math

import numpy as np
import pytest

import golden_util as gu

BL_DEVICE_NONE = -2
BL_E_INPUT, BL_E_UNSUPPORTED, BL_E_ARG = 1, 3, 5
TRIPLES_CUT, TRIPLES_MIX = 1, 2   # BL_VARIANTS_TRIPLES_CUT, BL_VARIANTS_TRIPLES_MIX

POWER = dict(power_frac=0.3, p=2.5, gamma_min=2.0, gamma_max=1000.0, kappa_frac=0.0, kappa=0.0, w=0.0)
KAPPA = dict(power_frac=0.0, p=0.0, gamma_min=0.0, gamma_max=0.0, kappa_frac=0.4, kappa=4.0, w=1.5)


@pytest.fixture()
def bl(built_library):
    import blacklight_amd
    return blacklight_amd


def _context(bl, case, tmp_path, **overrides):
    fx, params, mock_args = gu.load_case(case)
    return bl.Context(bl.Params.from_dict(dict(params, output_file=str(tmp_path / "image.npz"), **overrides)), device=BL_DEVICE_NONE)


def _lists(sweep=None, cuts=None, cameras=None, electrons=None):
    """A bl_sweep_lists from plain lists: sweep = dict(rat_low, rat_high, rho_cgs), cuts = [...], cameras = dict(th, ph), electrons =
    dict(kappa = [...], ...); a cut list of more than BL_MAX_SWEEP entries sets the count alone. None: a NULL member."""
    from blacklight_amd import _capi
    made = {}
    for name, struct, given in (("sweep", _capi.Sweep, sweep), ("cameras", _capi.SweepCameras, cameras), ("electrons", _capi.SweepElectrons, electrons),
                                ("cuts", _capi.SweepCuts, None if cuts is None else dict(sigma_max=cuts))):
        if given is None:
            continue
        made[name] = struct()
        for key, values in given.items():
            setattr(made[name], "n_" + key, len(values))
            for k, x in enumerate(values[:_capi.BL_MAX_SWEEP]):
                getattr(made[name], key)[k] = x
    lists = _capi.SweepLists(*(C.pointer(made[name]) if name in made else None for name in ("sweep", "cuts", "cameras", "electrons")))
    lists.keep = made
    return lists


def _apply(ctx, lists):
    rc = ctx._lib.bl_apply_sweep_lists(ctx._ctx, C.byref(lists))
    return rc, ctx._lib.bl_last_error(ctx._ctx).decode()


def _state(ctx):
    """Everything a context holds that an apply can change, as bytes and plain values."""
    from blacklight_amd import _capi
    lib, n = ctx._lib, ctx.num_variants
    rows, flags = np.full((4, n), np.nan), C.c_int(-1)
    assert lib.bl_variants_get(ctx._ctx, n, *(row.ctypes.data_as(C.c_void_p) for row in rows), C.byref(flags)) == 0
    n_cameras, n_pol = ctx.num_cameras, ctx.num_polarized_variants
    angles = np.full((2, max(1, n_cameras)), np.nan)
    assert lib.bl_cameras_get(ctx._ctx, n_cameras, *(row.ctypes.data_as(C.c_void_p) for row in angles)) == 0
    mixes = []
    for v in range(max(1, n_pol)):
        mix = _capi.ElectronMix()
        assert lib.bl_polarized_variant_electrons(ctx._ctx, v, C.byref(mix)) == 0
        mixes.append(bytes(mix))
    return dict(rows=rows.tobytes(), flags=flags.value,
                counts=(ctx.num_electron_models, ctx.num_density_units, ctx.num_sigma_cuts, n_pol, n_cameras, n), num_quantities=ctx.num_quantities,
                paths=[ctx.variant_output_path(0, v, c) for c in range(max(1, n_cameras)) for v in range(n)], angles=angles.tobytes(),
                frames=[bytes(ctx.camera_frame_of(c)) for c in range(max(1, n_cameras))], frame=bytes(ctx.camera_frame), electrons=mixes,
                warnings=ctx.warnings)


# ---------------------------------------------------------------------------------------------------------------- all or nothing
HELD = dict(sweep=dict(rat_low=[1.0, 2.0], rat_high=[10.0, 40.0], rho_cgs=[1.0e-16, 3.0e-16]), cuts=[1.0, -1.0], cameras=dict(ph=[10.0, 250.0]))
# lists an apply would accept, in front of the fault of each case: an apply that stored list by list would have changed them
NEW_CAMERAS, NEW_PAIRS = dict(th=[30.0, 40.0, 50.0]), dict(rat_low=[3.0, 3.0, 3.0], rat_high=[5.0, 6.0, 7.0])
REFUSED = [
    ("camera lengths", "sim_multifreq", {}, HELD, dict(sweep=NEW_PAIRS, cuts=[2.0], cameras=dict(th=[17.0, 60.0], ph=[0.0, 0.0, 90.0])),
     BL_E_INPUT, "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (3 and 2) in input file.\n"),
    ("camera refusal", "sim_multifreq", dict(image_crossings="true"), dict(HELD, cameras=dict(ph=[250.0])), dict(sweep=NEW_PAIRS, cuts=[2.0], cameras=NEW_CAMERAS),
     BL_E_UNSUPPORTED, "Error: Cameras: image_crossings counts crossings of one camera's plane; n >= 2 cameras need image_crossings = false.\n"),
    ("model", "sim_multifreq", {}, HELD, dict(sweep=dict(rat_low=[3.0, 3.0], rat_high=[5.0, math.inf]), cuts=[2.0], cameras=NEW_CAMERAS),
     BL_E_ARG, "Error: bl_set_electron_models: model 1 has a ratio that is not finite.\n"),
    ("unit", "sim_multifreq", {}, HELD, dict(sweep=dict(NEW_PAIRS, rho_cgs=[2.0e-16, 0.0]), cuts=[2.0], cameras=NEW_CAMERAS),
     BL_E_ARG, "Error: bl_set_density_units: unit 1 is not a finite value > 0.\n"),
    ("cuts", "sim_render", {}, dict(sweep=dict(rat_low=[2.0], rat_high=[40.0], rho_cgs=[3.0e-16]), cuts=[1.0], cameras=dict(ph=[10.0, 250.0])),
     dict(sweep=dict(rat_low=[3.0], rat_high=[5.0], rho_cgs=[2.0e-16]), cuts=[2.0, 3.0], cameras=NEW_CAMERAS),
     BL_E_UNSUPPORTED, "Error: Sigma cuts: a cut cell drops out of a rendering, and renderings come out once; n >= 2 cuts need render_num_images = 0.\n"),
]


@pytest.mark.parametrize("name, case, overrides, held, refused, code, text", REFUSED, ids=[entry[0] for entry in REFUSED])
def test_a_refused_apply_changes_nothing_a_context_held(bl, tmp_path, name, case, overrides, held, refused, code, text):
    with _context(bl, case, tmp_path, **overrides) as ctx:
        assert _apply(ctx, _lists(**held))[0] == 0
        before = _state(ctx)
        n_cameras = len(held["cameras"]["ph"])
        assert before["counts"] == (len(held["sweep"]["rat_low"]), len(held["sweep"]["rho_cgs"]), len(held["cuts"]), 0, n_cameras, np.prod(before["counts"][:3]))
        own_th = ctx.params.get("camera_th") * 180.0 / math.pi   # (the block's own camera_th: its radians, which no degree value need give back)
        assert ctx.cameras == [(own_th, ph) for ph in held["cameras"]["ph"]]
        assert _apply(ctx, _lists(**refused)) == (code, text)
        assert _state(ctx) == before


def test_a_refused_polarized_apply_changes_nothing_a_context_held(bl, tmp_path):
    """Triples with their own cuts and mixes, and cameras at the block's own camera_th; the mix check (kappa = 6) refuses the tuples
    after the call's cameras were accepted."""
    from blacklight_amd import _capi
    with _context(bl, "sim_polarized", tmp_path) as ctx:
        assert _apply(ctx, _lists(cameras=dict(ph=[10.0, 250.0])))[0] == 0
        low, high, rho, cut = (np.array(v) for v in ([1.0, 2.0], [10.0, 40.0], [1.0e-16, 3.0e-16], [0.5, -1.0]))
        mixes = (_capi.ElectronMix * 2)()
        for v, mapping in enumerate((POWER, KAPPA)):
            for key, value in mapping.items():
                setattr(mixes[v], key, value)
        assert ctx._lib.bl_set_polarized_variants_electrons(ctx._ctx, 2, *(a.ctypes.data_as(C.c_void_p) for a in (low, high, rho, cut)), C.cast(mixes, C.c_void_p)) == 0
        before = _state(ctx)
        assert before["counts"] == (0, 0, 0, 2, 2, 2) and before["flags"] == TRIPLES_CUT | TRIPLES_MIX
        assert before["electrons"] == [bytes(mixes[0]), bytes(mixes[1])] and ctx.polarized_electrons == [POWER, KAPPA]
        refused = _lists(sweep=NEW_PAIRS, cameras=NEW_CAMERAS, electrons=dict(kappa_frac=[0.4], kappa=[4.0, 6.0, 4.5], w=[1.5]))
        assert _apply(ctx, refused) == (BL_E_ARG, "Error: bl_set_polarized_variants_electrons: variant 1: Polarized transport only supports kappa in [3.5, 5].\n")
        assert _state(ctx) == before and ctx.polarized_electrons == [POWER, KAPPA]


# ---------------------------------------------------------------------------------------------------------------- the first failure
BAD_CAMERAS = dict(th=[17.0, 60.0], ph=[0.0, 0.0, 90.0])
PAIRS = dict(rat_low=[1.0, 1.0], rat_high=[10.0, 40.0])
ELECTRONS = dict(kappa_frac=[0.4], kappa=[4.0], w=[1.5])
# Two faults in one call. Every expected code and text is what the library before this test existed returned for the entry - the four
# nested apply calls, each through the public setters - recorded by running this table against it; none is taken from the one apply.
TWO_FAULTS = [
    ("camera lengths, unsupported models", "formula_64", dict(sweep=PAIRS, cameras=BAD_CAMERAS),
     BL_E_INPUT, "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (3 and 2) in input file.\n"),
    ("non-finite model, bad unit", "sim_multifreq", dict(sweep=dict(rat_low=[1.0, 1.0], rat_high=[10.0, math.inf], rho_cgs=[-1.0])),
     BL_E_ARG, "Error: bl_set_electron_models: model 1 has a ratio that is not finite.\n"),
    ("bad unit, refused cuts", "sim_render", dict(sweep=dict(rat_low=[1.0], rat_high=[40.0], rho_cgs=[-1.0]), cuts=[1.0, 3.0]),
     BL_E_ARG, "Error: bl_set_density_units: unit 0 is not a finite value > 0.\n"),
    ("too many cuts, unequal pairs", "sim_multifreq", dict(sweep=dict(rat_low=[1.0], rat_high=[10.0, 40.0]), cuts=[1.0] * 17),
     BL_E_INPUT, "Error: Too many entries in a sweep list: at most 16 for this build.\n"),
    ("polarized: bad unit, refused cuts", "sim_polarized", dict(sweep=dict(PAIRS, rho_cgs=[1.0e-16, -1.0]), cuts=[1.0, 3.0]),
     BL_E_ARG, "Error: bl_set_polarized_variants: the unit of variant 1 is not a finite value > 0.\n"),
    ("electrons: camera lengths, electron lists without polarization", "formula_64", dict(sweep=PAIRS, cameras=BAD_CAMERAS, electrons=ELECTRONS),
     BL_E_INPUT, "Error: sweep_kappa_frac needs image_polarization = true in input file.\n"),
    ("electrons: camera lengths, unsupported variants", "sim_polarized_adaptive", dict(sweep=PAIRS, cameras=BAD_CAMERAS, electrons=ELECTRONS),
     BL_E_INPUT, "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (3 and 2) in input file.\n"),
    ("electrons: non-finite model, bad unit", "sim_polarized", dict(sweep=dict(rat_low=[1.0, 1.0], rat_high=[10.0, math.inf], rho_cgs=[-1.0]), electrons=ELECTRONS),
     BL_E_ARG, "Error: bl_set_polarized_variants: the unit of variant 0 is not a finite value > 0.\n"),
    ("electrons: bad unit, refused cuts", "sim_polarized", dict(sweep=dict(PAIRS, rho_cgs=[1.0e-16, -1.0]), cuts=[1.0, 3.0], electrons=ELECTRONS),
     BL_E_UNSUPPORTED, "Error: Sigma cuts: the polarized axis is not built yet; polarized runs render one sigma cut (image_polarization = true).\n"),
    ("electrons: too many cuts, unequal pairs", "sim_polarized", dict(sweep=dict(rat_low=[1.0], rat_high=[10.0, 40.0]), cuts=[1.0] * 17, electrons=ELECTRONS),
     BL_E_INPUT, "Error: sweep_rat_low and sweep_rat_high must have the same number of entries (1 and 2) in input file.\n"),
]


@pytest.mark.parametrize("name, case, lists, code, text", TWO_FAULTS, ids=[entry[0] for entry in TWO_FAULTS])
def test_of_two_faults_the_first_is_reported(bl, tmp_path, name, case, lists, code, text):
    with _context(bl, case, tmp_path) as ctx:
        before = _state(ctx)
        assert _apply(ctx, _lists(**lists)) == (code, text)
        assert _state(ctx) == before


# ---------------------------------------------------------------------------------------------------------------- Python reads the context
def _ptrs(*lists):
    arrays = [np.array(values, dtype=np.float64) for values in lists]
    return arrays, [a.ctypes.data_as(C.c_void_p) for a in arrays]


def test_properties_read_what_the_c_interface_set(bl, tmp_path):
    with _context(bl, "sim_multifreq", tmp_path) as ctx:
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts, ctx.polarized_variants, ctx.polarized_cuts) == ([], [], [], [], None)
        keep, (low, high, rho, cuts) = _ptrs([1.0, 2.0, 3.0], [10.0, 40.0, 160.0], [1.0e-16, 3.0e-16], [1.0, -1.0])
        assert ctx._lib.bl_set_sigma_cuts(ctx._ctx, 2, cuts) == 0
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts) == ([], [], [1.0, -1.0])
        assert ctx._lib.bl_set_electron_models(ctx._ctx, 3, low, high) == 0
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts) == ([(10.0, 1.0), (40.0, 2.0), (160.0, 3.0)], [], [1.0, -1.0])
        assert ctx._lib.bl_set_density_units(ctx._ctx, 2, rho) == 0
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts) == ([(10.0, 1.0), (40.0, 2.0), (160.0, 3.0)], [1.0e-16, 3.0e-16], [1.0, -1.0])
        assert ctx._lib.bl_set_sigma_cuts(ctx._ctx, 0, None) == 0 and ctx._lib.bl_set_electron_models(ctx._ctx, 0, None, None) == 0
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts) == ([], [1.0e-16, 3.0e-16], [])
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set) == ([], None, False)
    with _context(bl, "sim_polarized", tmp_path) as ctx:
        from blacklight_amd import _capi
        keep, (low, high, rho, cuts) = _ptrs([1.0, 2.0], [10.0, 40.0], [1.0e-16, 3.0e-16], [0.5, -1.0])
        mixes = (_capi.ElectronMix * 2)()
        for v, mapping in enumerate((POWER, KAPPA)):
            for key, value in mapping.items():
                setattr(mixes[v], key, value)
        triples, block = [(10.0, 1.0, 1.0e-16), (40.0, 2.0, 3.0e-16)], ctx.polarized_electrons
        assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 2, low, high, rho) == 0
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set, ctx.polarized_electrons) == (triples, None, False, block * 2)
        assert ctx._lib.bl_set_polarized_variants_sigma(ctx._ctx, 2, low, high, rho, cuts) == 0
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set, ctx.polarized_electrons) == (triples, [0.5, -1.0], False, block * 2)
        assert ctx._lib.bl_set_polarized_variants_electrons(ctx._ctx, 2, low, high, rho, None, C.cast(mixes, C.c_void_p)) == 0
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set, ctx.polarized_electrons) == (triples, None, True, [POWER, KAPPA])
        assert ctx._lib.bl_set_polarized_variants_electrons(ctx._ctx, 2, low, high, rho, cuts, C.cast(mixes, C.c_void_p)) == 0
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set, ctx.polarized_electrons) == (triples, [0.5, -1.0], True, [POWER, KAPPA])
        assert (ctx.electron_models, ctx.density_units, ctx.sigma_cuts) == ([], [], [])
        assert ctx._lib.bl_set_polarized_variants(ctx._ctx, 0, None, None, None) == 0
        assert (ctx.polarized_variants, ctx.polarized_cuts, ctx.polarized_electrons_set, ctx.polarized_electrons) == ([], None, False, block)


def test_properties_after_a_refused_apply_are_the_lists_held_before(bl, tmp_path):
    with _context(bl, "sim_multifreq", tmp_path) as ctx:
        ctx.set_electron_models([10.0, 40.0], rat_low=[1.0, 2.0])
        ctx.set_density_units([1.0e-16, 3.0e-16])
        ctx.set_sigma_cuts([1.0, -1.0])
        ctx.set_cameras([17.0, 60.0], [0.0, 90.0])
        p = ctx.params.copy()
        for line in ("sweep_camera_th = 30,40,50", "sweep_rat_low = 3,3,3", "sweep_rat_high = 5,6,7", "sweep_rho_cgs = 2e-16", "sweep_cut_sigma_max = 1,3",
                     "sweep_camera_ph = 1,2"):
            p.set_line(line)
        with pytest.raises(bl.BlacklightError) as err:
            ctx.apply_sweep(p)
        assert err.value.code == BL_E_INPUT and str(err.value) == "Error: sweep_camera_ph must have one entry or as many as sweep_camera_th (2 and 3) in input file."
        assert ctx.electron_models == [(10.0, 1.0), (40.0, 2.0)] and ctx.density_units == [1.0e-16, 3.0e-16] and ctx.sigma_cuts == [1.0, -1.0]
        assert ctx.cameras == [(17.0, 0.0), (60.0, 90.0)] and ctx.num_variants == 8
    with _context(bl, "sim_polarized", tmp_path) as ctx:
        ctx.set_polarized_variants([10.0, 40.0], [1.0e-16, 3.0e-16], rat_low=[1.0, 2.0], sigma_max=[0.5, -1.0], electrons=[POWER, KAPPA])
        p = ctx.params.copy()
        for line in ("sweep_rat_low = 3,3,3", "sweep_rat_high = 5,6,7", "sweep_kappa_frac = 0.4", "sweep_kappa = 6", "sweep_w = 1.5"):
            p.set_line(line)
        with pytest.raises(bl.BlacklightError) as err:
            ctx.apply_sweep(p)
        assert err.value.code == BL_E_ARG and "variant 0: Polarized transport only supports kappa in [3.5, 5]." in str(err.value)
        assert ctx.polarized_variants == [(10.0, 1.0, 1.0e-16), (40.0, 2.0, 3.0e-16)] and ctx.polarized_cuts == [0.5, -1.0]
        assert ctx.polarized_electrons_set and ctx.polarized_electrons == [POWER, KAPPA]


def test_the_flux_fits_leave_the_context_byte_for_byte_as_it_was(bl, tmp_path):
    """Driven as tests/test_density_units_host.py and tests/test_polarized_electrons_host.py drive them: a stub render of uniform
    images whose flux is a power law of the unit."""
    from blacklight_amd import flux
    with _context(bl, "sim_dp_interp", tmp_path) as ctx:
        ctx.set_electron_models([10.0, 40.0], rat_low=[1.0, 2.0])
        ctx.set_density_units([5.0e-17])
        before = _state(ctx)
        per_jy = 1.0 / flux.total_flux_jy(np.ones((1, 4)), ctx.params, 8.1e3)

        def render():   # total flux 0.1 R_high rho / 1e-16 Jy for the one model and every unit set
            (high, _), = ctx.electron_models
            image = np.array([np.full((1, 4), 0.1 * high * (rho / 1.0e-16) * per_jy) for rho in ctx.density_units])
            return dict(image=image.reshape(-1, 4), image_by_unit=image[None])

        ctx.render = render
        rho, got, renders = ctx.fit_density_unit(2.0, 8.1e3, 1.0e-18, 1.0e-14, rtol=1.0e-3, per_render=8)
        assert [abs(f - 2.0) <= 2.0e-3 for f in got] == [True, True] and renders >= 2
        assert _state(ctx) == before
    with _context(bl, "sim_polarized", tmp_path) as ctx:
        ctx.set_polarized_variants([7.0, 9.0], [5.0e-17, 6.0e-17], sigma_max=[0.5, -1.0], electrons=[POWER, KAPPA])
        before = _state(ctx)
        assert before["flags"] == TRIPLES_CUT | TRIPLES_MIX

        def render():   # Stokes-I flux 0.01 R_high rho / 1e-16 Jy for every variant set
            variants = ctx.polarized_variants
            image = np.zeros((len(variants), 4, 4))
            for v, (high, low, rho) in enumerate(variants):
                image[v, 0] = 0.01 * high * (rho / 1.0e-16) * per_jy
            return dict(image=image.reshape(-1, 4), image_by_variant=image)

        ctx.render = render
        found, renders = ctx.fit_density_units_polarized([(10.0, 1.0)], 1.0, 8.1e3, 1.0e-18, 1.0e-12, rtol=1.0e-3)
        assert abs(found[0][1] - 1.0) <= 1.0e-3 and renders >= 2
        assert _state(ctx) == before
