"""GPU: the seven electron lists (sweep_power_frac ... sweep_w) written in the .input file of a polarized run, rendered by
bin/blacklight_amd in one render per snapshot and written as one reference-layout file per tuple - each file, byte for byte
(sweep_util.file_bytes), the file of a run of its own with that tuple's pair and seven plasma_* values in the parameter block, in
the exact tier. Every command-line run is a fresh child process with a time limit; a test stops at the first one that fails."""
import os

import pytest

import golden_util as gu
import sweep_util as su

pytestmark = pytest.mark.gpu

EXACT = {"BLACKLIGHT_AMD_ARITHMETIC": "exact"}
# two pairs, and with them the seven keys: lists of two, and lists of one (every variant at that value)
PAIRS = [(1.0, 10.0), (1.0, 40.0)]
KEYS = dict(sweep_rat_low=su.comma(p[0] for p in PAIRS), sweep_rat_high=su.comma(p[1] for p in PAIRS), sweep_power_frac="0.3,0.2", sweep_p="2.5,3",
            sweep_gamma_min="2", sweep_gamma_max="1000,500", sweep_kappa_frac="0,0.25", sweep_kappa="4.3", sweep_w="1.5,2.5")
BLOCKS = [dict(plasma_rat_low=1.0, plasma_rat_high=10.0, plasma_power_frac=0.3, plasma_p=2.5, plasma_gamma_min=2, plasma_gamma_max=1000, plasma_kappa_frac=0,
               plasma_kappa=4.3, plasma_w=1.5),
          dict(plasma_rat_low=1.0, plasma_rat_high=40.0, plasma_power_frac=0.2, plasma_p=3, plasma_gamma_min=2, plasma_gamma_max=500, plasma_kappa_frac=0.25,
               plasma_kappa=4.3, plasma_w=2.5)]


def _params_with_grid(case, directory, **overrides):
    fx, params, mock_args = gu.load_case(case)
    grid_path = directory / "grid.blgrid"
    if not grid_path.exists():
        gu.golden_grid(mock_args).save_raw(grid_path)
    return dict(params, simulation_file=str(grid_path), **overrides), mock_args


def _tagged(path, tag):
    stem, ext = os.path.splitext(str(path))
    return f"{stem}.{tag}{ext}"


def test_tuples_of_the_input_file_equal_runs_of_their_own(built_library, tmp_path):
    import blacklight_amd as bl
    params, mock_args = _params_with_grid("sim_polarized_kappa", tmp_path)
    out = tmp_path / "sweep.npz"
    run = su.run_cli(su.write_input(tmp_path / "sweep.input", dict(params, output_file=str(out), **KEYS)), EXACT)
    assert "blacklight_amd: sweep of 2 variants per snapshot (2 polarized triples)" in run.stdout
    files = [_tagged(out, f"v{v:02d}") for v in range(2)]
    for v, block in enumerate(BLOCKS):
        single = tmp_path / f"single_{v}.npz"
        su.run_cli(su.write_input(tmp_path / f"single_{v}.input", dict(params, output_file=str(single), **block)), EXACT)
        assert su.file_bytes(files[v]) == su.file_bytes(single), (v, block)
    assert not out.exists()
    assert su.file_bytes(files[0]) != su.file_bytes(files[1])
    # ... and the Context route: one pass, the command line's files
    path = su.write_input(tmp_path / "context.input", dict(params, output_file=str(tmp_path / "context.npz"), **KEYS))
    with bl.Context.from_input(path) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(mock_args))
        got = ctx.render()
        assert got["stats"].launches_shade == got["stats"].n_chunks and ctx.num_variants == 2
        assert [m["power_frac"] for m in ctx.polarized_electrons] == [0.3, 0.2] and [m["w"] for m in ctx.polarized_electrons] == [1.5, 2.5]
        for v in range(2):
            ctx.write_output([dict(got, block_locs=None)], variant=v)
            assert su.file_bytes(ctx.variant_output_path(0, v)) == su.file_bytes(files[v]), v


def test_electron_lists_alone_and_two_cameras(built_library, tmp_path):
    """No pairs, no units, no power-law lists (the block's values): N is the longest electron list, at the block's pair and unit; with two
    cameras one file per (camera, tuple)"""
    params, mock_args = _params_with_grid("sim_polarized_kappa", tmp_path)
    cameras = [(60.0, 0.0), (35.0, 80.0)]
    keys = dict(sweep_kappa_frac="0.4,0,1", sweep_kappa="4,4,4.5", sweep_w="1.5,1.5,1", sweep_camera_th=su.comma(c[0] for c in cameras),
                sweep_camera_ph=su.comma(c[1] for c in cameras))
    blocks = [dict(plasma_kappa_frac=0.4, plasma_kappa=4, plasma_w=1.5), dict(plasma_kappa_frac=0, plasma_kappa=4, plasma_w=1.5),
              dict(plasma_kappa_frac=1, plasma_kappa=4.5, plasma_w=1)]
    out = tmp_path / "sweep.npz"
    run = su.run_cli(su.write_input(tmp_path / "sweep.input", dict(params, output_file=str(out), **keys)), EXACT)
    assert "blacklight_amd: sweep of 3 variants per snapshot (3 polarized triples)" in run.stdout
    for c, (th, ph) in enumerate(cameras):
        for v, block in enumerate(blocks):
            single = tmp_path / f"single_{c}_{v}.npz"
            su.run_cli(su.write_input(tmp_path / f"single_{c}_{v}.input", dict(params, output_file=str(single), camera_th=th, camera_ph=ph, **block)), EXACT)
            assert su.file_bytes(_tagged(out, f"c{c:02d}v{v:02d}")) == su.file_bytes(single), (c, v)
