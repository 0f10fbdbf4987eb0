"""GPU: sweep_cut_sigma_max in the .input file, rendered by bin/blacklight_amd in one pass per snapshot and written as one
reference-layout file per variant - each ...sNN file, byte for byte (sweep_util.file_bytes: all but the ZIP headers' time stamps), the
file of a run of its own with that cut_sigma_max (and pair, and unit) in the parameter block. Exact tier: a variant's rows are a fresh
render's bits. Every command-line run is a fresh child process with a time limit; a test stops at the first one that fails."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import sweep_util as su

pytestmark = pytest.mark.gpu

CUTS = [0.01, 0.1, 1.0, 10.0, -1.0]
EXACT = {"BLACKLIGHT_AMD_ARITHMETIC": "exact"}


def _params_with_grid(case, directory, **overrides):
    fx, params, mock_args = gu.load_case(case)
    grid_path = directory / "grid.blgrid"
    if not grid_path.exists():
        gu.golden_grid(mock_args).save_raw(grid_path)
    return dict(params, simulation_file=str(grid_path), **overrides)


def _tagged(path, tag):
    stem, ext = os.path.splitext(str(path))
    return f"{stem}.{tag}{ext}"


def test_cuts_alone_equal_runs_of_their_own(built_library, tmp_path):
    params = _params_with_grid("sim_multifreq", tmp_path, image_num_frequencies=2)
    out = tmp_path / "sweep.npz"
    run = su.run_cli(su.write_input(tmp_path / "sweep.input", dict(params, output_file=str(out), sweep_cut_sigma_max=su.comma(CUTS))), EXACT)
    assert "blacklight_amd: sweep of 5 variants per snapshot (1 electron models x 1 density units x 5 sigma cuts), one file each" in run.stdout
    images = []
    for s, cut in enumerate(CUTS):
        single = tmp_path / f"single_{s}.npz"
        su.run_cli(su.write_input(tmp_path / f"single_{s}.input", dict(params, output_file=str(single), cut_sigma_max=cut)), EXACT)
        assert su.file_bytes(_tagged(out, f"m00u00s{s:02d}")) == su.file_bytes(single), (s, cut)
        images.append(np.load(single)["I_nu"])
    assert not out.exists()
    for s in range(len(CUTS) - 1):   # five different images
        assert not np.array_equal(images[s], images[s + 1], equal_nan=True), s


def test_cuts_beside_models_and_units_equal_runs_of_their_own(built_library, tmp_path):
    pairs, units, cuts = [(1.0, 10.0), (2.0, 80.0)], [1.0e-16, 2.5e-16], [0.1, 1.0, -1.0]
    params = _params_with_grid("sim_multifreq", tmp_path, image_num_frequencies=2)
    out = tmp_path / "sweep.npz"
    keys = dict(sweep_rat_low=su.comma(p[0] for p in pairs), sweep_rat_high=su.comma(p[1] for p in pairs), sweep_rho_cgs=su.comma(units),
                sweep_cut_sigma_max=su.comma(cuts))
    run = su.run_cli(su.write_input(tmp_path / "sweep.input", dict(params, output_file=str(out), **keys)), EXACT)
    assert "blacklight_amd: sweep of 12 variants per snapshot (2 electron models x 2 density units x 3 sigma cuts), one file each" in run.stdout
    for m, (low, high) in enumerate(pairs):
        for u, rho in enumerate(units):
            for s, cut in enumerate(cuts):
                single = tmp_path / f"single_{m}{u}{s}.npz"
                su.run_cli(su.write_input(tmp_path / f"single_{m}{u}{s}.input", dict(params, output_file=str(single), plasma_rat_low=low, plasma_rat_high=high,
                                                                                  simulation_rho_cgs=rho, cut_sigma_max=cut)), EXACT)
                assert su.file_bytes(_tagged(out, f"m{m:02d}u{u:02d}s{s:02d}")) == su.file_bytes(single), (m, u, s)
    assert sorted(p for p in os.listdir(tmp_path) if p.startswith("sweep.") and p.endswith(".npz")) == \
        sorted(f"sweep.m{m:02d}u{u:02d}s{s:02d}.npz" for m in range(2) for u in range(2) for s in range(3))


def test_a_polarized_input_with_the_key_is_refused(built_library, tmp_path):
    params = _params_with_grid("sim_polarized", tmp_path)
    run = subprocess.run([su.EXE, su.write_input(tmp_path / "pol.input", dict(params, output_file=str(tmp_path / "x.npz"), sweep_cut_sigma_max="1,3"))],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 1, run.stdout + run.stderr
    assert run.stdout == "Error: Sigma cuts: the polarized axis is not built yet; polarized runs render one sigma cut (image_polarization = true).\n"
