"""GPU: sweep_frequency in the .input file, rendered by bin/blacklight_amd in one render per snapshot - one context, one set of
geodesics - and written as one reference-layout file per (camera, frequency, variant): each ...cCCfFFmMMu00 file, byte for byte
(sweep_util.file_bytes: all but the ZIP headers' time stamps), the file of a run of its own with that camera's angles and that
frequency as its one image_frequency in the parameter block (the single runs sweep the two electron models, to bound the time: an
earlier suite holds their files to runs of their own). Exact tier. Every command-line run is a fresh child process with a time limit;
the runs with the key are made once for the module."""
import os

import pytest

import frequency_util as fu
import golden_util as gu
import sweep_util as su

pytestmark = pytest.mark.gpu

BANDS = [8.6e10, 2.3e11, 3.45e11]
CAMERAS = [(60.0, 30.0), (163.0, 275.0)]
PAIRS = [(1.0, 10.0), (2.0, 160.0)]   # (R_low, R_high)
EXACT = {"BLACKLIGHT_AMD_ARITHMETIC": "exact"}


@pytest.fixture(scope="module")
def swept(built_library, tmp_path_factory):
    directory = tmp_path_factory.mktemp("frequencies_cli")
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    grid_path = directory / "grid.blgrid"
    gu.golden_grid(mock_args).save_raw(grid_path)
    params = dict(params, simulation_file=str(grid_path), camera_resolution=16, output_camera="true")
    out = directory / "lib.npz"
    keys = dict(sweep_frequency=su.comma(BANDS), sweep_camera_th=su.comma(th for th, _ in CAMERAS), sweep_camera_ph=su.comma(ph for _, ph in CAMERAS),
                sweep_rat_low=su.comma(low for low, _ in PAIRS), sweep_rat_high=su.comma(high for _, high in PAIRS))
    run = su.run_cli(su.write_input(directory / "lib.input", dict(params, output_file=str(out), **keys)), EXACT, timeout=300)
    return directory, params, run


def test_one_process_writes_a_file_per_camera_frequency_and_model(swept):
    directory, params, run = swept
    assert "blacklight_amd: 3 frequencies per snapshot rendered over one set of geodesics, one file per frequency, camera and variant" in run.stdout
    assert "blacklight_amd: 2 cameras per snapshot traced as one set of rays" in run.stdout
    names = sorted(p for p in os.listdir(directory) if p.startswith("lib.") and p.endswith(".npz"))
    assert names == [f"lib.c{c:02d}f{f:02d}m{m:02d}u00.npz" for c in range(2) for f in range(3) for m in range(2)]   # exactly the twelve
    assert not (directory / "lib.npz").exists()


@pytest.mark.parametrize("camera", range(2))
def test_each_file_is_the_file_of_a_run_of_its_own(swept, camera):
    directory, params, run = swept
    th, ph = CAMERAS[camera]
    keys = dict(sweep_rat_low=su.comma(low for low, _ in PAIRS), sweep_rat_high=su.comma(high for _, high in PAIRS))
    for f, hz in enumerate(BANDS):
        single = directory / f"single_{camera}_{f}.npz"
        block = dict(fu.one_frequency(params, hz), output_file=str(single), camera_th=th, camera_ph=ph, **keys)
        su.run_cli(su.write_input(directory / f"single_{camera}_{f}.input", block), EXACT, timeout=300)
        for m in range(len(PAIRS)):
            assert su.file_bytes(directory / f"lib.c{camera:02d}f{f:02d}m{m:02d}u00.npz") == su.file_bytes(directory / f"single_{camera}_{f}.m{m:02d}u00.npz"), (camera, f, m)


def test_sweep_over_two_devices_writes_the_same_files(swept, tmp_path):
    """BLACKLIGHT_AMD_DEVICES = 2 (one GPU rehearses two: device d % present): the sweep is applied on every device, a device's share
    holds the rows of all frequencies and variants - the same twelve files as the one-device run."""
    directory, params, run = swept
    keys = dict(sweep_frequency=su.comma(BANDS), sweep_camera_th=su.comma(th for th, _ in CAMERAS), sweep_camera_ph=su.comma(ph for _, ph in CAMERAS),
                sweep_rat_low=su.comma(low for low, _ in PAIRS), sweep_rat_high=su.comma(high for _, high in PAIRS))
    su.run_cli(su.write_input(tmp_path / "lib.input", dict(params, output_file=str(tmp_path / "lib.npz"), **keys)), dict(EXACT, BLACKLIGHT_AMD_DEVICES="2"), timeout=300)
    names = sorted(p for p in os.listdir(tmp_path) if p.endswith(".npz"))
    assert names == [f"lib.c{c:02d}f{f:02d}m{m:02d}u00.npz" for c in range(2) for f in range(3) for m in range(2)]
    for name in names:
        assert su.file_bytes(tmp_path / name) == su.file_bytes(directory / name), name


def test_one_entry_still_writes_the_f00_file(built_library, tmp_path):
    """The sweep decides the names, not its length - and the bytes are the plain run's."""
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    grid_path = tmp_path / "grid.blgrid"
    gu.golden_grid(mock_args).save_raw(grid_path)
    params = dict(params, simulation_file=str(grid_path), camera_resolution=16)
    run = su.run_cli(su.write_input(tmp_path / "one.input", dict(params, output_file=str(tmp_path / "one.npz"), sweep_frequency=repr(BANDS[2]))), EXACT, timeout=300)
    assert "blacklight_amd: 1 frequencies per snapshot" in run.stdout and not (tmp_path / "one.npz").exists()
    su.run_cli(su.write_input(tmp_path / "plain.input", dict(fu.one_frequency(params, BANDS[2]), output_file=str(tmp_path / "plain.npz"))), EXACT, timeout=300)
    assert su.file_bytes(tmp_path / "one.f00.npz") == su.file_bytes(tmp_path / "plain.npz")


def test_a_polarized_block_writes_its_frequency_files(built_library, tmp_path):
    fx, params, mock_args = gu.load_case("sim_polarized")
    grid_path = tmp_path / "grid.blgrid"
    gu.golden_grid(mock_args).save_raw(grid_path)
    params = dict(params, simulation_file=str(grid_path), image_tau="true")
    su.run_cli(su.write_input(tmp_path / "pol.input", dict(params, output_file=str(tmp_path / "pol.npz"), sweep_frequency=su.comma(BANDS[:2]))), EXACT, timeout=300)
    assert sorted(p for p in os.listdir(tmp_path) if p.endswith(".npz")) == ["pol.f00.npz", "pol.f01.npz"]
    for f, hz in enumerate(BANDS[:2]):
        single = tmp_path / f"single_{f}.npz"
        su.run_cli(su.write_input(tmp_path / f"single_{f}.input", dict(fu.one_frequency(params, hz), output_file=str(single))), EXACT, timeout=300)
        assert su.file_bytes(tmp_path / f"pol.f{f:02d}.npz") == su.file_bytes(single), f
