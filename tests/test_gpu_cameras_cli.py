"""GPU: sweep_camera_th / sweep_camera_ph in the .input file, rendered by bin/blacklight_amd as one set of rays per snapshot - one
context, one read of the snapshot - and written as one reference-layout file per (camera, variant): each ...cCCmMMuUU file, byte for
byte (sweep_util.file_bytes: all but the ZIP headers' time stamps), the file of a run of its own with that camera's angles and that
model in the parameter block. Exact tier. Every command-line run is a fresh child process with a time limit; the run with the keys
is made once for the module."""
import os

import pytest

import golden_util as gu
import sweep_util as su

pytestmark = pytest.mark.gpu

CAMERAS = [(0.0, 0.0), (60.0, 30.0), (163.0, 275.0)]
PAIRS = [(1.0, 10.0), (2.0, 160.0)]   # (R_low, R_high)
EXACT = {"BLACKLIGHT_AMD_ARITHMETIC": "exact"}


@pytest.fixture(scope="module")
def swept(built_library, tmp_path_factory):
    directory = tmp_path_factory.mktemp("cameras_cli")
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    grid_path = directory / "grid.blgrid"
    gu.golden_grid(mock_args).save_raw(grid_path)
    params = dict(params, simulation_file=str(grid_path), camera_resolution=16, output_camera="true")
    out = directory / "lib.npz"
    keys = dict(sweep_camera_th=su.comma(th for th, _ in CAMERAS), sweep_camera_ph=su.comma(ph for _, ph in CAMERAS),
                sweep_rat_low=su.comma(low for low, _ in PAIRS), sweep_rat_high=su.comma(high for _, high in PAIRS))
    run = su.run_cli(su.write_input(directory / "lib.input", dict(params, output_file=str(out), **keys)), EXACT, timeout=300)
    return directory, params, run


def test_one_process_writes_a_file_per_camera_and_model(swept):
    directory, params, run = swept
    assert "blacklight_amd: 3 cameras per snapshot traced as one set of rays, one file per camera and variant" in run.stdout
    assert "blacklight_amd: sweep of 2 variants per snapshot (2 electron models x 1 density units), one file each" in run.stdout
    names = sorted(p for p in os.listdir(directory) if p.startswith("lib.") and p.endswith(".npz"))
    assert names == [f"lib.c{c:02d}m{m:02d}u00.npz" for c in range(3) for m in range(2)]   # the names sort in (camera, variant) order
    assert not (directory / "lib.npz").exists()


@pytest.mark.parametrize("camera", range(3))
def test_each_file_is_the_file_of_a_run_of_its_own(swept, camera):
    directory, params, run = swept
    th, ph = CAMERAS[camera]
    for m, (low, high) in enumerate(PAIRS):
        single = directory / f"single_{camera}_{m}.npz"
        su.run_cli(su.write_input(directory / f"single_{camera}_{m}.input", dict(params, output_file=str(single), camera_th=th, camera_ph=ph,
                                                                              plasma_rat_low=low, plasma_rat_high=high)), EXACT, timeout=300)
        assert su.file_bytes(directory / f"lib.c{camera:02d}m{m:02d}u00.npz") == su.file_bytes(single), (camera, m)
