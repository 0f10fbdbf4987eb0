"""GPU: a sweep written in the .input file, rendered by bin/blacklight_amd in one pass per snapshot and written as one
reference-layout file per variant - each file, byte for byte, the file of a run of its own with that variant in the parameter
block (exact tier: a variant's rows are documented as a fresh render's bits). "Byte for byte" is
sweep_util.file_bytes: every byte of the file except the wall-clock time stamps of a .npz's ZIP headers, which two writes of the
same arrays two seconds apart do not share. Every command-line run is a fresh child process with a time limit; a test stops at
the first one that fails."""
import json
import os
import re

import numpy as np
import pytest

import golden_util as gu
import sweep_util as su

pytestmark = pytest.mark.gpu

PAIRS_LOW, PAIRS_HIGH = [1.0, 1.0, 2.0], [10.0, 40.0, 160.0]
UNITS = [1.0e-16, 3.0e-16]
TRIPLES = [(1.0, 10.0, 1.0e-16), (1.0, 40.0, 2.0e-16), (2.0, 160.0, 4.0e-16)]
EXACT = {"BLACKLIGHT_AMD_ARITHMETIC": "exact"}
TOLERANT = {"BLACKLIGHT_AMD_ARITHMETIC": "tolerant"}
SUBNORMAL = 2.0 ** -1022


def _params_with_grid(case, directory, **overrides):
    fx, params, mock_args = gu.load_case(case)
    grid_path = directory / "grid.blgrid"
    if not grid_path.exists():
        gu.golden_grid(mock_args).save_raw(grid_path)
    return dict(params, simulation_file=str(grid_path), **overrides), mock_args


def _unpolarized_sweep_keys():
    return dict(sweep_rat_low=su.comma(PAIRS_LOW), sweep_rat_high=su.comma(PAIRS_HIGH), sweep_rho_cgs=su.comma(UNITS))


def _tagged(path, tag):
    stem, ext = os.path.splitext(str(path))
    return f"{stem}.{tag}{ext}"


def _sweep_against_single_runs(directory, params, sweep_keys, variants, tags, env):
    """One run with the sweep keys, then one run per variant with its values in the block; returns the sweep's files."""
    out = directory / "sweep.npz"
    run = su.run_cli(su.write_input(directory / "sweep.input", dict(params, output_file=str(out), **sweep_keys)), env)
    assert f"blacklight_amd: sweep of {len(variants)} variants per snapshot" in run.stdout
    files = [_tagged(out, tag) for tag in tags]
    for v, (low, high, rho) in enumerate(variants):
        single = directory / f"single_{v}.npz"
        su.run_cli(su.write_input(directory / f"single_{v}.input", dict(params, output_file=str(single), plasma_rat_low=low, plasma_rat_high=high,
                                                                       simulation_rho_cgs=rho)), env)
        assert su.file_bytes(files[v]) == su.file_bytes(single), (v, low, high, rho)
    assert not out.exists()
    return files


@pytest.fixture(scope="module")
def exact_three_by_two(built_library, tmp_path_factory):
    """The 3 x 2 unpolarized sweep of test 4 in the exact tier (two frequencies): its input's parameters and its six files."""
    directory = tmp_path_factory.mktemp("three_by_two")
    params, mock_args = _params_with_grid("sim_multifreq", directory, image_num_frequencies=2)
    variants = [(PAIRS_LOW[m], PAIRS_HIGH[m], UNITS[u]) for m in range(3) for u in range(2)]
    tags = [f"m{m:02d}u{u:02d}" for m in range(3) for u in range(2)]
    files = _sweep_against_single_runs(directory, params, _unpolarized_sweep_keys(), variants, tags, EXACT)
    return dict(directory=directory, params=params, mock_args=mock_args, files=files, variants=variants)


def test_unpolarized_three_by_two_equals_six_runs(exact_three_by_two):
    """Test 4, models x units: the fixture made the comparison; here, that the six files are six different images."""
    images = [np.load(f)["I_nu"] for f in exact_three_by_two["files"]]
    assert images[0].shape == (2, 16, 16)
    for a in range(6):
        for b in range(a + 1, 6):
            assert not np.array_equal(images[a], images[b], equal_nan=True), (a, b)


def test_polarized_triples_in_one_pass_equal_three_runs(built_library, tmp_path):
    """Stokes rows and the optical-depth row only: the one pass of DESIGN 4d (launches_shade == n_chunks, seen on the Context route)."""
    import blacklight_amd as bl
    params, mock_args = _params_with_grid("sim_polarized", tmp_path)
    keys = dict(sweep_rat_low=su.comma(t[0] for t in TRIPLES), sweep_rat_high=su.comma(t[1] for t in TRIPLES), sweep_rho_cgs=su.comma(t[2] for t in TRIPLES))
    files = _sweep_against_single_runs(tmp_path, params, keys, TRIPLES, [f"v{v:02d}" for v in range(3)], EXACT)
    path = su.write_input(tmp_path / "context.input", dict(params, output_file=str(tmp_path / "context.npz"), **keys))
    with bl.Context.from_input(path) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(mock_args))
        got = ctx.render()
        assert got["stats"].launches_shade == got["stats"].n_chunks and ctx.num_variants == 3
        for v in range(3):
            ctx.write_output([dict(got, block_locs=None)], variant=v)
            assert su.file_bytes(ctx.variant_output_path(0, v)) == su.file_bytes(files[v]), v


def test_per_variant_passes_equal_single_runs(built_library, tmp_path):
    """An auxiliary row (image_time) sends the polarized planner through one shading pass per variant."""
    import blacklight_amd as bl
    params, mock_args = _params_with_grid("sim_polarized", tmp_path, image_time="true")
    keys = dict(sweep_rat_low=su.comma(t[0] for t in TRIPLES), sweep_rat_high=su.comma(t[1] for t in TRIPLES), sweep_rho_cgs=su.comma(t[2] for t in TRIPLES))
    _sweep_against_single_runs(tmp_path, params, keys, TRIPLES, [f"v{v:02d}" for v in range(3)], EXACT)
    with bl.Context.from_input(su.write_input(tmp_path / "context.input", dict(params, **keys))) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(mock_args))
        st = ctx.render()["stats"]
        assert st.launches_shade == 3 * st.n_chunks   # (that this case is what its name says)


def test_series_with_a_sweep_names_and_reuses(built_library, tmp_path):
    """Test 5: two .athdf snapshots x (2 pairs x 2 units): 2 x 4 files, each the single run's file for that snapshot."""
    reader_dir = os.path.join(gu.GOLDEN_DIR, "reader")
    expected = np.load(os.path.join(reader_dir, "expected.npz"), allow_pickle=False)
    params = json.loads(str(expected["series_params"]))
    params["simulation_file"] = os.path.join(reader_dir, "series_{04d}.athdf")
    pairs, units = [(1.0, 10.0), (2.0, 80.0)], [1.0e-16, 2.5e-16]
    out = tmp_path / "image_{02d}.npz"
    keys = dict(sweep_rat_low=su.comma(p[0] for p in pairs), sweep_rat_high=su.comma(p[1] for p in pairs), sweep_rho_cgs=su.comma(units))
    run = su.run_cli(su.write_input(tmp_path / "series.input", dict(params, output_file=str(out), **keys)), EXACT)
    assert "geodesics integrated once for the series" in run.stdout
    assert "blacklight_amd: sweep of 4 variants per snapshot (2 electron models x 2 density units)" in run.stdout
    for m, (low, high) in enumerate(pairs):
        for u, rho in enumerate(units):
            single = tmp_path / f"single_m{m}u{u}" / "image_{02d}.npz"
            os.makedirs(single.parent)
            su.run_cli(su.write_input(tmp_path / f"single_m{m}u{u}.input", dict(params, output_file=str(single), plasma_rat_low=low, plasma_rat_high=high,
                                                                              simulation_rho_cgs=rho)), EXACT)
            for number in (3, 4):
                got = tmp_path / f"image_{number:02d}.m{m:02d}u{u:02d}.npz"
                assert su.file_bytes(got) == su.file_bytes(single.parent / f"image_{number:02d}.npz"), (m, u, number)
    assert sorted(os.path.basename(p) for p in os.listdir(tmp_path) if p.endswith(".npz")) == \
        sorted(f"image_{n:02d}.m{m:02d}u{u:02d}.npz" for n in (3, 4) for m in range(2) for u in range(2))
    # the block's own variant is the golden series: (R_low, R_high, unit) = (1, 10, 1e-16) is what the reference rendered
    for number in (3, 4):
        got = np.load(tmp_path / f"image_{number:02d}.m00u00.npz")
        assert gu.same_bits(got["I_nu"], expected[f"series_B_{number}_I_nu"]).all()


def test_tolerant_tier_files_lie_within_the_tier_of_the_exact_files(exact_three_by_two, tmp_path):
    """Test 6: the default tier's six files against the exact tier's, per pixel relative to the pixel's own intensity: the same NaN
    mask and |I - I_exact| <= max(1e-10 |I_exact|, 2^-1022 nu^3) (README, tests/test_gpu_variant_edges.py); every other record equal."""
    out = tmp_path / "sweep.npz"
    su.run_cli(su.write_input(tmp_path / "sweep.input", dict(exact_three_by_two["params"], output_file=str(out), **_unpolarized_sweep_keys())), TOLERANT)
    worst = 0.0
    for exact_file in exact_three_by_two["files"]:
        want, got = np.load(exact_file), np.load(tmp_path / os.path.basename(exact_file))
        assert want.files == got.files
        for name in want.files:
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            if name != "I_nu":
                assert got[name].tobytes() == want[name].tobytes(), name   # mass_msun, width, frequency, adaptive_num_levels
        a, b = got["I_nu"].reshape(2, -1), want["I_nu"].reshape(2, -1)
        nu3 = want["frequency"][:, None] ** 3
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isfinite(a), np.isfinite(b))
        finite = np.isfinite(b)
        err = np.abs(a - b)[finite]
        tol = np.maximum(1.0e-10 * np.abs(b), SUBNORMAL * nu3)[finite]
        worst = max(worst, float(np.max(err / tol)))
        print(os.path.basename(exact_file), "max |I - I_exact| / bound =", float(np.max(err / tol)))
        assert np.all(err <= tol), float(np.max(err / tol))
    print("worst over the six files:", worst)


def test_context_route_writes_the_command_lines_files(exact_three_by_two, tmp_path):
    """Test 7: Context.from_input -> render() -> write_output(variant=v)."""
    import blacklight_amd as bl
    path = su.write_input(tmp_path / "context.input", dict(exact_three_by_two["params"], output_file=str(tmp_path / "context.npz"), **_unpolarized_sweep_keys()))
    with bl.Context.from_input(path) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(exact_three_by_two["mock_args"]))
        got = ctx.render()
        assert ctx.num_variants == 6 and got["image"].shape[0] == 6 * 2
        for v, cli_file in enumerate(exact_three_by_two["files"]):
            ctx.write_output([dict(got, block_locs=None)], variant=v)
            assert os.path.basename(ctx.variant_output_path(0, v)) == os.path.basename(cli_file).replace("sweep", "context")
            assert su.file_bytes(ctx.variant_output_path(0, v)) == su.file_bytes(cli_file), v


def test_sweep_over_two_devices_writes_the_same_files(exact_three_by_two, tmp_path):
    """BLACKLIGHT_AMD_DEVICES = 2 (one GPU rehearses two: device d % present): a device's share holds the rows of all variants, so
    the sweep falls out of the row layout - the same files as the one-device run."""
    out = tmp_path / "sweep.npz"
    su.run_cli(su.write_input(tmp_path / "sweep.input", dict(exact_three_by_two["params"], output_file=str(out), **_unpolarized_sweep_keys())),
               dict(EXACT, BLACKLIGHT_AMD_DEVICES="2"))
    for one_device in exact_three_by_two["files"]:
        assert su.file_bytes(tmp_path / os.path.basename(one_device)) == su.file_bytes(one_device), one_device


def test_stdout_without_sweep_keys_is_what_it_was(exact_three_by_two, tmp_path):
    """A run without sweep keys prints the lines it printed before the keys existed, and no other (times masked); a run with them, one more."""
    params = exact_three_by_two["params"]
    plain = su.run_cli(su.write_input(tmp_path / "plain.input", dict(params, output_file=str(tmp_path / "plain.npz"))), EXACT)
    number = r"[0-9.e+-]+"
    block = ("\nCalculation completed.\nElapsed time:            N s\n  Integrating geodesics: N s\n  Reading simulation:    N s\n"
             "  Sampling simulation:   N s\n  Integrating image:     N s\n  Rendering:             N s\n\n"
             "blacklight_amd: exact arithmetic tier (BLACKLIGHT_AMD_ARITHMETIC=exact|tolerant)\n")
    assert re.sub(number + " s\n", "N s\n", plain.stdout) == block
    swept = su.run_cli(su.write_input(tmp_path / "swept.input", dict(params, output_file=str(tmp_path / "swept.npz"), **_unpolarized_sweep_keys())), EXACT)
    line = "blacklight_amd: sweep of 6 variants per snapshot (3 electron models x 2 density units), one file each; writing outputs: N s\n"
    assert re.sub(number + " s\n", "N s\n", swept.stdout) == block + line


def test_command_line_errors_of_a_sweep(built_library, tmp_path):
    """Error: ... on stdout, exit status 1: the parser's texts and a setter's refusal (formula mode)."""
    import subprocess
    fx, params, _ = gu.load_case("formula_flat")
    cases = [(dict(sweep_rat_low="1,1", sweep_rat_high="10"), "Error: sweep_rat_low and sweep_rat_high must have the same number of entries (2 and 1) in input file.\n"),
             (dict(sweep_rho_cgs="1e-16,,"), "Error: Empty entry in list (sweep_rho_cgs) in input file.\n")]
    for keys, message in cases:
        run = subprocess.run([su.EXE, su.write_input(tmp_path / "bad.input", dict(params, output_file=str(tmp_path / "x.npz"), **keys))],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 1 and run.stdout == message, run.stdout + run.stderr
    run = subprocess.run([su.EXE, su.write_input(tmp_path / "formula.input", dict(params, output_file=str(tmp_path / "x.npz"), sweep_rho_cgs="1e-16,2e-16"))],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and run.stdout == "Error: Density units: formula mode has no density (model_type = formula).\n", run.stdout + run.stderr
