"""Every optional cut alone, on the CPU: the oracle against tests/golden/cut_each.npz - the stock reference's 16^2 image over the small
mock with one of the 23 optional cuts switched on per case (fourteen cell thresholds, simulation_coefficients.cpp:361-374; nine
geometric settings, simulation_sampling.cpp:246-292, formula_coefficients.cpp:78-116) - and the threshold edges on the oracle alone.
tests/test_gpu_cuts_each.py holds the device to the oracle on the same cases, so what is pinned here is what it rests on:

  * the oracle built on host libm equals the recording bit for bit (image, sample_num, flags) on a host of the class that generated it,
    and stays inside tests/test_oracle_golden.py's envelope elsewhere;
  * the pinned-math oracle is within the project's tier-A bound, 1e-6 of the image maximum with equal sample_num, where a = 0;
  * each cut alone leaves between 0.05 and 0.95 of the flux of the frame without a cut - a condition, not a measurement: a case outside
    it says nothing about its cut - and its frame is not the frame without a cut;
  * thresholds of 0.0 and -0.0 are active (`cut >= 0.0`), a threshold that a sample equals does not cut it (strict comparisons), and
    the edges of the geometric settings; stated here so that the GPU edge test is known to compare against something that bites;
  * the seeds of the randomised GPU test are the first sixteen whose cuts leave light, with at most four replaced.

No formula-mode case with cut_midplane_theta or cut_midplane_z is recorded - the stock reference ends in a segmentation fault there
(cut_cases.UNRECORDED) - so those two are held to the flux share on the oracle only."""
import numpy as np
import pytest

import cut_cases as cc
import golden_util as gu
from test_oracle_golden import _generating_host_class

TIER_A = 1.0e-6   # the project's tier-A bound: per-pixel L-infinity relative to the image maximum (tests/test_gpu_parity.py)


def test_the_fixture_holds_every_cut():
    names = list(cc.RECORDED)
    assert names[0] == "sim_none" and "formula_none" in names
    for key in cc.CELL_THRESHOLDS:   # each alone: the only cut of its case, every other threshold off
        params = cc.RECORDED[key]["params"]
        assert float(params[key]) > 0.0
        assert all(float(params[other]) == -1.0 for other in cc.CELL_THRESHOLDS if other != key)
    geometric = [n for n in names if cc.geometric(n) and not n.startswith(("formula_", "spin_"))]
    assert geometric == ["cut_omit_near", "cut_omit_far", "cut_omit_in", "cut_omit_out", "cut_midplane_theta_pos", "cut_midplane_theta_neg",
                         "cut_midplane_z_pos", "cut_midplane_z_neg", "cut_plane"]
    assert float(cc.RECORDED["cut_midplane_theta_pos"]["params"]["cut_midplane_theta"]) > 0.0 > float(cc.RECORDED["cut_midplane_theta_neg"]["params"]["cut_midplane_theta"])
    assert float(cc.RECORDED["cut_midplane_z_pos"]["params"]["cut_midplane_z"]) > 0.0 > float(cc.RECORDED["cut_midplane_z_neg"]["params"]["cut_midplane_z"])
    for name in names:
        params = cc.RECORDED[name]["params"]
        assert int(params["camera_resolution"]) == 16 and cc.RECORDED[name]["I_nu"].shape == (256,)
        if params["model_type"] == "simulation" and name != "cut_sigma_max":
            assert float(params["cut_sigma_max"]) == -1.0
        assert float(params.get("simulation_a", 0.0)) == (0.5 if name.startswith("spin_") else 0.0)
    # (what the existing per-case tests parametrise over does not pick the file up)
    assert not any(c.startswith("cut_") for c in gu.CASES)


@pytest.mark.parametrize("name", list(cc.RECORDED))
def test_libm_oracle_equals_the_recording(name, built_library):
    want = cc.RECORDED[name]
    out = cc.oracle_case(name, variant="libm")
    assert out["image"].shape == (1, 256)
    if _generating_host_class():
        assert np.array_equal(out["sample_num"], want["sample_num"])
        assert np.array_equal(out["sample_flags"], want["sample_flags"])
        assert gu.same_bits(out["image"][0], want["I_nu"]).all()
    else:   # another libm build: tests/test_oracle_golden.py's envelope
        assert np.mean(out["sample_num"] == want["sample_num"]) > 0.95
        finite = np.isfinite(want["I_nu"]) & np.isfinite(out["image"][0])
        assert np.max(np.abs(out["image"][0] - want["I_nu"])[finite]) / np.nanmax(np.abs(want["I_nu"])) < 1e-5


@pytest.mark.parametrize("name", [n for n in cc.RECORDED if not cc.spinning(n)])
def test_pinned_math_oracle_within_tier_a(name, built_library):
    want = cc.RECORDED[name]
    out = cc.oracle_case(name)
    assert np.array_equal(out["sample_num"], want["sample_num"]) and np.array_equal(out["sample_flags"], want["sample_flags"])
    assert np.array_equal(np.isnan(out["image"][0]), np.isnan(want["I_nu"]))
    distance = float(np.nanmax(np.abs(out["image"][0] - want["I_nu"])) / np.nanmax(np.abs(want["I_nu"])))
    print(f"{name}: pinned math vs stock reference {distance:.2e}")
    assert distance < TIER_A


@pytest.mark.parametrize("name", [n for n in cc.ALL_CASES if not n.endswith("_none")])
def test_each_cut_takes_a_share_of_the_flux(name, built_library):
    whole = cc.oracle_case(cc.baseline(name))["image"]
    image = cc.oracle_case(name)["image"]
    assert np.nansum(whole[0]) > 0.0 and not np.isnan(image).any()
    left = cc.share(image, whole)
    print(f"{name}: {left:.3f} of the flux left")
    assert cc.SHARE[0] <= left <= cc.SHARE[1]
    assert not gu.same_bits(image, whole).all()
    if name in cc.RECORDED:   # ... and the recording says the same of itself
        recorded = float(cc.RECORDED[name]["I_nu"].sum() / cc.RECORDED[cc.baseline(name)]["I_nu"].sum())
        assert cc.SHARE[0] <= recorded <= cc.SHARE[1]
        assert not gu.same_bits(cc.RECORDED[name]["I_nu"], cc.RECORDED[cc.baseline(name)]["I_nu"]).all()


@pytest.mark.parametrize("edge", list(cc.edge_cases()))
def test_threshold_edges_on_the_oracle(edge, built_library):
    overrides, expected = cc.edge_cases()[edge]
    none = cc.oracle_case("sim_none")
    assert np.nanmax(none["image"]) > 0.0 and (none["image"] > 0.0).sum() > 128   # (not vacuous: there is light to cut)
    out = cc.oracle(*cc.edge_inputs(overrides))
    assert np.array_equal(out["sample_num"], none["sample_num"]) and np.array_equal(out["sample_flags"], none["sample_flags"])
    if expected == "none":
        assert gu.same_bits(out["image"], none["image"]).all()
    else:
        assert expected == "zero" and (out["image"] == 0.0).all()
    # a threshold of -1.0 in the same place is not active
    off = {key: -1.0 for key, value in overrides.items() if isinstance(value, float)}
    if off:
        assert gu.same_bits(cc.oracle(*cc.edge_inputs(off))["image"], none["image"]).all()


def test_negative_zero_reaches_the_parameter_block(built_library):
    """-0.0 is written as "-0.0" and stored with its sign: the edge cases above do test a negative zero."""
    import blacklight_amd as bl
    params, _ = cc.edge_inputs(dict(cut_rho_max=-0.0, cut_omit_out=-0.0))
    p = bl.Params.from_dict(params)
    for key in ("cut_rho_max", "cut_omit_out"):
        assert p.get(key) == 0.0 and np.signbit(p.get(key))


def test_a_threshold_that_a_sample_equals(built_library):
    cases = cc.equality_cases()
    assert sorted(cases) == ["rho_max_equal", "rho_min_equal", "rho_min_max_equal"]
    nearest = cc.oracle(*cc.edge_inputs(dict(simulation_interp="false")))
    for name, (at, beside) in cases.items():
        here = cc.oracle(*cc.edge_inputs(at))["image"]
        there = cc.oracle(*cc.edge_inputs(beside))["image"]
        print(f"{name}: {at} leaves {cc.share(here, nearest['image']):.4f}, its neighbour {cc.share(there, nearest['image']):.4f}")
        assert np.nanmax(here) > 0.0
        assert not gu.same_bits(here, there).all()                 # (the neighbouring double cuts the samples that equal the threshold)
        assert np.nansum(there[0]) < np.nansum(here[0])
        assert not gu.same_bits(here, nearest["image"]).all()    # (and the threshold itself cuts something)
    # both thresholds on one value: what is left is that cell's samples alone, and nothing beside it
    assert (cc.oracle(*cc.edge_inputs(cases["rho_min_max_equal"][1]))["image"] == 0.0).all()


def test_the_seeds_of_the_randomised_draws(built_library):
    """A rejected draw (no positive pixel on the oracle) is replaced with the next seed; at most four of sixteen may be."""
    kept, seed = [], 0
    while len(kept) < cc.N_DRAWS:
        assert seed < cc.N_DRAWS + cc.MAX_REPLACED, "more than four draws replaced"
        if cc.accepted(seed):
            kept.append(seed)
        seed += 1
    assert kept == cc.RANDOM_SEEDS
    # (the kept draws spread over the table: at least half of its 21 keys appear)
    drawn = set()
    for s in cc.RANDOM_SEEDS:
        params, _ = cc.random_configuration(s)
        none = cc.RECORDED["sim_none"]["params"]
        drawn |= {k for k in params if k.startswith("cut_") and not k.startswith("cut_plane_") and params[k] != none.get(k)}
    assert len(drawn) >= 12, sorted(drawn)
