"""The formula_ctl_* goldens (tools/make_goldens.py CONTROLLER_CASES) hold the branches of the Dormand-Prince step controller they are
there for (reference geodesics.cpp:136-224). Read straight from the committed files - the reference's own sample_num and sample_flags with
the pinned math library, and the ray_max_steps it ran with - so that a regenerated fixture which no longer reaches a branch fails here
and not silently in the comparisons that use it (tests/test_oracle_golden.py, tests/test_gpu_parity.py, tests/test_gpu_controller.py).

A ray that exhausts its retries (num_retry > ray_max_retries, geodesics.cpp:139-143) is one that ends flagged short of ray_max_steps; a
ray flagged with ray_max_steps samples ran out of steps instead.

The twelfth case of the table, zero spin with ray_step = 0.3, tolerances of 1e-12 and ray_max_retries = 1, has no file: every ray
exhausts its retries on its first step, and the reference, left with geodesic_num_steps = 0, stops with "Attempting to allocate empty
array." after its warning (geodesics.cpp:814, utils/array.cpp:163; the generator makes that run and expects that end). What the case
is there for is held to the CPU oracle here: only flagged rays, none with a sample."""
import numpy as np
import pytest

import golden_util as gu

CTL = [c for c in gu.CASES if c.startswith("formula_ctl_")]
# the reference's counts when the fixtures were made (the assertion is > 0; these are printed next to what the file holds)
RETRY_ROWS = {"formula_ctl_tol3": 1, "formula_ctl_retry1": 22, "formula_ctl_retry1_tol12": 15, "formula_ctl_retry2_tol13": 9}
NO_SAMPLE_FRAME = dict(formula_spin=0.0, ray_step=0.3, ray_tol_abs=1.0e-12, ray_tol_rel=1.0e-12, ray_max_retries=1)


def _counts(case):
    fx, params, _ = gu.load_case(case)
    num, flagged = fx["B_sample_num"], fx["B_sample_flags"] != 0
    assert num.shape == flagged.shape == (256,) and int(params["camera_resolution"]) == 16
    return fx, params, num, flagged, flagged & (num < int(params["ray_max_steps"]))


def test_the_eleven_files_are_there():
    assert CTL == sorted(["formula_ctl_tol3", "formula_ctl_tol12", "formula_ctl_abs9", "formula_ctl_rel9", "formula_ctl_retry1",
                          "formula_ctl_retry1_tol12", "formula_ctl_retry2_tol13", "formula_ctl_step03", "formula_ctl_step03_tol4",
                          "formula_ctl_a0_tol3", "formula_ctl_a0_retry2"])
    for case in CTL:
        fx, params, _ = gu.load_case(case)
        assert len(str(fx["controller_note"])) > 20 and params["model_type"] == "formula" and params["ray_integrator"] == "dp"


@pytest.mark.parametrize("case", sorted(RETRY_ROWS))
def test_retry_rows_hold_rays_that_exhaust_their_retries(case):
    fx, params, num, flagged, exhausted = _counts(case)
    print(f"{case}: {int(flagged.sum())} flagged, {int(exhausted.sum())} of them short of ray_max_steps = {params['ray_max_steps']} (when made: {RETRY_ROWS[case]})")
    assert exhausted.sum() > 0
    ray = int(fx["dump_rays"][0])   # the dumped ray is one of them, with the samples it had when it gave up
    assert exhausted[ray] and fx[f"B_ray{ray}_pos"].shape == (num[ray], 4)


def test_zero_spin_with_two_retries_has_no_flag_and_samples_everywhere():
    fx, params, num, flagged, exhausted = _counts("formula_ctl_a0_retry2")
    assert float(params["formula_spin"]) == 0.0 and int(params["ray_max_retries"]) == 2
    assert not flagged.any() and (num > 0).all()


def test_zero_spin_with_one_retry_leaves_no_sample(built_library):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    import oracle_api
    fx, params, _ = gu.load_case("formula_ctl_a0_retry2")
    params = dict(params, **NO_SAMPLE_FRAME)
    p = bl.Params.from_dict(params)
    out = oracle_api.render(p.ptr, None, _capi.RenderDesc, _capi.CameraFrame, n_rays=256, max_steps=int(params["ray_max_steps"]))
    assert (out["sample_flags"] != 0).all() and (out["sample_num"] == 0).all()
    assert np.isfinite(out["image"]).all()


def test_long_steps_with_loose_tolerances_give_short_rays():
    fx, params, num, flagged, exhausted = _counts("formula_ctl_step03_tol4")
    print(f"formula_ctl_step03_tol4: max sample_num {int(num.max())}, {int(num.sum())} samples")
    assert num.max() < 200 and not flagged.any()


@pytest.mark.parametrize("case", ["formula_ctl_tol12", "formula_ctl_a0_retry2"])
def test_tight_tolerances_without_a_retry_limit_that_bites_have_no_flag(case):
    fx, params, num, flagged, exhausted = _counts(case)
    assert float(params["ray_tol_abs"]) == float(params["ray_tol_rel"]) == 1.0e-12
    assert not flagged.any()
