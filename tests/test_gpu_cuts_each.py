"""GPU: every optional cut alone, in both arithmetic tiers, against the CPU oracle - which tests/test_cuts_each_host.py pins to the stock
reference's recording of the same cases (tests/golden/cut_each.npz). The decisions are spread over optional_cuts() (bl_locate.hip in
simulation mode, bl_shade.hip in formula mode), the cell-cut compare against +-inf thresholds (bl_sampling.h), the tolerant tier's
folded thresholds and guard band (FoldFastCuts), the two cut forms of bl_shade_fused2_kernel, and the plan (GeometricCut() takes the
locate step out of every coefficient kernel and keeps formula mode out of the tolerant tier): one cut per case, so that a wrong sign or
a swapped pair in one cannot hide behind another.

Which path a case takes is asserted through bl_stats, from the plan in bl_render.hip (PlanJob): the small mock is one block with evenly
spaced faces, so without a geometric cut the tolerant tier runs bl_shade_fused2_kernel (fused_variant 2) and the exact tier
bl_shade_exact2_kernel (3), both with the locate step inside (launches_locate 0); a geometric cut sends both through the locate kernel
(fused_variant 0, one launch per chunk), the tolerant tier still in its own arithmetic (bl_shade_fast_kernel); formula mode with a
geometric cut is rendered in exact arithmetic whatever was asked for.

Frames are 16^2 over the 32 x 24 x 32 mock; every oracle frame is computed once per session (cut_cases.oracle)."""
import numpy as np
import pytest
import torch   # noqa: F401  (before the library: see tests/test_gpu_defaults.py)

import cut_cases as cc
import golden_util as gu
from test_gpu_fused_loop import PER_PIXEL, _relative_per_pixel
from test_gpu_tolerant import EXPECTED, _distance

pytestmark = pytest.mark.gpu

TIER_A = 1.0e-6   # against the stock reference's recording, a = 0: per-pixel L-infinity relative to the image maximum


def _context(params, mock_args):
    import blacklight_amd as bl
    ctx = bl.Context(bl.Params.from_dict(params))
    if mock_args is not None:
        ctx.set_grid(cc.grid_of(mock_args))
    return ctx


def _both(params, mock_args, more=None):
    """The exact tier's frame, then the tolerant tier's, from one context; more(ctx, out) may render further frames."""
    out = {}
    with _context(params, mock_args) as ctx:
        ctx.set_arithmetic("exact")
        out["exact"] = ctx.render()
        ctx.set_arithmetic("tolerant")
        out["tolerant"] = ctx.render()
        if more is not None:
            more(ctx, out)
    return out


def _exact_is_the_oracle(exact, want):
    assert exact["stats"].arithmetic == 0
    assert np.array_equal(exact["sample_num"], want["sample_num"])
    assert np.array_equal(exact["sample_flags"], want["sample_flags"])
    assert exact["image"].shape == want["image"].shape
    same = gu.same_bits(exact["image"], want["image"])
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ from the oracle"


def _tolerant_within_its_bound(tol, exact):
    """Counts, flags and NaN mask of the exact tier; the fused kernel within its per-pixel bound, every other tolerant kernel within
    the tier's bound relative to the row maximum. Returns the distance it asserted."""
    assert np.array_equal(tol["sample_num"], exact["sample_num"])
    assert np.array_equal(tol["sample_flags"], exact["sample_flags"])
    assert np.array_equal(np.isnan(tol["image"]), np.isnan(exact["image"]))
    if tol["stats"].fused_variant == 2:
        distance = _relative_per_pixel(tol, exact)
        assert distance <= PER_PIXEL
    else:
        distance = _distance(tol["image"], exact["image"])
        assert distance < EXPECTED
    return distance


@pytest.mark.parametrize("name", cc.ALL_CASES)
def test_each_cut_alone(name, built_library):
    params, mock_args = cc.inputs(name)
    simulation = params["model_type"] == "simulation"
    threshold = name in cc.CELL_THRESHOLDS

    def more(ctx, out):   # the general cut block under bl_set_reproducible, and every decision left to the exact pass
        ctx.set_reproducible(True)
        ctx.debug_set_switches("GENERAL_CUTS")
        out["general"] = ctx.render()
        ctx.set_reproducible(False)
        ctx.debug_set_switches()
        ctx.debug_set_guard_band(1.0e30)
        out["wide"] = ctx.render()

    out = _both(params, mock_args, more if threshold else None)
    exact, tol = out["exact"], out["tolerant"]
    _exact_is_the_oracle(exact, cc.oracle_case(name))
    if name in cc.RECORDED and not cc.spinning(name):
        recorded = cc.RECORDED[name]
        assert np.array_equal(exact["sample_num"], recorded["sample_num"]) and np.array_equal(exact["sample_flags"], recorded["sample_flags"])
        assert float(np.max(np.abs(exact["image"][0] - recorded["I_nu"])) / np.max(np.abs(recorded["I_nu"]))) < TIER_A
    distance = _tolerant_within_its_bound(tol, exact)
    st_e, st_t = exact["stats"], tol["stats"]
    print(f"{name}: tolerant vs exact {distance:.2e}, fused_variant {st_e.fused_variant} / {st_t.fused_variant}, locate launches "
          f"{st_e.launches_locate} / {st_t.launches_locate}, deferred {st_t.n_deferred}")
    # which path ran (bl_render.hip PlanJob)
    if not simulation:
        assert st_e.fused_variant == 0 and st_t.fused_variant == 0 and st_e.launches_locate == 0 and st_t.launches_locate == 0
        if cc.geometric(name):   # no optional geometric cut in bl_shade_formula_fast_kernel: the exact kernels, the exact bits
            assert st_t.arithmetic == 0
            assert gu.same_bits(tol["image"], exact["image"]).all()
        else:
            assert st_t.arithmetic == 1
    elif cc.geometric(name):   # no locate step inside a coefficient kernel
        assert st_t.arithmetic == 1
        assert st_e.fused_variant == 0 and st_t.fused_variant == 0
        assert st_e.launches_locate == st_e.n_chunks >= 1 and st_t.launches_locate == st_t.n_chunks >= 1
    else:   # sim_none and a cell threshold alone: the kernels with the locate step inside
        assert st_t.arithmetic == 1
        assert st_e.fused_variant == 3 and st_t.fused_variant == 2
        assert st_e.launches_locate == 0 and st_t.launches_locate == 0
    if threshold:
        from blacklight_amd import _capi
        general, wide = out["general"], out["wide"]
        assert general["stats"].fused_variant == 2 and general["stats"].switches == _capi.SWITCHES["GENERAL_CUTS"] and general["stats"].composed_maps == 0
        assert wide["stats"].fused_variant == 2 and wide["stats"].switches == 0
        assert wide["stats"].n_deferred > 10 * max(st_t.n_deferred, 1)   # (every sample that reaches the cell cuts goes to the exact pass)
        for other in (general, wide):
            assert other["stats"].n_samples == st_t.n_samples
            print(f"  {name}: vs exact {_tolerant_within_its_bound(other, exact):.2e}, deferred {other['stats'].n_deferred}")


def _same_support(got, want):
    """The same zero, non-zero and NaN pixels."""
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0.0, want == 0.0))


@pytest.mark.parametrize("edge", list(cc.edge_cases()) + ["rho_min_equal", "rho_max_equal", "rho_min_max_equal"])
def test_threshold_edges(edge, built_library):
    """Thresholds of 0.0 and -0.0 (active: the reference's rule is `cut >= 0.0`, restated on the device as infinities on the host and
    as a bit mask), the edges of the geometric settings, and a threshold that a sample equals under nearest-neighbour sampling
    (strict comparisons: the sample survives; cut_cases.equality_cases finds the cell through the oracle, where the neighbouring double
    gives another frame)."""
    if edge in cc.edge_cases():
        overrides, expected = cc.edge_cases()[edge]
        beside = None
    else:
        overrides, beside = cc.equality_cases()[edge]
        expected = None
    params, mock_args = cc.edge_inputs(overrides)
    want = cc.oracle(params, mock_args)
    if beside is not None:   # the case bites on the oracle
        assert np.nanmax(want["image"]) > 0.0 and not gu.same_bits(want["image"], cc.oracle(*cc.edge_inputs(beside))["image"]).all()
    if expected == "none":
        assert gu.same_bits(want["image"], cc.oracle_case("sim_none")["image"]).all()
    if expected == "zero":
        assert (want["image"] == 0.0).all() and np.nanmax(cc.oracle_case("sim_none")["image"]) > 0.0
    out = _both(params, mock_args)
    exact, tol = out["exact"], out["tolerant"]
    _exact_is_the_oracle(exact, want)
    assert tol["stats"].arithmetic == 1
    distance = _tolerant_within_its_bound(tol, exact)
    assert _same_support(tol["image"], exact["image"])
    print(f"{edge}: tolerant vs exact {distance:.2e}, fused_variant {tol['stats'].fused_variant}, deferred {tol['stats'].n_deferred}, "
          f"lit pixels {int((exact['image'] > 0.0).sum())}")


@pytest.mark.parametrize("seed", cc.RANDOM_SEEDS)
def test_randomised_cuts_against_oracle(seed, built_library):
    """One to three cuts from the whole table with a camera angle, a spin, a sampling mode, a mesh layout, Cartesian Kerr-Schild
    coordinates and polarization among the draws (cut_cases.random_configuration): the exact tier against the oracle, bit for bit."""
    params, mock_args = cc.random_configuration(seed)
    want = cc.oracle(params, mock_args)
    assert np.nanmax(want["image"][0]) > 0.0   # (a kept draw: tests/test_cuts_each_host.py holds the seed list to that)
    with _context(params, mock_args) as ctx:
        ctx.set_arithmetic("exact")
        exact = ctx.render()
    _exact_is_the_oracle(exact, want)


def test_two_cameras_with_cuts(built_library):
    """cut_plane and cut_midplane_z - neither reads the camera's position - under bl_set_cameras with two cameras: each camera_slice is
    the bits of a one-camera render with those angles, in the exact tier and in the tolerant tier under bl_set_reproducible."""
    params, mock_args = cc.inputs("sim_none")
    cuts = dict(cc.RECORDED["cut_plane"]["params"], cut_midplane_z=float(cc.RECORDED["cut_midplane_z_neg"]["params"]["cut_midplane_z"]))
    params = dict(params, **{k: v for k, v in cuts.items() if k.startswith("cut_")})
    cameras = [(45.0, 0.0), (110.0, 200.0)]
    for tier in ("exact", "tolerant"):
        with _context(params, mock_args) as ctx:
            ctx.set_arithmetic(tier)
            ctx.set_reproducible(True)
            ctx.set_cameras([th for th, _ in cameras], [ph for _, ph in cameras])
            both = ctx.render()
            slices = [ctx.camera_slice(c) for c in range(2)]
        assert both["image"].shape == (1, 512) and both["stats"].launches_locate >= 1 and both["stats"].fused_variant == 0
        for (th, ph), part in zip(cameras, slices):
            one_params = dict(params, camera_th=th, camera_ph=ph)
            with _context(one_params, mock_args) as ctx:
                ctx.set_arithmetic(tier)
                ctx.set_reproducible(True)
                one = ctx.render()
            assert np.array_equal(both["sample_num"][part], one["sample_num"]) and np.array_equal(both["sample_flags"][part], one["sample_flags"])
            assert gu.same_bits(both["image"][:, part], one["image"]).all(), (tier, th, ph)
            assert np.nanmax(one["image"]) > 0.0
            if tier == "exact":   # ... which is the oracle's frame of that camera, and not the frame without the cuts
                want = cc.oracle(one_params, mock_args)
                _exact_is_the_oracle(one, want)
                without = cc.oracle(dict(cc.inputs("sim_none")[0], camera_th=th, camera_ph=ph), mock_args)
                assert not gu.same_bits(want["image"], without["image"]).all()
