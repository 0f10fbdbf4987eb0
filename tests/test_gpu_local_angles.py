"""GPU: theta and phi relative to the centre of the guessed cell (bl_local_angles.h, bl_stats.local_angles) against acos / atan2
(BL_SWITCH_GLOBAL_ANGLES) in the tolerant coefficient kernel's locate step.

Points: bl_debug_math ops 40 / 41 run the kernel's functions on given points against a given angular lattice. Every point must be either
undecided (the exact second pass's) or in the cell that the exact tier's angles (in extended and in double precision) and - where it decides -
the acos / atan2 path give, with a fraction within FRACTION_BOUND of the true one.

The reference angles are the exact tier's, in extended precision: theta = acos(c) of the exact tier's own quotient c = z / r (r from the
device's bl_hypot_g and bl_sqrt_g, so the same double; near the poles that theta is off the true polar angle by far more than the band, and
it is the one every decision is made with), taken as atan2(sqrt((1 - |c|) (1 + |c|)), c), which keeps its accuracy where acos does not; phi
= atan2(y, x) - atan2(a, r). FRACTION_BOUND is the rounding bound of d = angle - centre stated in bl_local_angles.h, over the distance
of two centres, plus the rounding of the fraction's own multiply-add:

    D_BOUND = 2 x 4e-16 (two one-step reciprocal roots) + 9 u (the exact tier's r, in phi) + 8 u (products, table) + 945 / 42240 / 16^11 (series)
    with u = 2^-53: 4.0e-15

Frames: a 64^2 camera over a 64 x 64 x 128 mock, looking down the polar axis (3 degrees: rays cross the axis and the seam of phi) and from
45 degrees, spin 0 and 0.9. The tolerant tier against the exact tier (same rays, per pixel within the tier's 1e-10), the local angles
against the switch (same gathers, images within 1e-12 per pixel, at most 1e-3 of the samples more for the exact pass), reproducible
frames likewise. A grid of 8 x 8 angular cells is beyond the series' reach: the plan keeps acos / atan2 there without any switch, and the image is the
switch run's bit for bit - asserted under bl_set_reproducible, where a frame is bit-reproducible at all; the default frame's composed maps
follow the run-to-run order of the records (tests/test_gpu_xcd_order.py), so two runs of one kernel differ in the last places and the
default frame is held to 1e-12 per pixel instead."""
import os
import sys

import numpy as np
import pytest
import torch   # (before the library: see tests/test_gpu_defaults.py)

import golden_util as gu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U = 2.0 ** -53
D_BOUND = 2 * 4.0e-16 + 9 * U + 8 * U + 945.0 / 42240.0 / 16.0 ** 11
LD = np.longdouble
PI = LD(np.pi) + LD(1.2246467991473532e-16)   # pi to extended precision: the double and its remainder


def _lattice(n_th, n_ph):
    """Faces and centres as blacklight_amd.mock.generate hands them on (through single precision, like the reader)."""
    def as_read(v):
        return v.astype(np.float32).astype(np.float64)
    thf, phf = np.linspace(0.0, np.pi, n_th + 1), np.linspace(0.0, 2.0 * np.pi, n_ph + 1)
    return as_read(thf), as_read(0.5 * (thf[:-1] + thf[1:])), as_read(phf), as_read(0.5 * (phf[:-1] + phf[1:]))


def _points_from_angles(r, th, ph, a):
    """Cartesian Kerr-Schild doubles of (r, theta, phi) (radiation_geometry.cpp:37-57 inverted), computed in extended precision"""
    r, th, ph = LD(1) * np.asarray(r, dtype=LD), np.asarray(th, dtype=LD), np.asarray(ph, dtype=LD)
    psi = ph + np.arctan2(LD(a), r)
    big_r = np.sqrt(r * r + LD(a) * LD(a))
    return np.stack([big_r * np.sin(th) * np.cos(psi), big_r * np.sin(th) * np.sin(psi), r * np.cos(th)], axis=-1).astype(np.float64)


def _reference_angles(ctx, points, a, dtype):
    x, y, z = (points[:, q] for q in range(3))
    rr2 = x * x + y * y + z * z   # bl_radial_coordinate2's operations, in its order
    if a == 0.0:
        r2 = rr2
    else:
        a2 = a * a
        r2 = 0.5 * (rr2 - a2 + ctx.debug_math(11, rr2 - a2, 2.0 * a * z))
    r = ctx.debug_math(12, r2)
    c = z / r
    if dtype is LD:
        c, two_pi = c.astype(LD), 2 * PI
        th = np.arctan2(np.sqrt((1 - np.abs(c)) * (1 + np.abs(c))), c)
    else:   # in the exact tier's precision (another library: the last place may differ)
        two_pi = 2.0 * np.pi
        th = np.arccos(c)
    ph = np.arctan2(y.astype(dtype), x.astype(dtype)) - np.arctan2(dtype(a), r.astype(dtype))
    ph = np.where(ph < 0, ph + two_pi, ph)
    ph = np.where(ph >= two_pi, ph - two_pi, ph)
    return th, ph


def _cell_and_fraction(angle, xf, xv):
    """simulation_sampling.cpp:352-394, :485-490: first cell whose upper face is >= the angle; anchor by the centre, stepping back at the ends"""
    n = xv.size
    c = np.clip(np.searchsorted(xf[1:].astype(angle.dtype), angle, side="left"), 0, n - 1)
    ge = angle >= xv[c]
    anchor = np.where(ge, np.where(c == n - 1, c - 1, c), np.where(c == 0, 0, c - 1))
    frac = (angle - xv[anchor].astype(angle.dtype)) / (xv[anchor + 1] - xv[anchor]).astype(angle.dtype)
    return anchor, frac


def _random_points(n, rng):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * np.exp(rng.uniform(np.log(2.0), np.log(50.0), size=(n, 1)))


def _adversarial_points(lattice, a, rng):
    thf, thv, phf, phv = lattice
    offsets = np.array([0.0, 1.0e-13, -1.0e-13, 1.0e-11, -1.0e-11, 1.0e-9, -1.0e-9])
    pts = []
    for marks, other_lo, other_hi, is_theta in ((np.concatenate([thf, thv]), 0.0, 2.0 * np.pi, True), (np.concatenate([phf, phv]), 0.05, np.pi - 0.05, False)):
        at = (marks[:, None].astype(LD) + offsets[None, :].astype(LD)).ravel()
        other = rng.uniform(other_lo, other_hi, size=at.size)
        r = np.exp(rng.uniform(np.log(2.0), np.log(50.0), size=at.size))
        if is_theta:
            at = np.clip(at, 0, PI)
            pts.append(_points_from_angles(r, at, other, a))
        else:
            pts.append(_points_from_angles(r, other, np.mod(at, 2 * PI), a))
    # the polar axis and its neighbourhood; the seam of phi
    near = np.array([0.0, 1.0e-15, 1.0e-12, 1.0e-9, 1.0e-7, 1.0e-6, 1.0e-4, 3.0e-3, 3.9e-3, 4.0e-3])
    for th in (near.astype(LD), PI - near.astype(LD)):
        for ph in rng.uniform(0.0, 2.0 * np.pi, size=6):
            pts.append(_points_from_angles(np.full(th.size, 7.3), th, np.full(th.size, ph), a))
    seam = np.array([0.0, 1.0e-15, 1.0e-13, 1.0e-12, 1.0e-11, 1.0e-10, 1.0e-9])
    for th in rng.uniform(0.02, np.pi - 0.02, size=8):
        for ph in (seam.astype(LD), 2 * PI - seam.astype(LD)):
            pts.append(_points_from_angles(np.full(ph.size, 11.0), np.full(ph.size, th), ph, a))
    pts.append(np.array([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0], [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [-3.0, -0.0, 1.0], [0.0, 3.0, 0.0], [0.0, -3.0, 0.0]]))
    return np.concatenate(pts)


@pytest.fixture(scope="module")
def ctx(built_library):
    import blacklight_amd as bl
    import bench
    with bl.Context(bl.Params.from_dict(dict(bench.WORKLOAD, camera_resolution=16))) as c:
        yield c


def _check_points(ctx, points, a, lattice, what):
    thf, thv, phf, phv = lattice
    got = ctx.debug_locate_angles(points, a, thf, thv, phf, phv)
    loc, glo = got["local"], got["global"]
    decided = loc["undecided"] == 0
    th, ph = _reference_angles(ctx, points, a, LD)
    th64, ph64 = _reference_angles(ctx, points, a, np.float64)
    worst = 0.0
    for angle, angle64, xf, xv, axis in ((th, th64, thf, thv, "th"), (ph, ph64, phf, phv, "ph")):
        want_cell, want_frac = _cell_and_fraction(angle, xf, xv)
        cell64, _ = _cell_and_fraction(angle64, xf, xv)
        inv_w = 1.0 / np.min(np.diff(xv))
        bound = D_BOUND * inv_w + 4.0 * U * (1.0 + np.abs(want_frac[decided]).astype(np.float64))
        err = np.abs(loc["frac_" + axis][decided].astype(LD) - want_frac[decided]).astype(np.float64)
        worst = max(worst, float(np.max(err / bound)) if err.size else 0.0)
        assert np.array_equal(loc["cell_" + axis][decided], want_cell[decided]), (what, axis)
        assert np.array_equal(loc["cell_" + axis][decided], cell64[decided]), (what, axis)
        both = decided & (glo["undecided"] == 0)
        assert np.array_equal(loc["cell_" + axis][both], glo["cell_" + axis][both]), (what, axis)
        assert np.all(err <= bound), (what, axis, float(np.max(err / bound)))
    print(f"{what}: {points.shape[0]} points, undecided {int((~decided).sum())} local / {int((glo['undecided'] != 0).sum())} global, "
          f"worst fraction error {worst:.2f} of the bound")
    return float((~decided).mean())


@pytest.mark.parametrize("spin", [0.0, 0.9])
@pytest.mark.parametrize("cells", [(32, 64), (256, 256)])
def test_points_are_undecided_or_located_as_by_the_global_angles(ctx, spin, cells):
    rng = np.random.default_rng(20240 + cells[0])
    lattice = _lattice(*cells)
    undecided = _check_points(ctx, _random_points(1 << 16, rng), spin, lattice, f"random, a = {spin}, {cells}")
    if cells == (256, 256):   # (acos / atan2 alone leave about none; a guess good to 1e-6 rad leaves about 2e-4)
        assert undecided <= 1.0e-3
    points = _adversarial_points(lattice, spin, rng)
    _check_points(ctx, points, spin, lattice, f"adversarial, a = {spin}, {cells}")
    # on the polar axis no angle is decided
    axis = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]])
    assert np.all(ctx.debug_locate_angles(axis, spin, *lattice)["local"]["undecided"] == 1)


# ---- frames

@pytest.fixture(scope="module")
def frame_grid():
    from blacklight_amd import mock
    return mock.generate(n_r=64, n_th=64, n_ph=128)


@pytest.fixture(scope="module")
def coarse_grid():
    from blacklight_amd import mock
    return mock.generate(n_r=64, n_th=8, n_ph=8)


def _render(grid, spin, camera_th, tier="tolerant", switch=False, reproducible=False):
    import blacklight_amd as bl
    import bench
    params = dict(bench.WORKLOAD, camera_resolution=64, camera_th=camera_th, simulation_a=spin)
    with bl.Context(bl.Params.from_dict(params)) as c:
        c.set_arithmetic(tier)
        c.set_reproducible(reproducible)
        if switch:
            c.debug_set_switches("GLOBAL_ANGLES")
        c.set_grid(grid)
        out = c.render()
        out["stats"] = c.stats
    return out


def _same_rays(got, want):
    assert np.array_equal(got["sample_num"], want["sample_num"])
    assert np.array_equal(got["sample_flags"], want["sample_flags"])
    assert got["stats"].n_samples == want["stats"].n_samples


def _relative_per_pixel(got, want):
    a, b = got["image"], want["image"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b)
        scale = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
        return float(np.nanmax(np.where(b != 0.0, err / scale, err)))


@pytest.mark.parametrize("reproducible", [False, True])
@pytest.mark.parametrize("camera_th", [3.0, 45.0])
@pytest.mark.parametrize("spin", [0.0, 0.9])
def test_frames_match_the_exact_tier_and_the_global_angles(frame_grid, spin, camera_th, reproducible):
    exact = _render(frame_grid, spin, camera_th, "exact")
    local = _render(frame_grid, spin, camera_th, reproducible=reproducible)
    switch = _render(frame_grid, spin, camera_th, switch=True, reproducible=reproducible)
    assert local["stats"].fused_variant == 2 and switch["stats"].fused_variant == 2
    assert local["stats"].local_angles == 1 and local["stats"].switches == 0
    assert switch["stats"].local_angles == 0 and switch["stats"].switches != 0
    assert exact["stats"].local_angles == 0
    n_samples = local["stats"].n_samples
    print(f"a = {spin}, camera_th = {camera_th}, reproducible = {reproducible}: local vs exact {_relative_per_pixel(local, exact):.2e}, "
          f"switch vs exact {_relative_per_pixel(switch, exact):.2e}, local vs switch {_relative_per_pixel(local, switch):.2e}, "
          f"deferred {local['stats'].n_deferred} local / {switch['stats'].n_deferred} switch of {n_samples}")
    for tolerant in (local, switch):
        _same_rays(tolerant, exact)
        assert _relative_per_pixel(tolerant, exact) <= 1.0e-10
    assert local["stats"].n_gathers == switch["stats"].n_gathers
    assert _relative_per_pixel(local, switch) <= 1.0e-12
    assert local["stats"].n_deferred <= switch["stats"].n_deferred + 1.0e-3 * n_samples


def test_a_coarse_grid_keeps_the_global_angles_without_a_switch(coarse_grid):
    # (bit for bit where the tier is bit-reproducible: bl_set_reproducible; composed maps differ from run to run in the last places)
    plain, switch = _render(coarse_grid, 0.0, 45.0, reproducible=True), _render(coarse_grid, 0.0, 45.0, switch=True, reproducible=True)
    assert plain["stats"].fused_variant == 2 and switch["stats"].fused_variant == 2
    assert plain["stats"].local_angles == 0 and plain["stats"].switches == 0
    assert switch["stats"].local_angles == 0 and switch["stats"].switches != 0
    _same_rays(plain, switch)
    assert plain["stats"].n_deferred == switch["stats"].n_deferred
    assert gu.same_bits(plain["image"], switch["image"]).all()
    composed = _render(coarse_grid, 0.0, 45.0)
    assert composed["stats"].local_angles == 0 and composed["stats"].switches == 0
    assert _relative_per_pixel(composed, switch) <= 1.0e-12
