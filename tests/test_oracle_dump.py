"""The CPU oracle's one-ray dump of coefficients (blo_render_dump, blo_dump_coefficients: k T_e, j_nu, alpha_nu, delta tau), which
tests/test_gpu_variant_edges.py reads to prove which branches of the transfer step its cases reach: the dumped samples are the ones
the ray's images integrate - and blo_render, whose blo_extra keeps its layout for the callers built against it."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import oracle_api

M_E_C2 = 9.1093837015e-28 * 2.99792458e10 ** 2


def _run(overrides, ray):
    import blacklight_amd as bl
    from blacklight_amd import _capi
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    params = dict(params, image_tau="true", **overrides)
    p = bl.Params.from_dict(params)
    grid = gu.golden_grid(mock_args)
    n = int(params["camera_resolution"]) ** 2
    plain = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4)
    out = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4, dump_ray=ray,
                            max_steps=int(params["ray_max_steps"]))
    assert gu.same_bits(plain["image"], out["image"]).all()   # (dumping changes nothing)
    return out


@pytest.mark.parametrize("overrides", [{}, {"simulation_rho_cgs": 1.0e-13}, {"image_frequency": 1.0e15, "simulation_rho_cgs": 1.0e-19}],
                         ids=["fixture", "thick", "underflow"])
@pytest.mark.parametrize("ray", [528, 330])
def test_dump_is_what_the_ray_integrates(built_library, overrides, ray):
    out = _run(overrides, ray)
    d = out["dump"]
    n = int(out["sample_num"][ray])
    assert n > 0 and all(len(d[k]) == n for k in ("kte", "j", "alpha", "dtau"))
    # the optical depth image is the sum of the dumped steps', in the same order: the same bits
    tau = 0.0
    for step in d["dtau"]:
        tau += step
    assert gu.same_bits(out["image"][1, ray], tau)
    # the intensity, restated over the dumped coefficients (unpolarized.cpp:74-110) in numpy's exp / expm1
    nu = float(out["frequencies"][0])
    intensity = 0.0
    for j, alpha, dtau in zip(d["j"], d["alpha"], d["dtau"]):
        if alpha > 0.0:
            intensity = np.exp(-dtau) * (intensity + j / alpha * np.expm1(dtau)) if dtau <= 100.0 else j / alpha
    want = out["image"][0, ray] / nu ** 3
    emitting_without_absorption = (d["j"] > 0.0) & ~(d["alpha"] > 0.0)
    if not emitting_without_absorption.any():   # (without alpha the dump holds no step length to restate j dl with)
        assert abs(intensity - want) <= 1.0e-12 * abs(want) + 2.0 ** -1074 * n
    # k T_e: finite and positive wherever a sample emits, a plausible temperature (Theta_e), NaN where no coefficients are formed
    emits = d["j"] > 0.0
    assert np.all(np.isfinite(d["kte"][emits]) & (d["kte"][emits] > 0.0))
    formed = np.isfinite(d["kte"])
    assert formed.any() and np.all(d["kte"][formed] / M_E_C2 < 1.0e4)
    assert np.all(d["j"][~formed] == 0.0) and np.all(d["alpha"][~formed] == 0.0)


def test_blo_render_reads_no_more_than_blo_extra(built_library):
    """A caller that allocates exactly blo_extra and asks for a ray dump: blo_render reads and writes nothing beyond the struct (the
    words after it here point at a sentinel buffer, which stays as it was)"""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    p = bl.Params.from_dict(params)
    grid = gu.golden_grid(mock_args)
    n, max_steps = int(params["camera_resolution"]) ** 2, int(params["ray_max_steps"])
    sentinel = np.full(max_steps, 7.0)
    size = C.sizeof(oracle_api.Extra)
    raw = (C.c_uint8 * (size + 8 * 8))()
    tail = (C.c_void_p * 8).from_buffer(raw, size)
    for k in range(8):
        tail[k] = sentinel.ctypes.data
    extra = oracle_api.Extra.from_buffer(raw)
    extra.num_threads, extra.dump_ray = 4, 528
    dump = dict(pos=np.zeros((max_steps, 4)), dir=np.zeros((max_steps, 4)), len=np.zeros(max_steps))
    for name, arr in dump.items():
        setattr(extra, f"dump_{name}", arr.ctypes.data_as(C.c_void_p))
    image, sample_num, sample_flags = np.zeros((1, n)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    d = _capi.RenderDesc()
    d.n_rays, d.outputs_on_device = n, 0
    d.image, d.sample_num, d.sample_flags = (a.ctypes.data_as(C.c_void_p) for a in (image, sample_num, sample_flags))
    frame, freqs, err = _capi.CameraFrame(), np.zeros(1), C.create_string_buffer(1024)
    L = oracle_api.load()
    rc = L.blo_render(p.ptr, C.byref(grid.desc()), C.byref(d), C.byref(frame), freqs.ctypes.data_as(C.c_void_p), C.byref(extra),
                      err, C.c_size_t(len(err)))
    assert rc == 0, err.value.decode()
    assert np.all(sentinel == 7.0)
    assert extra.dump_num == sample_num[528] > 0
    want = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4)
    assert gu.same_bits(image, want["image"]).all()


@pytest.mark.parametrize("overrides", [{}, {"simulation_rho_cgs": 1.0e-12}, {"image_frequency": 1.0e15}, {"image_rotation_split": "true"}],
                         ids=["fixture", "thick", "1e15hz", "split"])
@pytest.mark.parametrize("ray", [300, 297])
def test_polarized_dump_changes_nothing_and_is_what_the_ray_integrates(built_library, overrides, ray):
    """blo_render_dump_polarized (blo_dump_polarized: j_Q, j_V, alpha_Q, alpha_V, rho_Q, rho_V, delta lambda_cgs), which
    tests/test_gpu_polarized_edges.py reads: a render with both dumps on returns the image, sample_num and sample_flags of a render
    without, bit for bit; the dumped values hang together with blo_dump_coefficients' and with the optical-depth row"""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    fx, params, mock_args = gu.load_case("sim_polarized")
    params = dict(params, **overrides)
    p = bl.Params.from_dict(params)
    grid = gu.golden_grid(mock_args)
    n, max_steps = int(params["camera_resolution"]) ** 2, int(params["ray_max_steps"])
    plain = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4)
    one = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4, dump_ray=ray, max_steps=max_steps)
    out = oracle_api.render(p.ptr, grid.desc(), _capi.RenderDesc, _capi.CameraFrame, n_rays=n, num_threads=4, dump_ray=ray, max_steps=max_steps,
                            dump_polarized=True)
    for got in (one, out):
        assert gu.same_bits(plain["image"], got["image"]).all()
        assert np.array_equal(plain["sample_num"], got["sample_num"]) and np.array_equal(plain["sample_flags"], got["sample_flags"])
    names = ("j_q", "j_v", "alpha_q", "alpha_v", "rho_q", "rho_v", "dlambda")
    assert not any(name in one["dump"] for name in names)   # (only when asked for)
    d = out["dump"]
    count = int(out["sample_num"][ray])
    assert count > 0 and all(len(d[name]) == count for name in names)
    assert all(gu.same_bits(d[name], one["dump"][name]).all() for name in ("pos", "dir", "len", "kte", "j", "alpha", "dtau"))
    assert gu.same_bits(d["dtau"], d["alpha"] * d["dlambda"]).all() and np.all(d["dlambda"] > 0.0)
    tau = 0.0
    for step in d["dtau"]:
        tau += step
    assert gu.same_bits(out["image"][4, ray], tau)   # rows I, Q, U, V, tau
    formed = np.isfinite(d["kte"])
    assert formed.any() and all(np.all(d[name][~formed] == 0.0) for name in names[:6])
    # polarized emission and absorption never exceed the unpolarized ones; the fixture's plasma rotates wherever it has coefficients
    assert np.all(np.hypot(d["j_q"], d["j_v"]) <= d["j"] * (1.0 + 1.0e-12)) and np.all(np.hypot(d["alpha_q"], d["alpha_v"]) <= d["alpha"] * (1.0 + 1.0e-12))
    assert np.all(np.hypot(d["rho_q"], d["rho_v"])[formed] > 0.0)
