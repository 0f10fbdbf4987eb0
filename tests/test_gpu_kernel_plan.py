"""GPU: which kernel instantiations a render launches. bl_render decides them once (PlanKernels, bl_render.hip) and says so on one
`kernels:` line per render under BLACKLIGHT_AMD_DEBUG_COUNTERS; the launch wrappers launch what that plan
names and refuse an argument block that disagrees with it. Pinned here for the smallest configurations that reach each branch:
the line itself, the bl_stats fields that follow from it, and a second render of the same camera, which locates nothing."""
import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

FALLBACK = dict(fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)
FOUR_FREQUENCIES = dict(image_num_frequencies=4, image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log")
POWER_LAW = dict(plasma_power_frac=0.3, plasma_p=2.5, plasma_gamma_min=1.0, plasma_gamma_max=1000.0)

# The expected choices are the kernels that a kernel trace (rocprofv3 --kernel-trace) of the commit BEFORE the kernel plan existed
# showed for each configuration - bl_shade_fused2_kernel<true, true, false, false> reads shade=fused2<1,1,0,0> and so on - not what
# PlanKernels says today: a plan that drifts from what used to run fails here.
# id: (golden case, tier, parameter overrides, mesh overrides, setup, expected line)
CASES = {
    "tolerant": ("sim_dp_interp", "tolerant", {}, {}, {},
                 "shade=fused2<1,1,0,0> redo=<0,0,1,1>+0 transfer=composed locate=none geodesic=<DP,0,1,0>"),
    "tolerant_spin": ("sim_dp_interp", "tolerant", dict(simulation_a=0.9), {}, {},
                      "shade=fused2<0,1,0,0> redo=<0,0,1,0>+0 transfer=composed locate=none geodesic=<DP,0,0,0>"),
    "exact": ("sim_dp_interp", "exact", {}, {}, {},
              "shade=exact2<1> redo=none transfer=lane<0> locate=none geodesic=<DP,0,1,0>"),
    "reproducible": ("sim_dp_interp", "tolerant", {}, {}, dict(reproducible=True),
                     "shade=fused2<1,0,0,0> redo=<0,0,1,1>+0 transfer=quad locate=none geodesic=<DP,0,1,0>"),
    "tolerant_four_frequencies": ("sim_dp_interp", "tolerant", FOUR_FREQUENCIES, {}, {},
                                  "shade=fused2<1,0,1,0> redo=<0,0,1,1>+0 transfer=freq locate=none geodesic=<DP,0,1,0>"),
    "exact_four_frequencies": ("sim_dp_interp", "exact", FOUR_FREQUENCIES, {}, {},
                               "shade=exact<1> redo=none coefficients_freq=<1> transfer=lane<0> locate=plain<1> geodesic=<DP,0,1,0>"),
    "power_law": ("sim_dp_interp", "tolerant", POWER_LAW, {}, {},
                  "shade=fast<0,1> redo=<0,1,1,0>+0 transfer=quad locate=plain<1> geodesic=<DP,0,1,0>"),
    "optical_depth": ("sim_dp_interp", "tolerant", dict(image_tau="true"), {}, {},
                      "shade=fast<0,1> redo=<0,1,1,0>+0 transfer=quad+tau locate=plain<1> geodesic=<DP,0,1,0>"),
    "refined": ("sim_dp_interp", "tolerant", {}, dict(_refined=1), {},
                "shade=fused2<1,1,0,1> redo=<0,0,1,1>+0 transfer=composed locate=none geodesic=<DP,0,1,0>"),
    # (the last block's upper edge, where the reference reads past its arrays: the policy is an argument, no kernel's choice)
    "refined_block_interpolation": ("sim_dp_interp", "tolerant", dict(simulation_block_interp="true", **FALLBACK), dict(_refined=1), dict(undefined_policy="edge"),
                                    "shade=fast<0,2> redo=<0,1,1,0>+0 transfer=quad locate=general<1,0,0,0> geodesic=<DP,0,1,0>"),
    "formula": ("formula_64", "tolerant", dict(camera_resolution=32), {}, {},
                "shade=formula_fast redo=<1,0,0,0>+0 transfer=quad locate=none geodesic=<DP,0,0,0>"),
    "auxiliary_rows": ("sim_aux_images", "exact", dict(camera_resolution=32), {}, {},
                       "shade=shade<0,1,0,0,0,0> redo=none transfer=aux locate=plain<1> geodesic=<DP,1,1,0>"),
    "polarized": ("sim_polarized", "tolerant", dict(camera_resolution=32), {}, {},
                  "shade=polarized2<1,0,1> redo=none polarized_frames transfer=aux polarized=matrix locate=none geodesic=<DP,0,1,0>"),
    "polarized_sample_rows": ("sim_polarized", "tolerant", dict(camera_resolution=32, image_length="true"), {}, {},
                              "shade=polarized2<1,1,0> redo=none polarized_coefficients=<0,1> polarized_frames transfer=aux "
                              "polarized=matrices_beside locate=none geodesic=<DP,0,1,0>"),
    "polarized_tensor_transport": ("sim_polarized", "tolerant", dict(camera_resolution=32), {}, dict(switches=["TENSOR_TRANSPORT"]),
                                   "shade=polarized2<1,0,1> redo=none polarized_frames transfer=aux polarized=tensor locate=none geodesic=<DP,0,1,0>"),
    "no_fused_locate": ("sim_dp_interp", "tolerant", {}, {}, dict(switches=["NO_FUSED_LOCATE"]),
                        "shade=fast<1,0> redo=<0,0,1,1>+0 transfer=quad locate=plain<1> geodesic=<DP,0,1,0>"),
}
FUSED_VARIANT = {"fused2": 2, "exact2": 3, "polarized2": 4}   # bl_stats.fused_variant (include/blacklight_amd.h)


def _render(capfd, monkeypatch, case, tier, over, mesh, setup, renders=1):
    """The configuration rendered `renders` times in one context; per render, its stats and the stages of its `kernels:` line."""
    import blacklight_amd as bl
    monkeypatch.setenv("BLACKLIGHT_AMD_DEBUG_COUNTERS", "1")   # (read when the context is created)
    fx, params, mock_args = gu.load_case(case)
    out = []
    with bl.Context(bl.Params.from_dict(dict(params, **over))) as ctx:
        ctx.set_arithmetic(tier)
        if mock_args is not None:
            ctx.set_grid(gu.golden_grid(dict(mock_args, **mesh)))
        if setup.get("reproducible"):
            ctx.set_reproducible(True)
        if setup.get("undefined_policy"):
            ctx.set_undefined_policy(setup["undefined_policy"])
        if setup.get("switches"):
            ctx.debug_set_switches(*setup["switches"])
        for _ in range(renders):
            capfd.readouterr()
            stats = ctx.render()["stats"]
            lines = [line for line in capfd.readouterr().err.splitlines() if line.startswith("kernels: ")]
            assert len(lines) == 1, lines
            out.append((stats, _stages(lines[0][len("kernels: "):])))
    return out


def _stages(line):
    return dict(word.split("=", 1) if "=" in word else (word, "") for word in line.split())


def _check_stats(stats, stages):
    assert stats.fused_variant == FUSED_VARIANT.get(stages["shade"].split("<")[0], 0)
    assert stats.launches_locate == (stats.n_chunks if stages["locate"] != "none" else 0)
    assert stats.launches_geodesic == (stats.n_chunks if stages["geodesic"] != "none" else 0)
    assert stats.n_chunks >= 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_line_names_what_used_to_run(name, capfd, monkeypatch, built_library):
    case, tier, over, mesh, setup, expected = CASES[name]
    (stats, stages), = _render(capfd, monkeypatch, case, tier, over, mesh, setup)
    assert stages == _stages(expected)
    _check_stats(stats, stages)
    assert stats.geodesics_reused == 0 and stats.sampling_reused == 0


def test_second_render_of_a_camera_locates_nothing(capfd, monkeypatch, built_library):
    case, tier, over, mesh, setup, expected = CASES["no_fused_locate"]
    (first, first_stages), (second, second_stages) = _render(capfd, monkeypatch, case, tier, over, mesh, setup, renders=2)
    assert first_stages == _stages(expected)
    # the resident records and located samples shaded again: the same kernels but for the two stages that are not run
    assert second_stages == dict(first_stages, locate="none", geodesic="none")
    assert second.geodesics_reused == 1 and second.sampling_reused == 1
    _check_stats(first, first_stages)
    _check_stats(second, second_stages)
    assert np.isfinite(second.ms_total)
