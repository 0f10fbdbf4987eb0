"""Shared by tests/test_cuts_each_host.py and tests/test_gpu_cuts_each.py: the cases of tests/golden/cut_each.npz, the two formula-mode
cases the reference cannot record, the threshold edges, the equality cases and the randomised draws - with the CPU oracle's frame of
each, rendered once per session and left unchanged."""
import json

import numpy as np

import golden_util as gu
import oracle_api

RECORDED = gu.load_cut_cases()
# Formula mode with a midplane cut: formula_coefficients.cpp:97 and :104 store into sample_cut, which only simulation mode allocates
# (simulation_sampling.cpp:155), and the stock reference ends in a segmentation fault - there is no image to record. The device and the
# oracle skip the sample, which is what the reference's `continue` does behind the store; these two are held to the oracle alone.
UNRECORDED = {"formula_cut_midplane_theta_neg": dict(cut_midplane_theta=-30.0), "formula_cut_midplane_z_pos": dict(cut_midplane_z=6.0)}
ALL_CASES = list(RECORDED) + list(UNRECORDED)
QUANTITIES = ("rho", "n_e", "p_gas", "theta_e", "b", "sigma", "beta_inverse")
CELL_THRESHOLDS = [f"cut_{q}_{side}" for q in QUANTITIES for side in ("min", "max")]
SHARE = (0.05, 0.95)   # of the flux of the frame without a cut: a cut outside it says nothing (tools/make_goldens.py CUT_SHARE)


def inputs(name):
    """(params, mock_args) of a recorded or unrecorded case."""
    if name in UNRECORDED:
        return dict(RECORDED["formula_none"]["params"], **UNRECORDED[name]), None
    return dict(RECORDED[name]["params"]), RECORDED[name]["mock_args"]


def baseline(name):
    return "formula_none" if name.startswith("formula_") else "sim_none"


def spinning(name):
    """a != 0: the spin cases and every formula-mode case (formula_spin = 0.9). Against the stock reference sample counts may move there
    (glibc's hypot / pow against the pinned library's), so the tier-A bound is asked where a = 0."""
    params, _ = inputs(name)
    return float(params["formula_spin" if params["model_type"] == "formula" else "simulation_a"]) != 0.0


def geometric(name):
    return name not in ("sim_none", "formula_none") and name not in CELL_THRESHOLDS


_grids, _frames = {}, {}


def grid_of(mock_args):
    if mock_args is None:
        return None
    key = json.dumps(mock_args, sort_keys=True)
    if key not in _grids:
        _grids[key] = gu.golden_grid(mock_args)
    return _grids[key]


def oracle(params, mock_args, variant="blmath"):
    """The CPU oracle's frame of a configuration (every image row, sample_num, sample_flags): computed once, shared, not to be changed."""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    key = (json.dumps(params, sort_keys=True), json.dumps(mock_args, sort_keys=True), variant)
    if key not in _frames:
        p = bl.Params.from_dict(params)
        grid = grid_of(mock_args)
        res = int(params["camera_resolution"])
        out = oracle_api.render(p.ptr, grid.desc() if grid is not None else None, _capi.RenderDesc, _capi.CameraFrame, n_rays=res * res,
                                variant=variant, max_steps=int(params["ray_max_steps"]), n_freq=int(params.get("image_num_frequencies", 1)))
        for name in ("image", "sample_num", "sample_flags"):
            out[name].setflags(write=False)
        _frames[key] = out
    return _frames[key]


def oracle_case(name, variant="blmath"):
    return oracle(*inputs(name), variant=variant)


def share(image, whole):
    return float(np.nansum(image[0])) / float(np.nansum(whole[0]))


# ---- threshold edges: the reference's activity rule is `cut >= 0.0` - a threshold of 0.0 or -0.0 is active, one of -1.0 is not
def edge_cases():
    """{id: (overrides on sim_none, what the frame has to be: "none" = sim_none's bits, "zero" = no light at all)}.
    An upper threshold of zero cuts every sample whose value is positive: densities, pressures and temperatures always are, and a
    sample with B = 0 (so b, sigma and 1 / beta of zero) has no coefficients anyway (simulation_coefficients.cpp:389-395) - no light is
    left. A lower threshold of zero cuts nothing, as no value is negative."""
    edges = {}
    for q in QUANTITIES:
        for label, zero in (("zero", 0.0), ("negative_zero", -0.0)):
            edges[f"{q}_max_{label}"] = ({f"cut_{q}_max": zero}, "zero")
            edges[f"{q}_min_{label}"] = ({f"cut_{q}_min": zero}, "none")
    for label, zero in (("zero", 0.0), ("negative_zero", -0.0)):
        edges[f"omit_in_{label}"] = (dict(cut_omit_in=zero), "none")      # r < 0 never
        edges[f"omit_out_{label}"] = (dict(cut_omit_out=zero), "zero")    # r > 0 always
    edges["plane_zero_normal"] = (dict(cut_plane="true", cut_plane_origin="1.0,-2.0,0.5", cut_plane_normal="0.0,0.0,0.0"), "none")   # 0 < 0 never
    edges["omit_near_and_far"] = (dict(cut_omit_near="true", cut_omit_far="true"), "zero")   # (but for a sample in the plane through the centre itself)
    return edges


def edge_inputs(overrides):
    params, mock_args = inputs("sim_none")
    return dict(params, **overrides), mock_args


# ---- a threshold that a sample equals: nearest-neighbour sampling, where a sample's rho_cgs is float64(float32 cell value) * simulation_rho_cgs
_equality = {}


def equality_cases():
    """{id: (overrides on sim_none with simulation_interp = "false", overrides of the neighbouring threshold that has to give another frame)}.
    The cell is found through the oracle: over the sorted values v_k = float64(cell rho) * simulation_rho_cgs near the recorded
    cut_rho_min, the frame with cut_rho_min = v_k cuts the samples of the cells below v_k, so it changes between v_k and v_{k+1}
    exactly where the rays sample a cell of value v_k; bisection finds such a k. The comparisons are strict (rho_cgs < min, rho_cgs >
    max): at v_k the samples of that cell survive, at the next double above (min) or below (max) they are cut."""
    if _equality:
        return _equality
    params, mock_args = inputs("sim_none")
    params["simulation_interp"] = "false"
    unit = float(params["simulation_rho_cgs"])
    target = float(RECORDED["cut_rho_min"]["params"]["cut_rho_min"])
    values = np.unique(np.asarray(grid_of(mock_args).prim[0], dtype=np.float32)).astype(np.float64) * unit
    values = values[(values > 0.97 * target) & (values < 1.03 * target)]

    def frame(k):
        return oracle(dict(params, cut_rho_min=float(values[k])), mock_args)["image"]

    lo, hi = 0, values.size - 1
    assert hi > lo and not gu.same_bits(frame(lo), frame(hi)).all()
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if gu.same_bits(frame(lo), frame(mid)).all():
            lo = mid
        else:
            hi = mid
    v = float(values[lo])   # (sampled: the frame changes between values[lo] and values[lo + 1])
    above, below = float(np.nextafter(v, np.inf)), float(np.nextafter(v, 0.0))
    nearest = dict(simulation_interp="false")
    _equality["rho_min_equal"] = (dict(nearest, cut_rho_min=v), dict(nearest, cut_rho_min=above))
    _equality["rho_max_equal"] = (dict(nearest, cut_rho_max=v), dict(nearest, cut_rho_max=below))
    # ... and both at once: only the samples of cells with exactly this value are left
    _equality["rho_min_max_equal"] = (dict(nearest, cut_rho_min=v, cut_rho_max=v), dict(nearest, cut_rho_min=above, cut_rho_max=v))
    return _equality


# ---- randomised draws from the whole table of cuts
N_DRAWS, MAX_REPLACED = 16, 4


def random_configuration(seed):
    """One to three cuts from the whole table, a camera angle, a spin, a sampling mode, a mesh layout, Cartesian Kerr-Schild coordinates
    in a quarter of the draws and polarization in a quarter: (params, mock_args)."""
    rng = np.random.default_rng(4100 + seed)
    params, mock_args = inputs("sim_none")
    recorded = {key: float(RECORDED[key]["params"][key]) for key in CELL_THRESHOLDS}
    table = [(lambda key=key: {key: recorded[key] * float(2.0 ** rng.uniform(-1.0, 1.0))}) for key in CELL_THRESHOLDS]
    table += [lambda: dict(cut_omit_near="true"), lambda: dict(cut_omit_far="true"),
              lambda: dict(cut_omit_in=float(rng.uniform(3.0, 10.0))), lambda: dict(cut_omit_out=float(rng.uniform(5.0, 20.0))),
              lambda: dict(cut_midplane_theta=float(rng.uniform(3.0, 30.0))), lambda: dict(cut_midplane_theta=-float(rng.uniform(3.0, 30.0))),
              lambda: dict(cut_midplane_z=float(rng.uniform(0.3, 3.0))), lambda: dict(cut_midplane_z=-float(rng.uniform(0.3, 3.0))),
              lambda: dict(cut_plane="true", cut_plane_origin=",".join(repr(float(x)) for x in rng.uniform(-3.0, 3.0, 3)),
                           cut_plane_normal=",".join(repr(float(x)) for x in rng.normal(size=3)))]
    assert len(table) == 23
    over = {}
    for entry in rng.choice(len(table), size=int(rng.integers(1, 4)), replace=False):
        over.update(table[int(entry)]())
    over.update(camera_th=float(rng.uniform(10.0, 170.0)), camera_ph=float(rng.uniform(0.0, 360.0)),
                simulation_a=float(rng.choice([0.0, 0.5, 0.9])), simulation_interp=str(rng.choice(["true", "false"])),
                fallback_nan="false", fallback_rho=1.0e-6, fallback_pgas=1.0e-8)
    mesh = [{}, dict(_blocks=[2, 2, 2]), dict(_refined=1)][int(rng.integers(0, 3))]
    if int(rng.integers(0, 4)) == 0:   # the same arrays read as a Cartesian Kerr-Schild box, looked at along x (tests/test_gpu_parity.py)
        over.update(simulation_coord="cks", camera_th=float(rng.uniform(75.0, 100.0)), camera_ph=float(rng.uniform(-15.0, 15.0)))
    if int(rng.integers(0, 4)) == 0:
        over.update(image_polarization="true")
    return dict(params, **over), dict(mock_args, **mesh)


def accepted(seed):
    """A draw is kept only if the oracle's frame has a positive pixel (cuts that leave no light test nothing)."""
    image = oracle(*random_configuration(seed))["image"]
    return bool(np.nanmax(image[0]) > 0.0)


# The first N_DRAWS accepted seeds, counted from 0: a rejected draw is replaced with the next seed (test_cuts_each_host.py holds this
# list to that rule on the CPU, and to at most MAX_REPLACED replacements)
RANDOM_SEEDS = [0, 1, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17]   # (2 and 9: cuts that leave no light)
