"""Helpers of the frequency-list tests (tests/test_frequencies_host.py, tests/test_gpu_frequencies.py, tests/test_gpu_frequencies_cli.py):
the list they use, the test side's own statement of the image-row layout, and the one-frequency block a row is held against."""

L = [3.45e11, 8.6e10, 2.3e11, 2.3e11, 1.0e12]   # unordered, with a duplicate; taken at lengths 1 to 5 (both sides of the plan's n_nu >= 4)


def labels(params, n):
    """Every image row of a block with n frequencies, in row order (radiation_integrator.cpp:436-520), as (quantity, frequency or None,
    component): Stokes rows 4 l + a, time, length, then lambda, emission, tau by frequency, the cell values 7 l + k, crossings."""
    def on(key):
        return str(params.get(key, "false")).lower() == "true"
    simulation = params["model_type"] == "simulation"
    rows = []
    if on("image_light"):
        stride = 4 if simulation and on("image_polarization") else 1
        rows += [("light", l, a) for l in range(n) for a in range(stride)]
    rows += [(name, None, 0) for name in ("time", "length") if on("image_" + name)]
    rows += [(name, l, 0) for name in ("lambda", "emission", "tau") if on("image_" + name) for l in range(n)]
    rows += [(name, l, k) for name in ("lambda_ave", "emission_ave", "tau_int") if simulation and on("image_" + name) for l in range(n) for k in range(7)]
    rows += [("crossings", None, 0)] if on("image_crossings") else []
    return rows


def rows_of(params, n, l):
    """Where the rows of a one-frequency block lie in a block with n frequencies, for frequency l: one index per row of the former."""
    many = labels(params, n)
    return [many.index((name, None if f is None else l, k)) for name, f, k in labels(params, 1)]


def one_frequency(params, hz):
    """The block with image_num_frequencies = 1 and image_frequency = hz - that exact double."""
    params = {k: v for k, v in params.items() if k not in ("image_frequency_start", "image_frequency_end", "image_frequency_spacing")}
    return dict(params, image_num_frequencies=1, image_frequency=repr(float(hz)))
