"""The closed-form proper distance without a GPU (blacklight_amd/csrc/bl_distance_closed.h through tests/distance_host_main.cpp): rays
integrated on the CPU with bl_geodesic_rhs<true> and the Dormand-Prince tableau, the reference's s and the closed mode's quantities
side by side. Held to the header's own figures - not to what the program happens to print:

  * the closed derivative lies within the relative distance of the reference's that the header's table adds up;
  * per accepted step |Q_ref - Q| is at most the derived bound (the bound itself, not the 16-fold band);
  * every decided step has ceil(Q) == ceil(Q_ref);
  * at most 1e-6 of the steps of the whole sample are undecided (a cap: the band is ~1e-10 in Q);
  * what the header assumes of a stage's point (f, |k_t| / |k|, l.l) holds at every stage the program evaluated.

Ray sets: a = 0, plane camera at r = 50 and 45 degrees, a 64^2 lattice; 200 impact parameters within 1e-3 of 3 sqrt(3) M; a = 0.9 from
r = 1000 (large s); a = 0.5; ray_flat. Once built plainly, once under AddressSanitizer and UndefinedBehaviorSanitizer (stand-alone).

LOOSE_AND_TIGHT: the first and the third of them again at ray_tol = 1e-3 with ray_step = 0.3 (an accepted step spans many samples and its
stages lie far from the accepted path) and the first at ray_tol = 1e-12 (errors near 1 all the time), held to the same figures of the
header; their undecided share is printed, not capped. What the header assumes of a stage's point is needed where a stage's d s / d lambda
enters a count, which is in accepted steps: the program counts those under the figures' own names and the stages of rejected steps under
rejected_*. On the sets at 1e-8 and 1e-12 both are held to the header's limits, as before the split; at 1e-3 with steps of 0.3 r the first
tries near the hole are rejected with |k_t| / |k| up to 10.7 at a stage (1 160 and 8 such stages), and the accepted steps stay within 1.81
of the 2 assumed."""
import os
import subprocess

import pytest

from blacklight_amd import build as bl_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
SETS = ("a0", "ring", "a09", "a05", "flat")
LOOSE_AND_TIGHT = ("a0_loose", "a09_loose", "a0_tight")


def _build(directory, extra):
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(bl_build.hipcc()))), "include")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{hip_include}", f"-I{bl_build.INCLUDE}", f"-I{bl_build.CSRC}"]
    program = os.path.join(directory, "distance_host_main")
    run = subprocess.run(["g++", os.path.join(REPO, "tests", "distance_host_main.cpp"), "-o", program] + flags + extra, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return program


def _figures(program, name):
    run = subprocess.run([program, name], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]   # (anything else: a crash, or a sanitizer's report)
    print(f"--- {name}\n{run.stdout}")
    return {words[0]: float(words[1]) for words in (line.split() for line in run.stdout.splitlines())}


def _check(fig, name):
    assert fig["rays"] == (200 if name == "ring" else 4096) and fig["steps"] > fig["rays"]
    assert fig["assumption_failures"] == 0
    assert fig["max_derivative"] <= fig["derivative_bound"]
    assert fig["max_ratio"] <= 1.0
    assert fig["ceil_mismatch"] == 0
    if name != "flat":
        assert fig["stages"] > 6 * fig["rays"] and fig["max_f"] <= 4.0 and fig["max_eps_l_in_u"] <= 64.0 and fig["max_kt_over_k"] <= 2.0
    if name in ("a09", "a09_loose"):
        assert fig["max_s"] > 1000.0   # (the set is there for large s)
    if name in SETS:   # (the stages of rejected steps as well, as before the program told the two apart)
        assert fig["rejected_assumption_failures"] == 0
        if name != "flat":
            assert fig["rejected_max_f"] <= 4.0 and fig["rejected_max_eps_l_in_u"] <= 64.0 and fig["rejected_max_kt_over_k"] <= 2.0


@pytest.fixture(scope="module")
def all_figures(tmp_path_factory):
    program = _build(str(tmp_path_factory.mktemp("distance_host")), [])
    return {name: _figures(program, name) for name in SETS}


@pytest.mark.parametrize("name", SETS)
def test_closed_distance_within_its_bound(all_figures, name):
    _check(all_figures[name], name)


def test_share_of_undecided_steps(all_figures):
    steps = sum(fig["steps"] for fig in all_figures.values())
    undecided = sum(fig["undecided"] for fig in all_figures.values())
    print(f"steps {steps:.0f} undecided {undecided:.0f} largest ratio {max(fig['max_ratio'] for fig in all_figures.values()):.4f}")
    assert steps > 1.0e6 and undecided <= 1.0e-6 * steps


@pytest.fixture(scope="module")
def loose_and_tight_figures(tmp_path_factory):
    program = _build(str(tmp_path_factory.mktemp("distance_host_tolerances")), [])
    return {name: _figures(program, name) for name in LOOSE_AND_TIGHT}


@pytest.mark.parametrize("name", LOOSE_AND_TIGHT)
def test_closed_distance_at_other_tolerances(loose_and_tight_figures, name):
    fig = loose_and_tight_figures[name]
    print(f"{name}: steps {fig['steps']:.0f} undecided {fig['undecided']:.0f} (share {fig['undecided'] / fig['steps']:.2e}) largest ratio {fig['max_ratio']:.4f} "
          f"|k_t| / |k| at most {fig['max_kt_over_k']:.4f}; in rejected steps {fig['rejected_max_kt_over_k']:.4f}, {fig['rejected_assumption_failures']:.0f} stages outside the assumptions")
    _check(fig, name)


def test_the_same_under_host_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in (statically: a stand-alone binary, nothing
    preloaded). A report ends the program with another exit code than _figures takes."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + SANITIZE, capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the host toolchain cannot link the sanitizer runtimes: " + linked.stderr.strip().splitlines()[-1])
    program = _build(str(tmp_path), SANITIZE)
    for name in SETS + LOOSE_AND_TIGHT:
        _check(_figures(program, name), name)
