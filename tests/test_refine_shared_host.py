"""The criteria both refinement calls share (blacklight_amd/csrc/bl_refine.h) on their own, through tests/refine_host_main.cpp: the
stand-alone program walks a block pixel by pixel as the kernel does and must decide as the numpy restatement of the reference does
(tests/refine_restatement.py) - built plainly and under ASan / UBSan, where a read beside the block or an undefined operation fails."""
import os
import subprocess

import numpy as np
import pytest

import refine_restatement as rr
from blacklight_amd import build as bl_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITERIA = ("val", "abs_grad", "rel_grad", "abs_lapl", "rel_lapl")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _cases():
    rng = np.random.default_rng(777)
    cases = []
    for n in range(120):
        bs = int(rng.choice([2, 3, 4, 8, 16, 17]))
        p = {}
        for name, scale in zip(CRITERIA, (1.0, 0.5, 1.0, 0.5, 2.0)):
            p[f"adaptive_{name}_cut"] = float(rng.uniform(0.0, scale))
            p[f"adaptive_{name}_frac"] = float(rng.choice([-1.0, 0.0, 0.1, 0.25, 0.5, 0.9]))
        block = rng.uniform(0.0, 1.5, (bs, bs)) * np.abs(np.sin(np.arange(bs * bs).reshape(bs, bs) * rng.uniform(0.01, 1.0)))
        kind = n % 5
        if kind == 1:
            block[rng.random((bs, bs)) < 0.3] = np.nan
        elif kind == 2:
            block[rng.random((bs, bs)) < 0.2] = 0.0
            block[rng.random((bs, bs)) < 0.1] = np.inf
        elif kind == 3:
            block = block - 0.6
        elif kind == 4:
            block[...] = rng.choice([np.nan, 0.0, -0.0, np.inf, 1.0])
        cases.append((bs, p, block))
    return cases


def _build(directory, extra):
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", f"-I{bl_build.INCLUDE}", f"-I{bl_build.CSRC}"]
    program = os.path.join(directory, "refine_host_main")
    run = subprocess.run(["g++", "-o", program, os.path.join(REPO, "tests", "refine_host_main.cpp")] + flags + extra, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return program


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("sanitized", [False, True])
def test_the_shared_criteria_alone_plain_and_under_the_sanitizers(tmp_path, sanitized):
    program = _build(str(tmp_path), SANITIZE if sanitized else [])
    cases = _cases()
    lines = "".join(" ".join([str(bs)] + [repr(p[f"adaptive_{name}_cut"]) for name in CRITERIA] + [repr(p[f"adaptive_{name}_frac"]) for name in CRITERIA]
                             + [repr(float(v)) for v in block.reshape(-1)]) + "\n" for bs, p, block in cases)
    run = subprocess.run([program], input=lines, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    got = [line.split()[0] == "1" for line in run.stdout.splitlines()]
    want = [bool(rr.evaluate_block(block, p)) for bs, p, block in cases]
    assert len(got) == len(cases) and got == want, [n for n, (g, w) in enumerate(zip(got, want)) if g != w]
    assert any(want) and not all(want)
