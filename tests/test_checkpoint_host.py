"""The checkpoint code without a GPU (blacklight_amd/csrc/bl_checkpoint.cpp through tests/checkpoint_host_main.cpp): the reference's
own geodesic checkpoints (tests/golden/reader/geodesic_*.ckpt) read, turned into chunks of sample records behind a small record gate -
in pixel order and through a shuffled pixel map - turned back into a file and written; and what the reader says of files that are cut
or lie about their extents. Once built plainly, once under AddressSanitizer and UndefinedBehaviorSanitizer."""
import concurrent.futures
import json
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
from blacklight_amd import build as bl_build
from test_gpu_checkpoint import read_checkpoint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READER_DIR = os.path.join(gu.GOLDEN_DIR, "reader")
FRAME = ("cam_x", "u_con", "u_cov", "norm_con", "norm_con_c", "hor_con_c", "vert_con_c")
# the file's Arrays in order, with the bytes of an entry; geodesic_num_steps (an int of its own) precedes the fifth
ARRAYS = [("camera_pos", 8), ("camera_dir", 8), ("image_frequencies", 8), ("momentum_factors", 8), ("sample_flags", 1), ("sample_num", 4),
          ("sample_pos", 8), ("sample_dir", 8), ("sample_len", 8)]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build(directory, extra):
    """The stand-alone program from its two translation units (side by side), with the host compiler. The library's headers name HIP
    types, so the HIP headers are on the include path; nothing of HIP is linked."""
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(bl_build.hipcc()))), "include")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{hip_include}", f"-I{bl_build.INCLUDE}", f"-I{bl_build.CSRC}"]
    sources = [os.path.join(REPO, "tests", "checkpoint_host_main.cpp"), os.path.join(bl_build.CSRC, "bl_checkpoint.cpp")]
    objects = [os.path.join(directory, os.path.basename(src)[:-4] + ".o") for src in sources]
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
        runs = list(pool.map(lambda pair: subprocess.run(["g++", "-c", pair[0], "-o", pair[1]] + flags + extra, capture_output=True, text=True),
                             zip(sources, objects)))
    for run in runs:
        assert run.returncode == 0, run.stderr
    program = os.path.join(directory, "checkpoint_host_main")
    run = subprocess.run(["g++", "-o", program] + objects + extra, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return program


def _header_offsets(data):
    """Where each Array's five extents start in a geodesic checkpoint"""
    offsets, at = [], 7 * 32
    for n, (_, itemsize) in enumerate(ARRAYS):
        if n == 4:
            at += 4
        offsets.append(at)
        at += 20 + int(np.prod(np.frombuffer(data[at:at + 20], dtype="<i4").astype(np.int64))) * itemsize
    assert at == len(data)
    return offsets


def _run(program, *args):
    run = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert run.returncode in (0, 2), run.stdout + run.stderr   # (anything else: a crash, or a sanitizer's report)
    return run


def _check(program, case, tmp_path):
    expected = np.load(os.path.join(READER_DIR, "expected_checkpoint.npz"), allow_pickle=False)
    params = json.loads(str(expected[f"{case}_params"]))
    camera = [params["camera_resolution"], params["image_num_frequencies"], params["ray_max_steps"]]
    fixture = os.path.join(READER_DIR, f"geodesic_{case}.ckpt")
    data = open(fixture, "rb").read()
    ref = read_checkpoint(fixture)
    n_pix = ref["sample_num"].size
    assert n_pix == 64

    # file -> chunks -> file, in pixel order and through a shuffled map
    out = str(tmp_path / case)
    run = _run(program, "roundtrip", fixture, *camera, out)
    assert run.returncode == 0, run.stdout + run.stderr
    facts = dict(word.split("=") for word in run.stdout.splitlines()[0].split())
    assert int(facts["most"]) == ref["sample_num"].max() and int(facts["gate"]) >= int(facts["most"])
    assert int(facts["chunks_ordered"]) >= 3 and int(facts["chunks_shuffled"]) >= 3
    assert "small gate: Scratch budget too small for the samples of one checkpointed ray" in run.stdout
    written = open(out + ".ordered", "rb").read()
    assert len(written) == len(data)
    assert open(out + ".shuffled", "rb").read() == written
    got = read_checkpoint(out + ".ordered")
    for name in FRAME + ("camera_pos", "camera_dir", "image_frequencies", "momentum_factors"):
        assert got[name].shape == ref[name].shape and gu.same_bits(got[name], ref[name]).all(), name
    assert got["geodesic_num_steps"] == ref["geodesic_num_steps"]
    for name in ("sample_flags", "sample_num"):
        assert got[name].dtype == ref[name].dtype and np.array_equal(got[name], ref[name]), name
    beyond = np.arange(ref["geodesic_num_steps"])[None, :] >= ref["sample_num"][:, None]   # [pixel][step]: past the pixel's samples
    for name in ("sample_pos", "sample_dir", "sample_len"):
        assert got[name].shape == ref[name].shape, name
        assert not got[name][beyond].view(np.uint64).any(), name
    # (sample_dir: shape and tail only - a save renormalises momenta that the load took as renormalised already;
    # test_gpu_checkpoint.py::test_save_matches_the_reference_file holds its values to the reference's)
    assert gu.same_bits(got["sample_pos"][~beyond], ref["sample_pos"][~beyond]).all()
    assert gu.same_bits(got["sample_len"][~beyond], ref["sample_len"][~beyond]).all()

    # cut files: at 100 000 bytes, inside each Array's extents, one byte before the end
    offsets = _header_offsets(data)
    bad = str(tmp_path / f"{case}_bad.ckpt")
    for cut in [100000] + [at + 10 for at in offsets] + [len(data) - 1]:
        with open(bad, "wb") as f:
            f.write(data[:cut])
        run = _run(program, "read", bad, *camera)
        assert run.returncode == 2 and "checkpoint" in run.stdout.splitlines()[0], (cut, run.stdout)
    # extents whose product lies beyond the reader's cap (2^36 bytes), or wraps 64 bits on its way: refused before anything is allocated
    # (a vector of that size is filled with zeros as it is made: the process would hold it, or die of it)
    for extents in ([4, 1 << 30, 8, 1, 1], [1 << 16, 1 << 16, 1 << 16, 1 << 16, 1]):
        with open(bad, "wb") as f:
            f.write(data[:offsets[0]] + np.array(extents, dtype="<i4").tobytes() + data[offsets[0] + 20:])
        run = _run(program, "read", bad, *camera)
        assert run.returncode == 2 and "damaged" in run.stdout.splitlines()[0], (extents, run.stdout)
        assert int(run.stdout.splitlines()[-1].split("=")[1]) < 256 << 10, run.stdout   # peak_rss_kib: under 256 MiB
    # ... and the fixture itself reads
    assert _run(program, "read", fixture, *camera).stdout.splitlines()[0] == "ok"


@pytest.fixture(scope="module")
def plain_program(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("checkpoint_host")), [])


@pytest.mark.parametrize("case", ["sim", "formula"])
def test_reference_checkpoints_round_trip_on_the_host(plain_program, case, tmp_path):
    _check(plain_program, case, tmp_path)


def test_the_same_under_host_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in (statically: a stand-alone binary, nothing
    preloaded), over the same inputs, the cut files included. A report ends the program with another exit code than the two _run takes."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + SANITIZE, capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("the host toolchain cannot link the sanitizer runtimes: " + linked.stderr.strip().splitlines()[-1])
    program = _build(str(tmp_path), SANITIZE)
    for case in ("sim", "formula"):
        _check(program, case, tmp_path)
