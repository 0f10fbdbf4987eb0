"""Helpers of the .input sweep tests (tests/test_input_sweep_host.py, tests/test_gpu_input_sweep.py)."""
import io
import os
import struct
import subprocess
import zipfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "blacklight_amd", "bin", "blacklight_amd")


def file_bytes(path):
    """The bytes of an output file that are the writer's: all of them for .npy and raw files; for a .npz every byte except the
    modification time and date of its ZIP headers (two 16-bit fields per local and per central header, zip_format.cpp: the wall
    clock at the moment of writing, in two-second steps - the one thing two writes of the same arrays do not share)."""
    data = bytearray(open(path, "rb").read())
    if data[:4] != b"PK\x03\x04":
        return bytes(data)
    with zipfile.ZipFile(io.BytesIO(bytes(data))) as archive:
        offsets = [info.header_offset for info in archive.infolist()]
        central = archive.start_dir
    for offset in offsets:
        assert data[offset:offset + 4] == b"PK\x03\x04"
        data[offset + 10:offset + 14] = bytes(4)
    at = central
    while data[at:at + 4] == b"PK\x01\x02":
        data[at + 12:at + 16] = bytes(4)
        name, extra, comment = struct.unpack_from("<HHH", data, at + 28)
        at += 46 + name + extra + comment
    assert data[at:at + 4] in (b"PK\x05\x06", b"PK\x06\x06"), "central directory not walked to its end"
    return bytes(data)


def write_input(path, params):
    with open(path, "w") as f:
        for key, value in params.items():
            f.write(f"{key} = {value}\n")
    return str(path)


def run_cli(input_path, env=None, timeout=600):
    """One fresh child process of bin/blacklight_amd; the caller stops at the first non-zero exit status (assert)."""
    full = dict(os.environ)
    full.update(env or {})
    run = subprocess.run([EXE, str(input_path)], capture_output=True, text=True, timeout=timeout, env=full)
    assert run.returncode == 0, run.stdout + run.stderr
    return run


def comma(values):
    return ",".join(repr(float(v)) for v in values)
