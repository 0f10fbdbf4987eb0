"""bl_set_grid_device without a GPU: what the host decides about a bl_device_cells description before anything is launched
(CheckDeviceCells, blacklight_amd/csrc/bl_grid.cpp).

One table of cases, driven twice: through the library on a host-only context (device = -2), where a refused description gives
BL_E_ARG with its text and a valid one goes on to the context's own refusal, BL_E_DEVICE; and through tests/device_grid_host_main.cpp,
built with bl_grid.cpp alone, plainly and under AddressSanitizer and UndefinedBehaviorSanitizer (the extent check multiplies 64-bit
numbers it does not trust). Nothing is loaded into Python under a sanitizer.

Extents: the 8 blocks of 16 x 12 x 16 cells of the sim_multiblock goldens in both layouts, with and without the ninth variable of
plasma_model = code_kappa, each at the exact extent and one element short; one block of 2048 x 2048 x 1024 = 2^32 cells, whose
extent a 32-bit product would wrap to zero; a variable stride of 2^62, whose product with 7 leaves 64 bits."""
import ctypes as C
import os
import subprocess

import pytest

import golden_util as gu
from blacklight_amd import build as bl_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
E_DEVICE, E_ARG = 4, 5   # include/blacklight_amd.h
F32, F64 = 0, 1
NO_CELLS = "bl_device_cells: the description is NULL."
NO_PRIM = "bl_device_cells: prim is NULL."
BAD_DTYPE = "bl_device_cells: dtype must be BL_CELLS_F32 or BL_CELLS_F64."
MISALIGNED = "bl_device_cells: prim is not aligned to its element type."
BAD_VAR_STRIDE = "bl_device_cells: var_stride must be at least 1."
BAD_BLOCK_STRIDE = "bl_device_cells: block_stride must be at least 1."
TOO_SHORT = "bl_device_cells: n_elements is smaller than what the strides and the grid's extents reach."
HOST_ONLY = "Host-only context: no HIP device selected (the hot path has no CPU fallback)."

BLOCK = 16 * 12 * 16
PRIM = 0x10000   # an address nothing reads


def _case(want, n_blocks=8, n=(16, 12, 16), n_var=8, ind_kappa=0, first=0, code_kappa=0, cells=1, prim=PRIM, dtype=F32, wait=0,
          var_stride=8 * BLOCK, block_stride=BLOCK, n_elements=64 * BLOCK):
    return dict(want=want, n_blocks=n_blocks, n_i=n[0], n_j=n[1], n_k=n[2], n_var=n_var, ind_kappa=ind_kappa, first=first, code_kappa=code_kappa,
                cells=cells, prim=prim, dtype=dtype, wait=wait, var_stride=var_stride, block_stride=block_stride, n_elements=n_elements)


VB = dict(var_stride=8 * BLOCK, block_stride=BLOCK)          # [var][block]: the reference's
BV = dict(var_stride=BLOCK, block_stride=8 * BLOCK)          # [block][var], 8 variables
BV9 = dict(var_stride=BLOCK, block_stride=9 * BLOCK)         # [block][var], 9 variables
KAPPA = dict(n_var=9, ind_kappa=8)
HUGE = dict(n_blocks=1, n=(2048, 2048, 1024), var_stride=1 << 32, block_stride=1 << 32)
CASES = {
    "null_cells": _case(NO_CELLS, cells=0),
    "null_prim": _case(NO_PRIM, prim=0),
    "dtype_2": _case(BAD_DTYPE, dtype=2),
    "dtype_negative": _case(BAD_DTYPE, dtype=-1),
    "f64_at_4_bytes": _case(MISALIGNED, prim=PRIM + 4, dtype=F64),
    "f32_at_2_bytes": _case(MISALIGNED, prim=PRIM + 2),
    "var_stride_0": _case(BAD_VAR_STRIDE, var_stride=0),
    "block_stride_0": _case(BAD_BLOCK_STRIDE, block_stride=0),
    "block_stride_negative": _case(BAD_BLOCK_STRIDE, block_stride=-BLOCK),
    "vb_exact": _case(None, **VB),
    "vb_f64_wait": _case(None, dtype=F64, wait=1, **VB),
    "vb_one_short": _case(TOO_SHORT, n_elements=64 * BLOCK - 1, **VB),
    "bv_exact": _case(None, **BV),
    "bv_one_short": _case(TOO_SHORT, n_elements=64 * BLOCK - 1, **BV),
    "vb_variables_3_to_10_exact": _case(None, n_var=11, first=3, n_elements=88 * BLOCK, **VB),
    "vb_variables_3_to_10_one_short": _case(TOO_SHORT, n_var=11, first=3, n_elements=88 * BLOCK - 1, **VB),
    "vb_kappa_exact": _case(None, code_kappa=1, n_elements=72 * BLOCK, **VB, **KAPPA),
    "vb_kappa_one_short": _case(TOO_SHORT, code_kappa=1, n_elements=72 * BLOCK - 1, **VB, **KAPPA),
    "vb_kappa_not_read": _case(None, code_kappa=0, n_elements=64 * BLOCK, **VB, **KAPPA),   # (another plasma model: eight variables are read)
    "bv_kappa_exact": _case(None, code_kappa=1, n_elements=72 * BLOCK, **BV9, **KAPPA),
    "bv_kappa_one_short": _case(TOO_SHORT, code_kappa=1, n_elements=72 * BLOCK - 1, **BV9, **KAPPA),
    "bv_kappa_not_read": _case(None, code_kappa=0, n_elements=72 * BLOCK - BLOCK, **BV9, **KAPPA),
    "two_to_32_cells_exact": _case(None, n_elements=1 << 35, **HUGE),
    "two_to_32_cells_one_short": _case(TOO_SHORT, n_elements=(1 << 35) - 1, **HUGE),
    "two_to_32_cells_wrapped": _case(TOO_SHORT, n_elements=1 << 20, **HUGE),
    "stride_leaves_64_bits": _case(TOO_SHORT, var_stride=1 << 62, block_stride=BLOCK, n_elements=(1 << 63) - 1),
    "negative_extent": _case(TOO_SHORT, n_elements=-1, **VB),
}
FIELDS = ("n_blocks", "n_i", "n_j", "n_k", "n_var", "ind_kappa", "first", "code_kappa", "cells", "prim", "dtype", "wait", "var_stride", "block_stride", "n_elements")


def test_struct_size_is_the_librarys(built_library):
    from blacklight_amd import _capi
    assert C.sizeof(_capi.DeviceCells) == _capi.lib().bl_device_cells_sizeof() == 48


@pytest.mark.parametrize("slice_call", [False, True])
def test_refusals_on_a_host_only_context(built_library, slice_call):
    """Every description of the table through bl_set_grid_device (and bl_set_grid_slice_device on a slow-light context): its refusal
    word for word, and for a valid one the host-only context's BL_E_DEVICE - the check ran first and let it through."""
    import blacklight_amd as bl
    from blacklight_amd import _capi
    contexts = {}
    try:
        for code_kappa in (0, 1):
            fx, params, _ = gu.load_case("slow_interp" if slice_call else ("sim_code_kappa" if code_kappa else "sim_dp_interp"))
            if slice_call and code_kappa:
                params = dict(params, plasma_model="code_kappa")
            contexts[code_kappa] = bl.Context(bl.Params.from_dict(params), device=-2)
        L = _capi.lib()
        for name, case in CASES.items():
            ctx = contexts[case["code_kappa"]]
            g = _capi.GridDesc()
            g.n_blocks, g.n_i, g.n_j, g.n_k, g.n_var = (case[k] for k in ("n_blocks", "n_i", "n_j", "n_k", "n_var"))
            g.ind_kappa = case["ind_kappa"]
            for offset, field in enumerate(("ind_rho", "ind_pgas", "ind_uu1", "ind_uu2", "ind_uu3", "ind_bb1", "ind_bb2", "ind_bb3")):
                setattr(g, field, case["first"] + offset)
            cells = _capi.DeviceCells()
            cells.prim, cells.dtype, cells.wait = case["prim"] or None, case["dtype"], case["wait"]
            cells.var_stride, cells.block_stride, cells.n_elements = case["var_stride"], case["block_stride"], case["n_elements"]
            handed = C.byref(cells) if case["cells"] else None
            rc = L.bl_set_grid_slice_device(ctx._ctx, 0, C.byref(g), handed, 0.0) if slice_call else L.bl_set_grid_device(ctx._ctx, C.byref(g), handed)
            text = L.bl_last_error(ctx._ctx).decode()
            want_code, want_text = (E_ARG, case["want"]) if case["want"] is not None else (E_DEVICE, HOST_ONLY)
            assert (rc, text) == (want_code, f"Error: {want_text}\n"), name
            assert L.bl_grid_host_bytes(ctx._ctx) == 0
    finally:
        for ctx in contexts.values():
            ctx.close()


def test_python_refuses_what_is_no_device_tensor(built_library):
    """Context.set_grid_device raises ValueError before the C call for anything that is no torch tensor in device memory"""
    import numpy as np
    import torch
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case("sim_dp_interp")
    grid = gu.golden_grid(mock_args)
    with bl.Context(bl.Params.from_dict(params), device=-2) as ctx:
        for prim in (grid.prim, torch.from_numpy(grid.prim), torch.from_numpy(grid.prim.astype(np.float64))):
            with pytest.raises(ValueError):
                ctx.set_grid_device(grid, prim)
        with pytest.raises(ValueError):
            ctx.set_grid_device(grid, torch.from_numpy(grid.prim), dims="guess")


def test_grid_describes_itself_without_cells():
    """mock.Grid.desc() with prim = None: geometry and indices, eight variables (nine with an entropy index), prim NULL"""
    import dataclasses
    fx, params, mock_args = gu.load_case("sim_multiblock")
    grid = gu.golden_grid(mock_args)
    bare = dataclasses.replace(grid, prim=None)
    a, b = grid.desc(), bare.desc()
    assert b.prim is None and bare.shape == grid.shape
    for field in ("n_blocks", "n_i", "n_j", "n_k", "n_var", "ind_rho", "ind_bb3", "ind_kappa", "x1f", "x3v", "levels", "locations", "n_3_root"):
        assert getattr(a, field) == getattr(b, field), field
    assert dataclasses.replace(bare, ind_kappa=8).desc().n_var == 9 and dataclasses.replace(bare, n_var=11).desc().n_var == 11


def _build(directory, extra):
    """The stand-alone program from its two translation units with the host compiler (the library's headers name HIP types, so the
    HIP headers are on the include path; nothing of HIP is linked)"""
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(bl_build.hipcc()))), "include")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{hip_include}", f"-I{bl_build.INCLUDE}", f"-I{bl_build.CSRC}"]
    sources = [os.path.join(REPO, "tests", "device_grid_host_main.cpp"), os.path.join(bl_build.CSRC, "bl_grid.cpp")]
    program = os.path.join(directory, "device_grid_host_main")
    run = subprocess.run(["g++", "-o", program] + sources + flags + extra, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return program


@pytest.mark.parametrize("sanitized", [False, True])
def test_the_check_alone_plain_and_under_the_sanitizers(tmp_path, sanitized):
    program = _build(str(tmp_path), SANITIZE if sanitized else [])
    lines = "".join(" ".join(str(case[field]) for field in FIELDS) + "\n" for case in CASES.values())
    run = subprocess.run([program], input=lines, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    want = ["ok" if case["want"] is None else f"refused {E_ARG} {case['want']}" for case in CASES.values()]
    assert run.stdout.splitlines() == want, [name for name, got, w in zip(CASES, run.stdout.splitlines(), want) if got != w]
