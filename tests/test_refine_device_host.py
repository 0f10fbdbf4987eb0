"""bl_adaptive_refine_device / Context.adaptive_refine_device where there is no device: a host-only context refuses the call with
BL_E_DEVICE and its text, and the Python method hands nothing to the C call that is not a device tensor. (What the call decides is
held against bl_adaptive_refine on the GPU: test_gpu_refine_device.py.)"""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu

BL_DEVICE_NONE = -2
E_DEVICE = 4
NO_DEVICE = ("Error: Host-only context: no HIP device selected (bl_adaptive_refine_device reads the image in device memory; "
             "bl_adaptive_refine decides on the host).\n")


def _host_context(bl):
    fx, params, _ = gu.load_case("sim_adaptive")
    return bl.Context(bl.Params.from_dict(params), device=BL_DEVICE_NONE), params


def test_a_host_only_context_refuses_the_device_call(built_library):
    import blacklight_amd as bl
    ctx, params = _host_context(bl)
    with ctx:
        res, bs = int(params["camera_resolution"]), int(params["adaptive_block_size"])
        n_blocks = (res // bs) ** 2
        image = np.ones((ctx.num_quantities, res * res))
        flags = np.full(n_blocks, 7, dtype=np.uint8)
        count = C.c_int32(-1)
        rc = ctx._lib.bl_adaptive_refine_device(ctx._ctx, 0, n_blocks, None, image.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                                                C.byref(count), None)
        assert (rc, ctx._lib.bl_last_error(ctx._ctx).decode()) == (E_DEVICE, NO_DEVICE)
        assert count.value == -1 and (flags == 7).all()   # a refused call changes nothing
        # ... and the host call still decides on that context
        got, nxt = ctx.adaptive_refine(0, image)
        assert got.shape == (n_blocks,)


def test_the_python_call_takes_device_tensors_only(built_library):
    import torch
    import blacklight_amd as bl
    ctx, params = _host_context(bl)
    with ctx:
        res = int(params["camera_resolution"])
        rows = ctx.num_quantities
        with pytest.raises(ValueError):
            ctx.adaptive_refine_device(0, np.ones((rows, res * res)))
        with pytest.raises(ValueError):
            ctx.adaptive_refine_device(0, torch.ones((rows, res * res), dtype=torch.float32))
        with pytest.raises(ValueError):
            ctx.adaptive_refine_device(0, torch.ones((rows, res * res), dtype=torch.float64))   # right type, host memory
        with pytest.raises(ValueError):
            ctx.adaptive_refine_device(0, 0, rows=rows, pixels=res * res)                        # a null pointer
