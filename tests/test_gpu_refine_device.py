"""bl_adaptive_refine_device (bl_refine_kernel, csrc/bl_refine.hip) against bl_adaptive_refine, the host call the reference's goldens and
a numpy restatement hold (test_host_steps.py, test_refinement_sweep.py). One source computes the criteria for both (csrc/bl_refine.h),
so there is no tolerance anywhere: flags and next lists are equal or the test fails. Random draws over the parameter space; the block
sizes at which the kernel maps blocks to lanes differently; the edges of the decision, each with the flags written out; what the call
refuses; the whole adaptive loop in device memory against the loop through the host; and the kernel behind the caller's stream."""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

CRITERIA = ("val", "abs_grad", "rel_grad", "abs_lapl", "rel_lapl")
E_UNSUPPORTED, E_ARG = 3, 5
NOT_DEVICE = ("Error: bl_adaptive_refine_device: image must be device memory of the context's device that holds the examined row to its end inside one "
              "allocation; an image in host memory goes through bl_adaptive_refine.")
ONE_PIXEL = ("Error: bl_adaptive_refine_device: with adaptive_block_size = 1 a gradient criterion reads the pixel beside its one-pixel block, outside "
             "the block (as bl_adaptive_refine and the reference do): there is no defined result to reproduce.")
TWO_MODELS = "Error: bl_adaptive_refine reads one image: not with two or more electron models (bl_set_electron_models)."


def _params(case="sim_adaptive", on=CRITERIA, **over):
    """The fixture's parameters without its regions, the criteria of `on` switched on with frac 0.25 (the others off), then `over`."""
    fx, params, _ = gu.load_case(case)
    for key in [k for k in params if k.startswith("adaptive_region_")]:
        params.pop(key)
    params["adaptive_num_regions"] = 0
    for name in CRITERIA:
        params[f"adaptive_{name}_frac"] = 0.25 if name in on else -1.0
    params.update(over)
    return params


def _upload(image):
    tensor = torch.from_numpy(np.ascontiguousarray(image)).to("cuda")
    torch.cuda.synchronize()   # (the library decides on streams of its own: the caller has synchronised)
    return tensor


def _both(ctx, level, image, locs=None):
    """The host's (flags, next) after holding the device call's to them"""
    want_flags, want_next = ctx.adaptive_refine(level, image, locs)
    flags, nxt = ctx.adaptive_refine_device(level, _upload(image), locs)
    assert flags.dtype == want_flags.dtype and np.array_equal(flags, want_flags), (level, np.flatnonzero(flags != want_flags)[:8])
    assert nxt.dtype == want_next.dtype and np.array_equal(nxt, want_next), level
    return want_flags, want_next


# ------------------------------------------------------------------ 1. random draws
def _draw(seed):
    rng = np.random.default_rng(52000 + seed)
    polarized = seed % 2 == 1          # both row layouts ...
    kind = (seed // 2) % 4             # ... and every image kind, by construction
    bs = int(rng.choice([2, 3, 4, 8, 16]))
    res = bs * int(rng.choice([2, 3, 4, 5]))
    n_nu = int(rng.choice([1, 1, 3]))
    over = dict(camera_resolution=res, adaptive_block_size=bs, adaptive_max_level=int(rng.integers(1, 4)), camera_width=float(rng.uniform(8.0, 40.0)),
                image_num_frequencies=n_nu, adaptive_frequency_num=int(rng.integers(1, n_nu + 1)))
    if n_nu > 1:
        over.update(image_frequency_start=1.0e11, image_frequency_end=4.0e11, image_frequency_spacing="log")
    for name, scale in zip(CRITERIA, (1.0, 0.5, 1.0, 0.5, 2.0)):
        over[f"adaptive_{name}_cut"] = float(rng.uniform(0.0, scale))
        over[f"adaptive_{name}_frac"] = float(rng.choice([-1.0, -1.0, 0.0, 0.1, 0.25, 0.5, 0.9]))
    regions = int(rng.choice([0, 0, 1, 2]))
    over["adaptive_num_regions"] = regions
    half = over["camera_width"] / 2.0
    for r in range(1, regions + 1):
        x0, x1 = sorted(rng.uniform(-half, half, 2))
        y0, y1 = sorted(rng.uniform(-half, half, 2))
        over.update({f"adaptive_region_{r}_level": int(rng.integers(0, 3)), f"adaptive_region_{r}_x_min": float(x0), f"adaptive_region_{r}_x_max": float(x1),
                     f"adaptive_region_{r}_y_min": float(y0), f"adaptive_region_{r}_y_max": float(y1)})
    return _params("sim_polarized_adaptive" if polarized else "sim_adaptive", **over), kind, rng


def _image(rng, kind, rows, pixels):
    smooth = np.abs(np.sin(np.linspace(0.0, rng.uniform(1.0, 30.0), pixels) + rng.uniform(0.0, 6.0))) * rng.uniform(0.1, 2.0)
    image = np.stack([smooth * rng.uniform(0.2, 2.0) + rng.uniform(0.0, 0.3) * rng.random(pixels) for _ in range(rows)])
    if kind == 1:
        image[:, rng.random(pixels) < 0.2] = np.nan
    elif kind == 2:
        image[:, rng.random(pixels) < 0.1] = 0.0
        image[:, rng.random(pixels) < 0.05] = np.inf
    elif kind == 3:
        image = image - 0.7   # negative values: the relative criteria divide by sums that pass through zero
        image[:, rng.random(pixels) < 0.5] = np.nan
    return image


@pytest.mark.parametrize("seed", range(48))
def test_random_draws_decide_as_the_host_does(seed, built_library):
    import blacklight_amd as bl
    params, kind, rng = _draw(seed)
    res, bs = int(params["camera_resolution"]), int(params["adaptive_block_size"])
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        rows = ctx.num_quantities
        image, locs = _image(rng, kind, rows, res * res), None
        for level in range(int(params["adaptive_max_level"]) + 1):
            flags, nxt = _both(ctx, level, image, locs)
            if nxt.shape[0] == 0:
                break
            locs = nxt   # (the host's list goes forward: a mismatch shows at the level where it arises)
            image = _image(rng, kind, rows, nxt.shape[0] * bs * bs)


# ------------------------------------------------------------------ 2. shapes
def _mottled(rng, bs, blocks_v, blocks_u):
    """A frame of blocks_v x blocks_u blocks whose amplitude and roughness differ from block to block over decades, so that every
    criterion alone flags some blocks and not others: pixel = a_b (1 + s_b noise)."""
    amplitude = 10.0 ** rng.uniform(-1.5, 1.5, (blocks_v, blocks_u))
    rough = 10.0 ** rng.uniform(-3.0, 0.0, (blocks_v, blocks_u))
    noise = rng.uniform(-0.5, 0.5, (blocks_v * bs, blocks_u * bs))
    return np.kron(amplitude, np.ones((bs, bs))) * (1.0 + np.kron(rough, np.ones((bs, bs))) * noise)


SHAPE_CUTS = dict(adaptive_val_cut=1.0, adaptive_abs_grad_cut=0.05, adaptive_rel_grad_cut=0.05, adaptive_abs_lapl_cut=0.1, adaptive_rel_lapl_cut=0.1)


# bs = 8: a block is exactly one wave; 2: four lanes of a wave, no Laplacian pixel; 3: one Laplacian pixel; 16: exactly a workgroup's
# lanes; 17: strides that end in the middle of a wave; 64: 4096 pixels per block, sixteen strides
@pytest.mark.parametrize("bs,res", [(8, 32), (2, 10), (3, 15), (16, 64), (17, 34), (64, 128)])
@pytest.mark.parametrize("criterion", CRITERIA + ("all",))
def test_block_sizes_at_which_the_mapping_changes(bs, res, criterion, built_library):
    import blacklight_amd as bl
    on = CRITERIA if criterion == "all" else (criterion,)
    params = _params(on=on, camera_resolution=res, adaptive_block_size=bs, adaptive_max_level=1, **SHAPE_CUTS)
    rng = np.random.default_rng(bs * 100 + len(criterion))
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        image = _mottled(rng, bs, res // bs, res // bs).reshape(1, -1)
        flags, _ = _both(ctx, 0, image)
        if bs < 3 and criterion in ("abs_lapl", "rel_lapl"):
            assert not flags.any()            # no interior pixel: 0 / 0 examined, nothing refines
        elif res // bs >= 4:
            assert flags.any() and not flags.all()   # (the case decides something: both verdicts occur)


@pytest.mark.parametrize("n_blocks", [1, 3, 5, 257])
@pytest.mark.parametrize("bs", [4, 16])
def test_refined_levels_with_partly_filled_workgroups(n_blocks, bs, built_library):
    """Level 1 with a shuffled block list: blocks of 16 pixels share a workgroup four at a time (n_blocks = 1, 3, 5, 257 leave its last
    waves without a block), blocks of 256 take one each; a forced region makes the verdict depend on where the list says a block lies."""
    import blacklight_amd as bl
    res = bs * 10
    params = _params(camera_resolution=res, adaptive_block_size=bs, adaptive_max_level=3, camera_width=20.0, adaptive_num_regions=1,
                     adaptive_region_1_level=2, adaptive_region_1_x_min=-6.0, adaptive_region_1_x_max=1.0, adaptive_region_1_y_min=-2.0,
                     adaptive_region_1_y_max=7.0, **SHAPE_CUTS)
    rng = np.random.default_rng(7000 + n_blocks + bs)
    side = 2 * (res // bs)
    chosen = rng.permutation(side * side)[:n_blocks]
    locs = np.stack([chosen // side, chosen % side], axis=1).astype(np.int32)
    blocks = _mottled(rng, bs, n_blocks, 1)                      # block b: rows [b bs, (b + 1) bs) - its bs^2 pixels are one contiguous run
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        flags, nxt = _both(ctx, 1, blocks.reshape(1, -1), locs)
        if n_blocks == 257:
            assert flags.any() and not flags.all()
        # the forced region alone: a flat image refines nowhere else
        flat_flags, _ = _both(ctx, 1, np.ones((1, n_blocks * bs * bs)), locs)
        x = ((locs[:, 1] + 0.5) / side - 0.5) * 20.0
        y = ((locs[:, 0] + 0.5) / side - 0.5) * 20.0
        assert np.array_equal(flat_flags, (x > -6.0) & (x < 1.0) & (y > -2.0) & (y < 7.0))


# ------------------------------------------------------------------ 3. decision edges
def _frame_of_blocks(blocks, bs):
    """blocks: a list of (bs, bs) arrays, a 2 x 2 frame's root blocks in row-major order -> the (1, res^2) image"""
    return np.block([[blocks[0], blocks[1]], [blocks[2], blocks[3]]]).reshape(1, -1)


def _with_exceeding(count, low=0.5, high=2.0):
    block = np.full(16, low)
    block[np.random.default_rng(count).permutation(16)[:count]] = high
    return block.reshape(4, 4)


def test_fractions_at_the_cut_and_blocks_without_a_finite_pixel(built_library):
    """Value criterion alone, cut 1, frac 0.25, four blocks of 16 pixels: none finite (0 / 0 is NaN: not refined); 4 of 16 exceed
    (0.25 > 0.25 is false); 5 of 16 (refined); every pixel equal to the cut (strict >: none exceeds)."""
    import blacklight_amd as bl
    params = _params(on=("val",), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_val_cut=1.0)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        image = _frame_of_blocks([np.full((4, 4), np.nan), _with_exceeding(4), _with_exceeding(5), np.full((4, 4), 1.0)], 4)
        flags, nxt = _both(ctx, 0, image)
        assert flags.tolist() == [False, False, True, False]
        assert nxt.tolist() == [[2, 0], [2, 1], [3, 0], [3, 1]]


def test_a_zero_fraction_infinite_pixels_and_negative_zeros(built_library):
    """frac = 0: no pixel exceeding is 0 / 16 > 0, false; one is enough. Infinite pixels drop out of `examined`: 12 infinite and 4
    finite pixels of which 1 exceeds give 1 / 4 (not 1 / 16, not 13 / 16). -0.0 has the value 0, which exceeds no cut >= 0."""
    import blacklight_amd as bl
    params = _params(on=("val",), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_val_cut=1.0, adaptive_val_frac=0.0)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        image = _frame_of_blocks([_with_exceeding(0), _with_exceeding(1), np.full((4, 4), -0.0), np.full((4, 4), -2.0)], 4)
        flags, _ = _both(ctx, 0, image)
        assert flags.tolist() == [False, True, False, True]
    for frac, want in ((0.25, [False, True, False, False]), (0.2, [True, True, False, False])):
        params = _params(on=("val",), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_val_cut=1.0, adaptive_val_frac=frac)
        with bl.Context(bl.Params.from_dict(params)) as ctx:
            one_of_four, two_of_four = np.full(16, np.inf), np.full(16, -np.inf)
            one_of_four[[0, 5, 10, 15]] = [2.0, 0.5, 0.5, 0.5]
            two_of_four[[3, 6, 9, 12]] = [2.0, 2.0, 0.5, 0.5]
            image = _frame_of_blocks([one_of_four.reshape(4, 4), two_of_four.reshape(4, 4), np.full((4, 4), np.inf), np.full((4, 4), 0.0)], 4)
            flags, _ = _both(ctx, 0, image)
            assert flags.tolist() == want, frac
    # a cut of zero and zeros of both signs: |-0.0| > 0.0 is false
    params = _params(on=("val",), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_val_cut=0.0, adaptive_val_frac=0.0)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        tiny = np.full((4, 4), -0.0)
        tiny[2, 1] = -5.0e-324
        flags, _ = _both(ctx, 0, _frame_of_blocks([np.full((4, 4), -0.0), np.zeros((4, 4)), tiny, np.full((4, 4), -0.0)], 4))
        assert flags.tolist() == [False, False, True, False]


@pytest.mark.parametrize("criterion", ["rel_grad", "rel_lapl"])
def test_relative_criteria_over_a_denominator_of_exactly_zero(criterion, built_library):
    """All zeros: 0 / 0, NaN at every pixel, nothing examined, not refined. A checkerboard of +1 and -1: every sum in a denominator
    is exactly 0 under a non-zero difference - infinite, nothing examined. A block with one row of alternating signs among ones:
    some pixels infinite, the others finite and counted."""
    import blacklight_amd as bl
    params = _params(on=(criterion,), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_rel_grad_cut=0.5,
                     adaptive_rel_lapl_cut=0.5, **{f"adaptive_{criterion}_frac": 0.0})
    checker = np.where((np.add.outer(np.arange(4), np.arange(4)) % 2) == 0, 1.0, -1.0)
    mixed = np.ones((4, 4))
    mixed[1] = [1.0, -1.0, 1.0, -1.0]
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        flags, _ = _both(ctx, 0, _frame_of_blocks([np.zeros((4, 4)), checker, mixed, np.ones((4, 4))], 4))
        assert flags.tolist()[:2] == [False, False] and not flags[3]
        assert flags[2]   # (its finite pixels beside the row of alternating signs exceed 0.5)


def test_a_forced_region_overrides_and_the_last_level_refines_nothing(built_library):
    import blacklight_amd as bl
    params = _params(on=("val",), camera_resolution=8, adaptive_block_size=4, adaptive_max_level=1, adaptive_val_cut=1.0, camera_width=8.0,
                     adaptive_num_regions=1, adaptive_region_1_level=1, adaptive_region_1_x_min=0.5, adaptive_region_1_x_max=3.5,
                     adaptive_region_1_y_min=-3.5, adaptive_region_1_y_max=-0.5)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        flags, nxt = _both(ctx, 0, np.zeros((1, 64)))
        assert flags.tolist() == [False, True, False, False]   # block (v, u) = (0, 1): centre x = +2, y = -2
        # level 1 = adaptive_max_level: all zeros whatever the image and the region say, and nothing is launched
        loud = np.full((1, nxt.shape[0] * 16), 9.0)
        flags, last = _both(ctx, 1, loud, nxt)
        assert not flags.any() and last.shape == (0, 2)


# ------------------------------------------------------------------ 4. refusals
def _refused(ctx, call):
    import blacklight_amd as bl
    with pytest.raises(bl._capi.BlacklightError) as refusal:
        call()
    return refusal.value.code, ctx._lib.bl_last_error(ctx._ctx).decode().strip()


def test_what_the_call_refuses(built_library):
    import blacklight_amd as bl
    params = _params(camera_resolution=16, adaptive_block_size=4, adaptive_max_level=1)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        rows, pixels = ctx.num_quantities, 256
        pinned = ctx.pinned_array((rows, pixels))
        pinned[...] = 1.0
        assert _refused(ctx, lambda: ctx.adaptive_refine_device(0, pinned.ctypes.data, rows=rows, pixels=pixels)) == (E_ARG, NOT_DEVICE)
        pageable = np.ones((rows, pixels))
        assert _refused(ctx, lambda: ctx.adaptive_refine_device(0, pageable.ctypes.data, rows=rows, pixels=pixels)) == (E_ARG, NOT_DEVICE)
        good = _upload(np.ones((rows, pixels)))
        flags, nxt = ctx.adaptive_refine_device(0, good)   # (the context still decides)
        assert flags.shape == (16,)
    # two electron models (which a context takes with adaptive_max_level = 0 only): the host's refusal, word for word
    with bl.Context(bl.Params.from_dict(dict(params, adaptive_max_level=0))) as ctx:
        ctx.set_electron_models([10.0, 40.0])
        good = _upload(np.ones((ctx.num_quantities, 256)))
        assert _refused(ctx, lambda: ctx.adaptive_refine_device(0, good)) == (E_UNSUPPORTED, TWO_MODELS)
        assert _refused(ctx, lambda: ctx.adaptive_refine(0, good.cpu().numpy())) == (E_UNSUPPORTED, TWO_MODELS)
    # a tensor too short for the chosen row: a frame of 4096^2 pixels (128 MiB a row) claimed of a tensor of 1 MiB
    params = _params(camera_resolution=4096, adaptive_block_size=8, adaptive_max_level=1)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        short = torch.zeros(131072, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert _refused(ctx, lambda: ctx.adaptive_refine_device(0, short.data_ptr(), rows=ctx.num_quantities, pixels=4096 * 4096)) == (E_ARG, NOT_DEVICE)
        with pytest.raises(ValueError):
            ctx.adaptive_refine_device(0, short.reshape(1, -1))   # (the tensor's own shape: Python sees it first)
    # one-pixel blocks with a gradient criterion on; with the gradients off they decide as the host does
    for on, text in ((("val", "abs_grad"), ONE_PIXEL), (("rel_grad",), ONE_PIXEL), (("val", "abs_lapl", "rel_lapl"), None)):
        params = _params(on=on, camera_resolution=8, adaptive_block_size=1, adaptive_max_level=1, adaptive_val_cut=1.0)
        with bl.Context(bl.Params.from_dict(params)) as ctx:
            image = np.random.default_rng(3).uniform(0.0, 2.0, (1, 64))
            if text is None:
                flags, _ = _both(ctx, 0, image)
                assert np.array_equal(flags, image[0] > 1.0)
            else:
                assert _refused(ctx, lambda: ctx.adaptive_refine_device(0, _upload(image))) == (E_UNSUPPORTED, text)


# ------------------------------------------------------------------ 5. the loop end to end
@pytest.mark.parametrize("case", ["sim_adaptive", "sim_polarized_adaptive"])
def test_the_adaptive_loop_in_device_memory_is_the_loop_through_the_host(case, built_library):
    import blacklight_amd as bl
    fx, params, mock_args = gu.load_case(case)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(mock_args))
        through_host = ctx.render_adaptive(want_camera=True)
        on_device = ctx.render_adaptive_device(want_camera=True)
        assert len(on_device) == len(through_host) > 1
        for level, (got, want) in enumerate(zip(on_device, through_host)):
            for name in ("image", "sample_num", "sample_flags", "camera_pos", "camera_dir"):
                assert got[name].is_cuda and gu.same_bits(got[name].cpu().numpy(), want[name]).all(), (level, name)
            assert (got["block_locs"] is None and want["block_locs"] is None) or np.array_equal(got["block_locs"], want["block_locs"])
            assert np.array_equal(got["refinement_flags"], want["refinement_flags"]), level


@pytest.mark.parametrize("case", ["sim_adaptive", "sim_polarized_adaptive"])
def test_the_distributed_loop_decides_on_the_device_when_asked(case, built_library):
    """distributed.render_adaptive(refine_on_device=True) over two emulated ranks on the one GPU: the levels it returns are the
    default path's, bit for bit."""
    import blacklight_amd as bl
    from blacklight_amd import distributed as bd
    fx, params, mock_args = gu.load_case(case)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        ctx.set_grid(gu.golden_grid(mock_args))
        want, want_warnings = bd.render_adaptive(ctx, bd.EmulatedComm(2), want_camera=True)
        got, got_warnings = bd.render_adaptive(ctx, bd.EmulatedComm(2), want_camera=True, refine_on_device=True)
        assert got_warnings == want_warnings and len(got) == len(want) > 1
        for level, (a, b) in enumerate(zip(got, want)):
            assert sorted(a) == sorted(b), level
            for name in a:
                if isinstance(b[name], np.ndarray):
                    assert a[name].dtype == b[name].dtype and gu.same_bits(a[name], b[name]).all(), (level, name)
                else:
                    assert a[name] == b[name], (level, name)


# ------------------------------------------------------------------ 6. the caller's stream
def test_the_kernel_waits_for_what_the_caller_queued(built_library):
    """follow_torch_stream(): the tensor is filled by kernels torch has only queued when the call is made - a clone of a 128 MiB
    frame, 128 passes over it that keep the stream busy for milliseconds (each takes the device longer than the host takes to queue
    it, so the queue is still deep when the library's kernel is launched), and the doubling that leaves the final values. The
    decision is the host's on those."""
    import blacklight_amd as bl
    bs, res = 8, 4096
    params = _params(on=("val", "abs_lapl"), camera_resolution=res, adaptive_block_size=bs, adaptive_max_level=1, **SHAPE_CUTS)
    rng = np.random.default_rng(11)
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        final = _mottled(rng, bs, res // bs, res // bs).reshape(1, -1)
        half = _upload(final * 0.5)
        ctx.follow_torch_stream()
        image = half.clone()
        for _ in range(64):
            image.mul_(1024.0)
            image.div_(1024.0)
        image.mul_(2.0)
        flags, nxt = ctx.adaptive_refine_device(0, image)
        torch.cuda.synchronize()
        assert gu.same_bits(image.cpu().numpy(), final).all()
        want_flags, want_next = ctx.adaptive_refine(0, final)
        assert np.array_equal(flags, want_flags) and np.array_equal(nxt, want_next)
        assert want_flags.any() and not want_flags.all()
        # half the values decide otherwise: had the kernel run ahead of the doubling, the flags would differ
        assert not np.array_equal(ctx.adaptive_refine(0, final * 0.5)[0], want_flags)
