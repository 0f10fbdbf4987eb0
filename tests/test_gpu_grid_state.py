"""GPU: one context through a sequence of grids. A merged grid, a mesh through the block lattice, the merged grid again: each render
must be the render of a fresh context, bit for bit - nothing of a grid outlives the next bl_set_grid. A refused description leaves the
context without a grid, and the next good one brings the first image back."""
import re

import numpy as np
import pytest

import golden_util as gu
from test_grid_host import BAD_MESH, _duplicate_block
from test_gpu_table_budgets import MESHES, _mesh

pytestmark = pytest.mark.gpu


def _render(ctx):
    out = ctx.render()
    return out["image"].copy(), out["sample_num"].copy(), out["sample_flags"].copy()


def _same(got, want):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[0].shape == want[0].shape and gu.same_bits(got[0], want[0]).all()


def test_grids_in_turn_on_one_context(built_library):
    import blacklight_amd as bl
    from blacklight_amd import mock
    fx, params, _ = gu.load_case("sim_dp_interp")
    params = dict(params, camera_resolution=16)
    merged = gu.split_grid(mock.generate(n_r=16, n_th=8, n_ph=8), 2, 2, 2)
    grids = dict(merged=merged, mesh=_mesh(*MESHES["36k_64k"][:2]))
    assert grids["mesh"].prim.shape[1] == 288
    fresh = {}
    for name, grid in grids.items():
        with bl.Context(bl.Params.from_dict(params)) as ctx:
            ctx.set_arithmetic("exact")
            ctx.set_grid(grid)
            fresh[name] = _render(ctx)
        image = fresh[name][0]
        assert np.isfinite(image).all() and (image[0] > 0.0).sum() > image.shape[1] // 2
    assert not gu.same_bits(fresh["merged"][0], fresh["mesh"][0]).all()
    with bl.Context(bl.Params.from_dict(params)) as ctx:
        ctx.set_arithmetic("exact")
        for name in ("merged", "mesh", "merged"):
            ctx.set_grid(grids[name])
            _same(_render(ctx), fresh[name])
        with pytest.raises(bl.BlacklightError, match=re.escape(BAD_MESH)):
            ctx.set_grid(_duplicate_block(merged))
        with pytest.raises(bl.BlacklightError, match=re.escape("bl_render called before bl_set_grid.")):
            ctx.render()
        ctx.set_grid(merged)
        _same(_render(ctx), fresh["merged"])
