"""conv3_halo (csrc/conv3_halo.h) reads a unit's fragments one stage ahead, across the unit barrier, the patch-stage switch and the tile
boundary.  Every case of test_gpu_conv3_halo.py gives each workgroup a single tile (one workgroup runs per CU), so a workgroup's second
tile (`t > 0`, `after_epi`, the fragment reads issued ahead of the epilogue's stores) runs only in the full-size tests.  The cases here
cover that path for both column widths and for two column tiles, and Cin = 32: one channel block, where the patch stage switches every nine
units and every unit's look-ahead crosses a stage switch or a tile end.  Checked against a float64 reference, for run-to-run equality,
and -- with a batch of copies of one image -- for equality between a workgroup's first tile and its later ones."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import TOL, run_conv

pytestmark = pytest.mark.gpu

SMALL_CASES = [
    # N, Cin, H, W, Co, act
    (1, 32, 16, 16, 64, 1),      # one tile, one channel block
    (2, 32, 40, 56, 128, 0),     # one channel block, ragged tiles
]
MULTI_TILE_CASES = [
    (4, 64, 224, 224, 64, 1),    # 784 tiles: at least three per workgroup on 256 CUs, 64 columns
    (4, 32, 224, 224, 128, 0),   # the same for 128 columns, one channel block
    (2, 64, 224, 224, 256, 1),   # two column tiles, at least three tiles per workgroup pair
]


@functools.lru_cache(maxsize=None)
def _case(case):
    """(x, w, b, out, float64 reference) of one case, computed once.  The images of a multi-tile case are copies of one image."""
    N, Cin, H, W, Co, act = case
    g = torch.Generator().manual_seed(sum(case) * 11 + 3)
    x = torch.randn(1 if case in MULTI_TILE_CASES else N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    ref = F.relu(ref) if act == 1 else ref
    if case in MULTI_TILE_CASES:
        x = x.expand(N, -1, -1, -1).contiguous()
    out = run_conv(x, w, b, 3, 1, 1, 1, act, "f16x2")
    return x, w, b, out, ref


@pytest.mark.parametrize("case", SMALL_CASES + MULTI_TILE_CASES)
def test_conv3_halo_pipeline_matches_float64(case):
    x, w, b, out, ref = _case(case)
    act = case[5]
    scale = float(ref.pow(2).mean().sqrt()) + 1e-12
    for i in range(out.shape[0]):
        r = ref[i if ref.shape[0] > 1 else 0]
        err = float((out[i].double() - r).abs().max()) / scale
        print(f"case {case} image {i}: whole-map error {err:.3e}")
        assert err < TOL["f16x2"], (i, err)
        # every border row and column (where the patch's zero halo is read)
        H, W = x.shape[2:]
        edge = torch.zeros(H, W, dtype=torch.bool)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        e2 = float((out[i][:, edge].double() - r[:, edge]).abs().max()) / scale
        assert e2 < TOL["f16x2"], (i, e2)
    assert torch.equal(out, run_conv(x, w, b, 3, 1, 1, 1, act, "f16x2"))   # no race: a second launch gives the same bits


@pytest.mark.parametrize("case", MULTI_TILE_CASES)
def test_conv3_halo_later_tiles_equal_the_first(case):
    """All images are copies of one: every image of the output must equal the single-image call bit for bit (196 tiles: with one column
    tile that is one per workgroup, `t == 0` only), whichever tile of its workgroup computed it.  A fragment read too early or from the wrong stage differs here."""
    x, w, b, out, _ = _case(case)
    single = run_conv(x[:1], w, b, 3, 1, 1, 1, case[5], "f16x2")
    for i in range(out.shape[0]):
        assert torch.equal(out[i], single[0]), i
