"""GPU: the column form of adaptive scale fusion for the 4-byte element types (csrc/kernels.hip, asf_blend_col_kernel), through the hook
ocrvi_test_asf against the float64 reference aux_refs.asf_ref.

The kernel computes what belongs to a pixel -- tap rows and weights of the three coarse levels, scores, softmax, the thirteen blend
coefficients -- with one pixel per lane (lane r = row r of a 48-row segment of one column), in groups of ASF_G = 4 rows, and every
pixel's blend then reads its coefficients from its own lane.  What can go wrong in that structure, and what is aimed at it here:

* a coefficient read from a neighbouring lane, or a group offset wrong by one: weights steered so that every pixel's dominant level
  differs from that of the row above and below it, at sizes with fewer rows than a group or a segment (8), a short last segment (48 + 8),
  64 + 8 rows, and two images of two full segments and a partial one;
* negative taps through the mixed-precision fmas: signed inputs at the same sizes;
* coefficients or partial sums leaking between the lanes of a group: changing p2 at ONE pixel must change that output pixel only, bit
  for bit, for a pixel in the middle of a group, at a group's first and last row and at a segment's first and last row;
* results that depend on where a page sits in a batch.

Every side is at most 104, where the suite's plain budget TOL holds with no measured exception (tests/test_gpu_aux_kernels.py:
<= 1.23e-5 against 2e-5 at every size up to (2, 104, 72)).  No element is excluded."""
import functools

import pytest
import torch

import aux_refs as R
from test_gpu_aux_kernels import _asf_inputs, run_asf
from test_gpu_kernels import TOL, _rel_err

pytestmark = pytest.mark.gpu

DTS = ["f32", "f16x2"]
SIZES = [(1, 8, 8), (1, 56, 8), (1, 72, 16), (2, 104, 24)]
POKE_SIZE = (1, 56, 16)
# (row, column): the middle of a group of four rows; a group's first and last row; the first segment's last row and the second segment's
# first row (48 rows per segment); the map's first and last row
POKES = [(5, 3), (8, 0), (11, 15), (47, 6), (48, 9), (0, 7), (55, 12)]


def _row_steered(size, dt, seed):
    """The "steered" construction of tests/test_gpu_aux_kernels.py with the class changing from every row to the next: channel i of p2 is
    the indicator of class (y + x) % 4 == i and only score i sees it, with weight 20."""
    N, H, W = size
    ps, w, b = _asf_inputs(size, "plain", False, dt, seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cls = (yy + xx) % 4
    for i in range(4):
        ps[0][:, i] = (cls == i).float()        # 0 and 1: exact in every element type
        w[:, i] = 0.0
        w[i, i] = 20.0
    return ps, w, b


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("size", SIZES)
def test_asf_col_row_steered_weights(size, dt):
    ps, w, b = _row_steered(size, dt, 11 + sum(size))
    ref, att = R.asf_ref(*ps, w, b)
    win = att.argmax(1)
    for i in range(4):
        share = float((att[:, i] > 0.5).double().mean())
        assert share >= 0.20, (i, share)                           # 0.25 by construction
    assert bool((win[:, 1:] != win[:, :-1]).all())               # every pixel's dominant level differs from the row above
    got = run_asf(ps, w, b, dt)
    err = _rel_err(got.double(), ref)
    print(f"\n[asf col row-steered {size} {dt}] max |err| / rms {err:.3e}")
    assert torch.isfinite(got).all() and err < TOL[dt], err
    assert torch.equal(got, run_asf(ps, w, b, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("size", SIZES)
def test_asf_col_plain_weights_signed_inputs(size, dt):
    ps, w, b = _asf_inputs(size, "plain", True, dt, 23 + sum(size))
    ref, _ = R.asf_ref(*ps, w, b)
    got = run_asf(ps, w, b, dt)
    err = _rel_err(got.double(), ref)
    print(f"\n[asf col signed {size} {dt}] max |err| / rms {err:.3e}")
    assert torch.isfinite(got).all() and err < TOL[dt], err
    assert torch.equal(got, run_asf(ps, w, b, dt))


@functools.lru_cache(maxsize=None)
def _poke_base(dt):
    ps, w, b = _asf_inputs(POKE_SIZE, "plain", True, dt, 41)
    return ps, w, b, run_asf(ps, w, b, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pix", POKES)
def test_asf_col_one_pixel_poke_stays_in_its_pixel(pix, dt):
    """p2 enters only its own pixel's score and blend: with all 256 channels of p2 changed at one pixel, every other output pixel keeps
    its bits."""
    ps, w, b, base = _poke_base(dt)
    y, x = pix
    g = torch.Generator().manual_seed(1000 + 64 * y + x)
    p2 = ps[0].clone()
    p2[0, :, y, x] = R.round_to(torch.randn(256, generator=g) * 2.0 + 0.5, dt)
    got = run_asf([p2] + list(ps[1:]), w, b, dt)
    assert torch.isfinite(got).all()
    same = (got == base).all(1)[0]                                # [H][W]: all 256 channels of the pixel unchanged
    assert not bool(same[y, x]), "the poke did not reach its own pixel"
    same[y, x] = True
    changed = (~same).nonzero().tolist()
    assert not changed, (pix, changed[:8])
    ref, _ = R.asf_ref(p2, *ps[1:], w, b)
    err = _rel_err(got.double(), ref)
    assert err < TOL[dt], err


@pytest.mark.parametrize("dt", DTS)
def test_asf_col_batch_position_independent(dt):
    N, H, W = 3, 56, 16
    ps, w, b = _asf_inputs((N, H, W), "plain", True, dt, 57)
    ps = [p.clone() for p in ps]
    for p in ps:
        p[2] = p[0]                                               # the same page at positions 0 and 2, another one between them
    alone = run_asf([p[:1].contiguous() for p in ps], w, b, dt)
    got = run_asf(ps, w, b, dt)
    assert torch.isfinite(got).all()
    assert torch.equal(got[0], alone[0]) and torch.equal(got[2], alone[0])
    assert not torch.equal(got[1], alone[0])
