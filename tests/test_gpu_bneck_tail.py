"""The fused ResNet-50 layer1 chain of the f16x2 detector (csrc/bneck_tail.h): conv2 3x3 64->64 + ReLU, conv3 1x1 64->256 + identity +
ReLU (y) and the next block's conv1 1x1 256->64 + ReLU (t1') in one launch, through ocrvi_test_bneck_tail.  Checked against the float64
chain in torch on the same fp32 inputs at TOL["f16x2"] (2e-5 x rms of the reference, the project's bound for one f16x2 layer; a CPU
emulation of the f16x2 chain -- operands and stored tensors rounded to hi + lo, fp32 accumulation -- gives 1.5e-6 .. 3.8e-6 at these
shapes), over the whole map and over the border rows and columns alone; against the unfused chain through the existing hooks (held to the
same bound: if IT fails a case, the case is wrong); for run-to-run and batch invariance bit for bit; for the later tiles of a persistent
workgroup (4 x 224 x 224: 784 tiles on <= 256 workgroups); and for the range flag of both stored tensors.  The identity is always a buffer
of its own whose values are unrelated to t1 (the downsample output of layer1.0; the block input elsewhere)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_epilogues import run_conv_res
from test_gpu_kernels import TOL, run_conv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 16), (3, 17, 23), (1, 37, 45), (1, 5, 70)]   # one tile; ragged, several images; ragged; one tile row, ragged last column


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _h(t):
    return np.ascontiguousarray(t.numpy(), dtype=np.float32)


def run_bneck_tail(t1, idn, wb, y_only=False):
    """(y, t1') -- t1' is None for the y-only form; float32 CPU tensors in and out."""
    L = _L()
    w2, b2, w3, b3, w1, b1 = (_h(t) for t in wb)
    N, _, H, W = t1.shape
    td, idd = t1.cuda().contiguous(), idn.cuda().contiguous()
    y = torch.full((N, 256, H, W), float("nan"), device="cuda")
    tn = torch.full((N, 64, H, W), float("nan"), device="cuda")
    L.check(L.load().ocrvi_test_bneck_tail(0, td.data_ptr(), idd.data_ptr(), w2.ctypes.data, b2.ctypes.data, w3.ctypes.data, b3.ctypes.data,
                                           w1.ctypes.data, b1.ctypes.data, N, H, W, 1 if y_only else 0, y.data_ptr(), tn.data_ptr(), 0, None))
    return y.cpu(), (None if y_only else tn.cpu())


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    w2 = torch.randn(64, 64, 3, 3, generator=g) / np.sqrt(9 * 64)
    w3 = torch.randn(256, 64, generator=g) / np.sqrt(64)
    w1 = torch.randn(64, 256, generator=g) / np.sqrt(256)
    b2, b3, b1 = (torch.randn(n, generator=g) * 0.1 for n in (64, 256, 64))
    return w2, b2, w3, b3, w1, b1


def _inputs(shape, seed):
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(N, 64, H, W, generator=g)), torch.relu(torch.randn(N, 256, H, W, generator=g))


def _ref(t1, idn, wb):
    w2, b2, w3, b3, w1, b1 = (t.double() for t in wb)
    t2 = F.relu(F.conv2d(t1.double(), w2, b2, 1, 1))
    y = F.relu(F.conv2d(t2, w3[:, :, None, None], b3) + idn.double())
    return y, F.relu(F.conv2d(y, w1[:, :, None, None], b1))


def _unfused(t1, idn, wb):
    w2, b2, w3, b3, w1, b1 = wb
    t2 = run_conv(t1, w2, b2, 3, 1, 1, 1, 1, "f16x2")
    y = run_conv_res(t2, w3[:, :, None, None].contiguous(), b3, idn, 1, 1, 1, "f16x2")
    return y, run_conv(y, w1[:, :, None, None].contiguous(), b1, 1, 1, 1, 1, 1, "f16x2")


def _errs(out, ref):
    """max error / rms of the reference: over the whole map, and over the border rows and columns alone"""
    H, W = ref.shape[2:]
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    rms = float(ref.pow(2).mean().sqrt()) + 1e-12
    d = (out.double() - ref).abs()
    return float(d.max()) / rms, float(d[:, :, edge].max()) / rms


_CACHE = {}


def _case(shape):
    """inputs, weights, the float64 reference and the fused result of a shape: computed once, shared, never modified"""
    if shape not in _CACHE:
        wb = _weights(11 + sum(shape))
        t1, idn = _inputs(shape, 5 + 3 * sum(shape))
        _CACHE[shape] = (t1, idn, wb, _ref(t1, idn, wb), run_bneck_tail(t1, idn, wb))
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_bneck_tail_matches_float64(shape):
    t1, idn, wb, (ry, rt), (y, tn) = _case(shape)
    ey, et = _errs(y, ry), _errs(tn, rt)
    print("fused y", ey, "t1'", et)
    uy, ut = _unfused(t1, idn, wb)
    eu = _errs(uy, ry) + _errs(ut, rt)
    print("unfused", eu)
    assert max(eu) < TOL["f16x2"], ("the unfused chain misses the bound: the case is wrong", eu)
    assert max(ey) < TOL["f16x2"] and max(et) < TOL["f16x2"], (ey, et)
    # the fused and the unfused chain differ by fp32 rounding (K order) only
    assert float((y - uy).abs().max()) / float(ry.pow(2).mean().sqrt()) < TOL["f16x2"]
    assert float((tn - ut).abs().max()) / float(rt.pow(2).mean().sqrt()) < TOL["f16x2"]
    y2, tn2 = run_bneck_tail(t1, idn, wb)   # no race: a second launch gives the same bits
    assert torch.equal(y, y2) and torch.equal(tn, tn2)


@pytest.mark.parametrize("shape", [(3, 17, 23), (1, 5, 70)])
def test_bneck_tail_y_only(shape):
    """the form of a layer's last block: no phase C; y has the bits of the full form (same arithmetic, another unit stream)"""
    t1, idn, wb, (ry, _), (y, _) = _case(shape)
    yo, none = run_bneck_tail(t1, idn, wb, y_only=True)
    assert none is None
    e = _errs(yo, ry)
    print("y-only", e)
    assert max(e) < TOL["f16x2"], e
    assert torch.equal(yo, y)
    assert torch.equal(yo, run_bneck_tail(t1, idn, wb, y_only=True)[0])


def test_bneck_tail_batch_invariant():
    """N = 3 gives the same bits as three single-image calls (neither the kernel nor the K order depends on n_img or M)."""
    t1, idn, wb, _, (y, tn) = _case((3, 17, 23))
    for i in range(3):
        yi, ti = run_bneck_tail(t1[i:i + 1], idn[i:i + 1], wb)
        assert torch.equal(y[i:i + 1], yi) and torch.equal(tn[i:i + 1], ti), i


def test_bneck_tail_later_tiles_of_a_workgroup():
    """4 x 224 x 224, the four images copies of one: 784 tiles, >= 3 per workgroup on 256 CUs, so the ring runs across tile boundaries
    with the tail units in it.  Every image equals the single-image call bit for bit, and that one meets the float64 bound."""
    wb = _weights(77)
    t1, idn = _inputs((1, 224, 224), 78)
    y1, tn1 = run_bneck_tail(t1, idn, wb)
    ry, rt = _ref(t1, idn, wb)
    ey, et = _errs(y1, ry), _errs(tn1, rt)
    print("224 y", ey, "t1'", et)
    assert max(ey) < TOL["f16x2"] and max(et) < TOL["f16x2"], (ey, et)
    y4, tn4 = run_bneck_tail(t1.expand(4, -1, -1, -1).contiguous(), idn.expand(4, -1, -1, -1).contiguous(), wb)
    for i in range(4):
        assert torch.equal(y4[i], y1[0]) and torch.equal(tn4[i], tn1[0]), i
    yo, _ = run_bneck_tail(t1.expand(4, -1, -1, -1).contiguous(), idn.expand(4, -1, -1, -1).contiguous(), wb, y_only=True)
    for i in range(4):
        assert torch.equal(yo[i], y1[0]), i


def _flag():
    L = _L()
    v = C.c_int(0)
    L.check(L.load().ocrvi_range_flag(0, C.byref(v)))
    return v.value


def _reset():
    L = _L()
    L.check(L.load().ocrvi_range_reset(0, None))
    torch.cuda.synchronize()


def test_bneck_tail_raises_the_range_flag():
    """y passes 65520 where the identity is scaled up (the identity itself stays in range): the flag reports it, for both forms; at
    ordinary scale it stays down.  t1' alone: a conv1 bias that lifts it past the range while y stays ordinary."""
    t1, idn, wb, _, _ = _case((3, 17, 23))
    _reset()
    run_bneck_tail(t1, idn, wb)
    run_bneck_tail(t1, idn, wb, y_only=True)
    assert _flag() == 0
    big = idn.clone()
    big[1, 7, 3, 5] = 65000.0     # in range as an input; + conv3's output (rms ~ 1, here made > 520 by the bias below) passes 65520
    w2, b2, w3, b3, w1, b1 = wb
    b3big = b3.clone()
    b3big[7] = 1000.0
    for y_only in (False, True):
        _reset()
        run_bneck_tail(t1, big, (w2, b2, w3, b3big, w1, b1), y_only=y_only)
        assert _flag() == 1, y_only
    _reset()
    b1big = b1.clone()
    b1big[3] = 70000.0
    run_bneck_tail(t1, idn, (w2, b2, w3, b3, w1, b1big))
    assert _flag() == 1
    _reset()
    assert _flag() == 0
