"""GPU: gconv_x2_kernel (csrc/gconv_x2.hip), LocalMixing's grouped 3x3 convolutions in f16x2 on a full-height halo tile, alone through
ocrvi_test_gconv_x2 and inside the recogniser, every element held to the float64 reference of tests/conv_refs.py: equal to it on routed
integer data, within conv_bound on value data.  The kernel has the model's two epilogues: conv1 = act(conv + bias) -> f16x2 and conv2 =
act(conv + bias) + fp32 residual -> fp32.  Every launch writes into a NaN-filled output with 128 guard rows of a NaN payload behind it: all
elements finite, the guard rows untouched.  No element is excluded from any comparison.

  routing       routed_case integers, both epilogues, no activation and ReLU: output == reference.  One tile; W < 16; a last block of one
                pixel; bh = 6 with two blocks per row and a half-empty last tile; odd heights; 4, 8 and 12 groups; a second band of one
                row (H = 13); two bands and two images (H = 16)
  value         value_case on 2x6x80 and 1x7x100, both epilogues x none / ReLU / GELU: err <= conv_bound
  in place      conv2 with the residual buffer as the output buffer: bit-equal to separate buffers
  later tiles   5 different images of 12x40x128 (15 tiles per group) with the workgroups per group capped so that they walk 2 to 5 tiles:
                bit-equal to the uncapped launch (1 tile each), which is held to the bound
  independence  each image of 2x6x80 alone gives the bits it has inside the batch
  range flag    raised by one element of 65536, not by 65280
  plan          the tiling of the shapes above and of the benchmark's two shapes for 256, 304 and 64 CUs (no launch)
  model path    an 8-crop SVTRv2-base forward in f16x2 against a fresh child process with OCRVI_GCONV32=0 (conv_gemm): equal ids, log-probs
                within 1e-4 (the bar of tests/test_gpu_lin_x2.py)

Three products per fragment pair (the lo lo product dropped) hold the bound: the largest err / bound is printed per family.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

DT = "f16x2"
GUARD = 128
X_GUARD = 0x7FA5C3D2
CONV1, CONV2 = (0, None), (1, 1)            # (out_f32, res_post): the two epilogues
WORST = {}
ROUTE_SHAPES = ((1, 128, 4, 16), (1, 128, 1, 5), (1, 128, 2, 33), (2, 128, 6, 80), (1, 128, 5, 81), (1, 128, 7, 100), (1, 256, 4, 16),
                (1, 384, 4, 16), (1, 128, 13, 20), (2, 128, 16, 40))
VALUE_SHAPES = ((2, 128, 6, 80), (1, 128, 7, 100))
LATER = (5, 128, 12, 40)


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return -(-a // b)


def expect_plan(n, Cc, H, W, n_cu, max_wg=0):
    """gconv_x2_plan (csrc/gconv_x2.hip) as ocrvi_test_gconv_x2_plan reports it."""
    groups = Cc // 32
    bh = min(H, 12)
    nbx = min(12 // bh, 4, cdiv(W, 16))
    while nbx > 1 and (bh + 2) * (16 * nbx + 2) > 288:
        nbx -= 1
    by, bx = cdiv(H, bh), cdiv(W, 16 * nbx)
    ntile = n * by * bx
    slots = max(1, 2 * n_cu // groups)
    if max_wg > 0:
        slots = min(slots, max_wg)
    grid = cdiv(ntile, cdiv(ntile, min(ntile, slots)))
    return (bh, nbx, by, bx, ntile, grid, ntile // grid, cdiv(ntile, grid), groups, (bh + 2) * (16 * nbx + 2) * 128 + 9 * 32 * 128)


def plan_of(n, Cc, H, W, n_cu, max_wg=0):
    L = _L()
    plan = (C.c_int32 * 10)()
    L.check(L.load().ocrvi_test_gconv_x2_plan(n, Cc, H, W, n_cu, max_wg, plan))
    return tuple(plan)


def run_x2(x, w, b, res, act, epi, in_place=False, max_wg=0, check=True):
    """One launch: the output as rows [n H W, C] float32 on the GPU."""
    L = _L()
    of, rp = epi
    n, Cc, H, W = x.shape
    M = n * H * W
    raw = torch.full(((M + GUARD) * Cc * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    guard = raw[M * Cc * 4:].view(torch.int32)
    guard.fill_(X_GUARD)
    out = torch.full((n, Cc, H, W), float("nan"), device="cuda")
    xd = x.cuda().contiguous()
    rd = None if res is None else res.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_gconv_x2(0, xd.data_ptr(), wh.ctypes.data, bh.ctypes.data, None if rd is None else rd.data_ptr(), n, Cc, H, W,
                                         act, int(rp or 0), int(of), int(in_place), max_wg, raw.data_ptr(), out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert bool((guard == X_GUARD).all()), "the guard rows behind the output changed"
    if check:
        assert bool(torch.isfinite(out).all()), "an element of the output was not written (or is not finite)"
    return R.rows_of(out).contiguous()


def _bits(t):
    return t.view(torch.int32)


def _case_res(res, epi):
    return res if epi[1] is not None else None


def _hold(out, ref, bound, family, tag):
    q = R.err_ratio(out.cpu(), ref, bound)
    worst = float(q.max())
    print(f"\n[gconv_x2 {family} {tag}] max err / bound {worst:.3f}")
    WORST[family] = max(WORST.get(family, 0.0), worst)
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (family, tag, worst, int(bad.shape[0]), bad[:8].tolist())


def _ref_bound(x, w, b, res, act, epi):
    g = x.shape[1] // 32
    return (R.conv_ref(x, w, b, res, (1, 1), g, act, epi[1] or 0), R.conv_bound(x, w, b, res, (1, 1), g, act, epi[1] or 0, DT, epi[0]))


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[gconv_x2 summary] largest err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("epi", (CONV1, CONV2), ids=("conv1", "conv2"))
@pytest.mark.parametrize("i", range(len(ROUTE_SHAPES)))
def test_routing(i, epi):
    n, Cc, H, W = ROUTE_SHAPES[i]
    assert plan_of(n, Cc, H, W, _n_cu()) == expect_plan(n, Cc, H, W, _n_cu())
    x, w, b, res = R.routed_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, 11 + i, with_res=epi[1] is not None)
    for act in (R.ACT_NONE, R.ACT_RELU):
        out = run_x2(x, w, b, res, act, epi).cpu()
        ref = R.conv_ref(x, w, b, res, (1, 1), Cc // 32, act, epi[1] or 0)
        bad = (out.double() != ref).nonzero()
        assert bad.numel() == 0, (ROUTE_SHAPES[i], epi, act, int(bad.shape[0]), [(r, c, float(out[r, c]), float(ref[r, c])) for r, c in bad[:8].tolist()])


@pytest.mark.parametrize("epi", (CONV1, CONV2), ids=("conv1", "conv2"))
@pytest.mark.parametrize("shape", VALUE_SHAPES)
def test_value(shape, epi):
    n, Cc, H, W = shape
    x, w, b, res = R.value_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, DT, epi[0], 5)
    res = _case_res(res, epi)
    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_GELU):
        out = run_x2(x, w, b, res, act, epi)
        _hold(out, *_ref_bound(x, w, b, res, act, epi), "value", f"{n}x{H}x{W} out_f32 {epi[0]} act {act}")


def test_in_place():
    n, Cc, H, W = (2, 128, 6, 80)
    x, w, b, res = R.value_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, DT, 1, 6)
    apart = run_x2(x, w, b, res, R.ACT_GELU, CONV2)
    inpl = run_x2(x, w, b, res, R.ACT_GELU, CONV2, in_place=True)
    _hold(apart, *_ref_bound(x, w, b, res, R.ACT_GELU, CONV2), "in place", "separate buffers")
    bad = (_bits(apart) != _bits(inpl)).nonzero()
    assert bad.numel() == 0, (int(bad.shape[0]), bad[:8].tolist())


@pytest.mark.parametrize("epi", (CONV1, CONV2), ids=("conv1", "conv2"))
def test_later_tiles(epi):
    """The next tile's halo: fetched into registers before the MFMAs, staged into LDS behind them."""
    n, Cc, H, W = LATER
    x, w, b, res = R.value_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, DT, epi[0], 21)
    res = _case_res(res, epi)
    assert plan_of(n, Cc, H, W, _n_cu())[:8] == (12, 1, 1, 3, 15, 15, 1, 1)
    full = run_x2(x, w, b, res, R.ACT_GELU, epi)
    _hold(full, *_ref_bound(x, w, b, res, R.ACT_GELU, epi), "later", f"out_f32 {epi[0]} uncapped")
    walked = {1}
    for max_wg, (grid, lo, hi) in ((8, (8, 1, 2)), (5, (5, 3, 3)), (4, (4, 3, 4)), (3, (3, 5, 5))):
        assert plan_of(n, Cc, H, W, _n_cu(), max_wg)[5:8] == (grid, lo, hi)
        walked |= {lo, hi}
        out = run_x2(x, w, b, res, R.ACT_GELU, epi, max_wg=max_wg)
        bad = (_bits(out) != _bits(full)).nonzero()
        assert bad.numel() == 0, (epi, max_wg, int(bad.shape[0]), bad[:8].tolist())
    assert walked >= {1, 2, 3, 4}


@pytest.mark.parametrize("epi", (CONV1, CONV2), ids=("conv1", "conv2"))
def test_independent_of_n_img(epi):
    n, Cc, H, W = (2, 128, 6, 80)
    x, w, b, res = R.value_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, DT, epi[0], 7)
    res = _case_res(res, epi)
    both = _bits(run_x2(x, w, b, res, R.ACT_GELU, epi)).reshape(n, H * W, Cc)
    for i in range(n):
        one = _bits(run_x2(x[i:i + 1], w, b, None if res is None else res[i:i + 1], R.ACT_GELU, epi)).reshape(H * W, Cc)
        assert torch.equal(one, both[i]), i


def _flag():
    L = _L()
    v = C.c_int(0)
    L.check(L.load().ocrvi_range_flag(0, C.byref(v)))
    return v.value


def _reset():
    L = _L()
    L.check(L.load().ocrvi_range_reset(0, None))
    torch.cuda.synchronize()


def test_range_flag():
    """Channel 37 at pixel (3, 9) of image 1: 32 centre-tap weights of 1 against activations of 2048 (2040) = 65536 (65280)."""
    n, Cc, H, W = (2, 128, 6, 20)
    w = torch.zeros(Cc, 32, 3, 3)
    w[37, :, 1, 1] = 1.0
    w[5, 0, 0, 0] = 0.5
    b = torch.zeros(Cc)
    try:
        for v, want in ((2048.0, 1), (2040.0, 0)):
            x = torch.ones(n, Cc, H, W)
            x[1, 32:64, 3, 9] = v
            _reset()
            assert _flag() == 0
            out = run_x2(x, w, b, None, R.ACT_NONE, CONV1, check=False).reshape(n, H, W, Cc)
            assert _flag() == want, (v, _flag())
            if not want:
                assert float(out[1, 3, 9, 37]) == 65280.0
    finally:
        _reset()


def test_not_eligible_is_einval():
    """An fp32 output without the residual, and a residual added before the activation, are not the kernel's."""
    n, Cc, H, W = (1, 128, 4, 16)
    x, w, b, res = R.routed_case(n, Cc, H, W, Cc, (1, 1), Cc // 32, 3)
    with pytest.raises(ValueError):
        run_x2(x, w, b, None, R.ACT_NONE, (1, None))
    with pytest.raises(ValueError):
        run_x2(x, w, b, res, R.ACT_RELU, (1, 0))


@pytest.mark.parametrize("n_cu", (256, 304, 64))
def test_plan(n_cu):
    for shape in ROUTE_SHAPES + VALUE_SHAPES + (LATER, (256, 128, 12, 80), (256, 256, 6, 80), (3, 384, 3, 100), (1, 128, 30, 300)):
        for max_wg in (0, 3):
            plan = plan_of(*shape, n_cu, max_wg)
            assert plan == expect_plan(*shape, n_cu, max_wg), (shape, n_cu, max_wg, plan)
            bh, nbx, by, bx, ntile, grid, lo, hi, groups, smem = plan
            assert bh * nbx <= 12 and (bh + 2) * (16 * nbx + 2) <= 288 and 2 * smem <= 160 * 1024 and lo >= 1 and hi - lo <= 1
    # the benchmark's shapes: 12 x 16 and 6 x 32 tiles, equal walks on the MI355X
    assert plan_of(256, 128, 12, 80, 256)[:8] == (12, 1, 1, 5, 1280, 128, 10, 10)
    assert plan_of(256, 256, 6, 80, 256)[:8] == (6, 2, 1, 3, 768, 64, 12, 12)
    assert plan_of(1, 128, 4, 16, n_cu)[:8] == (4, 1, 1, 1, 1, 1, 1, 1)
    assert plan_of(1, 128, 1, 5, n_cu)[:5] == (1, 1, 1, 1, 1)
    assert plan_of(1, 128, 2, 33, n_cu)[:5] == (2, 3, 1, 1, 1)                # 4 x 50 halo pixels
    assert plan_of(3, 384, 3, 100, n_cu)[:5] == (3, 3, 1, 3, 9)               # four blocks per row would need 5 x 66 halo pixels
    assert plan_of(1, 128, 5, 81, n_cu)[:5] == (5, 2, 1, 3, 3)
    assert plan_of(1, 128, 7, 100, n_cu)[:5] == (7, 1, 1, 7, 7)
    assert plan_of(2, 128, 6, 80, n_cu)[:5] == (6, 2, 1, 3, 6)
    assert plan_of(256, 128, 12, 80, 304)[4:8] == (1280, 143, 8, 9) and plan_of(256, 128, 12, 80, 64)[4:8] == (1280, 32, 40, 40)
    assert plan_of(1, 128, 13, 20, n_cu)[:4] == (12, 1, 2, 2)
    assert plan_of(2, 128, 16, 40, n_cu)[:5] == (12, 1, 2, 3, 12)


_CHILD = """
import sys, numpy as np, torch
from ocr_vi_invoice_amd import SVTRv2
x = torch.from_numpy(np.load(sys.argv[1])).cuda()
m = SVTRv2("base", dtype="f16x2", seed=1234)
lp = m(x)
np.save(sys.argv[2], lp.cpu().numpy())
"""


def test_model_path_against_conv_gemm(tmp_path):
    from ocr_vi_invoice_amd import SVTRv2, synth
    x = synth.pad_crop_batch(synth.make_crops(5, 8, height=32, max_width=128), 32, 128)
    np.save(tmp_path / "x.npy", x)
    m = SVTRv2("base", dtype="f16x2", seed=1234)
    lp = m(torch.from_numpy(x).cuda()).cpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OCRVI_GCONV32="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "x.npy"), str(tmp_path / "lp.npy")], env=env, cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    old = torch.from_numpy(np.load(tmp_path / "lp.npy"))
    diff = float((lp - old).abs().max())
    print(f"\n[gconv_x2 model] 8 crops, SVTRv2-base f16x2: max |dlog-prob| vs OCRVI_GCONV32=0 {diff:.2e}; bit-equal {torch.equal(lp, old)}")
    assert diff < 1e-4, diff
    assert torch.equal(lp.argmax(-1), old.argmax(-1))
