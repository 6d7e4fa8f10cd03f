"""GPU: the exponent range of the f16x2 mode (include/ocrvi.h, csrc/common.h).

The reference is fp32 end to end (src/pipeline/pipeline2.py:312-318: 8 exponent bits); f16x2 keeps every GEMM operand as two fp16
halves, so it is only as wide as fp16's exponent.  Pinned here:

* the error law at the kernel level: activations scaled by 2^-12 .. 2^+12 through the ring GEMM and a 3x3 convolution against an fp64
  product of the same fp32 operands.  While |x| >= 2^-3 an element keeps >= 22 bits (relative error <= 2^-23); below that its lo half
  is a subnormal fp16 number and the error is absolute, 2^-25 per element, i.e. 2^-25 / rms(x) relative to the output.  Weights carry
  their own power-of-two scale per layer (ConvParams::wscale), so scaling them changes nothing;
* the supported range that follows from it: rms(x) in [2^-8, 2^+12] keeps the fp32 modes' 2e-5 budget (4e-5 at the lower edge);
* the upper edge is LOUD: a value with |x| >= 65520 raises the device's range flag wherever it is packed (input cast, GEMM epilogue,
  LayerNorm output), *_forward hands the flag to the handle without synchronising, ocrvi_{det,rec}_status return OCRVI_ERANGE and the
  facades raise OverflowError at the point where they synchronise anyway;
* the same at the model level: one layer of SVTRv2 driven to 2^-10 .. 2^+10 (LayerNorm affine scaled, the following Linear scaled back)
  stays within 1e-3 of the exact-fp32 mode's log-probs; driven past 65520 it raises.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1, "f16": 2, "f16x2": 3}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _flag():
    L = _L()
    v = C.c_int(0)
    L.check(L.load().ocrvi_range_flag(0, C.byref(v)))
    return v.value


def _reset():
    L = _L()
    L.check(L.load().ocrvi_range_reset(0, None))
    torch.cuda.synchronize()


def _gemm(a, w, b, dt, out_f32=1):
    L = _L()
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), device="cuda")
    ms = C.c_float(0)
    ad = a.cuda()
    wh, bh = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    L.check(L.load().ocrvi_test_gemm(0, DT[dt], ad.data_ptr(), wh.ctypes.data, bh.ctypes.data, None, M, K, N, 0, 0, out_f32, out.data_ptr(), 0,
                                     C.byref(ms)))
    return out.cpu()


def _law(scale_log2):
    """max |error| / rms(output) allowed for activations of rms 2^scale_log2: the fp32 modes' budget while every element keeps its
    22 bits, 5 x (2^-25 / rms(x)) -- five standard deviations of a sum of uniform +-2^-25 element errors -- below that."""
    s = 2.0 ** scale_log2
    return max(2e-5, 5.0 * 2.0 ** -25 / s)


@pytest.mark.parametrize("e", [-12, -10, -8, -4, 0, 4, 8, 12])
def test_ring_gemm_error_law_over_the_activation_range(e):
    _reset()
    g = torch.Generator().manual_seed(100 + e)
    M, K, N = 9000, 384, 384
    a = torch.randn(M, K, generator=g) * 2.0 ** e
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.zeros(N)
    ref = (a.double() @ w.double().t())
    rms = float(ref.pow(2).mean().sqrt())
    got = _gemm(a, w, b, "f16x2")
    err = float((got.double() - ref).abs().max()) / rms
    exact = float((_gemm(a, w, b, "f32").double() - ref).abs().max()) / rms
    print(f"\n[2^{e}] f16x2 max err / rms {err:.2e} (law {_law(e):.2e}); exact-fp32 mode {exact:.2e}")
    assert err < _law(e), (e, err)
    if -8 <= e:
        assert err < 4e-5          # the supported range: the fp32 modes' budget (2e-5) up to the 2^-8 edge's factor of two
    assert exact < 2e-5            # (the exact mode does not care)
    assert _flag() == 0            # nothing left fp16's range: max |a| = 5 sigma * 2^12 < 65520
    # a weight scale changes nothing: the packer normalises every layer by a power of two
    got_w = _gemm(a, w * 2.0 ** 9, b, "f16x2")
    assert float((got_w.double() / 2.0 ** 9 - ref).abs().max()) / rms < _law(e)


@pytest.mark.parametrize("e", [-10, 0, 10])
def test_conv3x3_error_law_over_the_activation_range(e):
    L = _L()
    _reset()
    g = torch.Generator().manual_seed(7 + e)
    x = torch.randn(2, 128, 24, 40, generator=g) * 2.0 ** e
    w = torch.randn(128, 128, 3, 3, generator=g) / np.sqrt(9 * 128)
    b = torch.zeros(128)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    out = torch.empty(ref.shape, device="cuda")
    wh, bh = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    ms = C.c_float(0)
    xd = x.cuda()
    L.check(L.load().ocrvi_test_conv(0, DT["f16x2"], xd.data_ptr(), wh.ctypes.data, bh.ctypes.data, 2, 128, 24, 40, 128, 3, 1, 1, 1, 0, out.data_ptr(), 0,
                                     C.byref(ms)))
    err = float((out.cpu().double() - ref).abs().max() / ref.pow(2).mean().sqrt())
    print(f"\n[2^{e}] conv3x3 f16x2 max err / rms {err:.2e} (law {_law(e):.2e})")
    assert err < _law(e) and _flag() == 0


def test_out_of_range_input_and_output_raise_the_flag():
    g = torch.Generator().manual_seed(3)
    M, K, N = 4000, 256, 256
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = torch.zeros(N)
    # (1) an input element fp16 cannot carry: caught where it is packed (the cast in front of the GEMM)
    _reset()
    a = torch.randn(M, K, generator=g)
    a[1234, 17] = 70000.0
    _gemm(a, w, b, "f16x2")
    assert _flag() == 1
    _reset()
    assert _flag() == 0
    # (2) inputs in range, OUTPUT out of range: the ring GEMM's epilogue packs f16x2 when the output is not fp32
    a = torch.randn(M, K, generator=g) * 2.0 ** 10
    out = _gemm(a, w * 2.0 ** 7, b, "f16x2", out_f32=0)          # output rms 2^17
    assert _flag() == 1
    assert not torch.isfinite(out).all()                          # what the flag is there to announce
    _reset()
    # (3) the same product with an fp32 output is representable and raises nothing; nor does anything in the other modes
    ok = _gemm(a, w * 2.0 ** 7, b, "f16x2", out_f32=1)
    assert torch.isfinite(ok).all() and _flag() == 0
    _gemm(a, w * 2.0 ** 7, b, "f32")
    assert _flag() == 0
    # (4) the largest representable magnitude passes: 65504 = fp16 max, 65519.9 still rounds to it
    a = torch.randn(M, K, generator=g)
    a[7, 7], a[8, 8] = 65504.0, -65519.0
    _gemm(a, w, b, "f16x2")
    assert _flag() == 0


def _scaled_block_sd(sd, s):
    """SVTRv2 state_dict with the MLP input of stage 0 / block 0 driven to rms ~ s: norm2's affine (svtrv2.py:95,100) times s, fc1's
    weight (svtrv2.py:30) divided by s -- the same function in exact arithmetic."""
    out = {k: v.clone() for k, v in sd.items()}
    out["stages.0.blocks.0.norm2.weight"] *= s
    out["stages.0.blocks.0.norm2.bias"] *= s
    out["stages.0.blocks.0.mlp.fc1.weight"] /= s
    return out


@pytest.mark.parametrize("e", [-10, -6, 6, 10])
def test_model_level_activation_scale_keeps_the_parity_bar(e):
    from ocr_vi_invoice_amd import SVTRv2, synth, weights
    sd = weights.make_rec_state_dict("tiny", seed=3)
    x = torch.from_numpy(synth.pad_crop_batch(synth.make_crops(5, 4, height=32, max_width=128), 32, 128)).cuda()
    base = SVTRv2("tiny", state_dict=sd, dtype="f32")(x)
    sds = _scaled_block_sd(sd, 2.0 ** e)
    ref = SVTRv2("tiny", state_dict=sds, dtype="f32")(x)
    assert float((ref - base).abs().max()) < 1e-3                                    # the rescaled model IS the same function
    m = SVTRv2("tiny", state_dict=sds, dtype="f16x2")
    m.reset_range()
    lp = m(x)
    m.check_range()                                                                  # in range: no error
    err = float((lp - ref).abs().max())
    print(f"\n[2^{e}] f16x2 vs f32 mode log-probs: max |d| {err:.2e}")
    assert err < 1e-3 and m.decode_probs(lp) == m.decode_probs(ref)


def test_model_level_overflow_is_reported_not_swallowed():
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, synth, weights
    sd = weights.make_rec_state_dict("tiny", seed=3)
    x = torch.from_numpy(synth.pad_crop_batch(synth.make_crops(5, 4, height=32, max_width=128), 32, 128)).cuda()
    bad = SVTRv2("tiny", state_dict=_scaled_block_sd(sd, 2.0 ** 17), dtype="f16x2")    # LayerNorm output ~ 2^17 > 65504
    bad.reset_range()
    lp = bad(x)                                                                      # forward itself never synchronises or raises
    with pytest.raises(OverflowError, match="65520"):
        bad.check_range()
    with pytest.raises(OverflowError):
        bad.decode_greedy(x)                                                         # the decode path checks where it waits for the ids
    # the exact-fp32 mode runs the same weights without complaint, and a healthy f16x2 model is clean again after the reset
    SVTRv2("tiny", state_dict=_scaled_block_sd(sd, 2.0 ** 17), dtype="f32")(x)
    good = SVTRv2("tiny", state_dict=sd, dtype="f16x2")
    good.reset_range()
    assert len(good.decode_greedy(x)) == 4
    good.check_range()
    del lp
    # detector: an input pixel value past fp16's range (a broken normalisation upstream) is caught by the first layout kernel
    det = DBNetPP(pretrained=False, dtype="f16x2", seed=3)
    det.reset_range()
    xi = torch.zeros(1, 3, 64, 96, device="cuda")
    det(xi)
    det.check_range()
    xi[0, 1, 5, 5] = 1e5
    det(xi)
    with pytest.raises(OverflowError):
        det.check_range()
    det.reset_range()


# ---------------------------------------------------------------------------------------------------------------------------------------
# One test per remaining f16x2 writer.  include/ocrvi.h promises that EVERY kernel that writes f16x2 elements raises the flag when it
# packs |x| >= 65520; each writer carries its own copy of the check, and the pointer to the flag word is a per-translation-unit device
# variable (a silent no-op in a unit that forgot OCRVI_RANGE_FLAG_TU()).  Per writer, with inputs that are themselves in range: the flag
# stays 0 at ordinary scale, is 1 when the OUTPUT passes 65520 (activation x 2^10, weight x 2^7, as case (2) above), and stays 0 for the
# same call in f32.  Not covered: the ring GEMM's 3x3 mode is 16-bit only (gemm_ring_eligible: esz == 2), so no f16x2 shape selects it.
# conv_gemm's generic store4 path (RES_UP2 / pixel-shuffle stores, unaligned rows), which ocrvi_test_conv's 16-byte aligned rows never
# take, is reached through ocrvi_test_conv_res with a half-resolution residual on a 1x1 whose 80 input channels keep it off the ring
# (test_res_up2_output_overflow_raises_the_flag), and the ring GEMM's own RES_UP2 epilogue by the same call at 64 channels.
from test_gpu_conv_epilogues import run_conv_res                     # noqa: E402
from test_gpu_kernels import _run_dcn, _run_stem_pool, run_conv      # noqa: E402


def _three_calls(run):
    """run(dt, activation scale, weight scale) -> output tensor(s)."""
    _reset()
    out = run("f16x2", 1.0, 1.0)
    assert _flag() == 0 and torch.isfinite(out).all()
    _reset()
    out = run("f16x2", 2.0 ** 10, 2.0 ** 7)
    assert _flag() == 1, "output past 65520 packed without raising the range flag"
    _reset()
    out = run("f32", 2.0 ** 10, 2.0 ** 7)
    assert _flag() == 0 and torch.isfinite(out).all() and float(out.abs().max()) > 65520.0
    _reset()


@pytest.mark.parametrize("case", [
    # conv_gemm, LDS-staged tile store (epi_lds: 16-byte aligned NHWC rows), 128-column tile: 3x3 / stride 2 is neither halo- nor ring-eligible
    (2, 64, 24, 32, 128, 3, 2, 1),
    # conv_gemm, the same store from the 32-column tile: a grouped 3x3 (N_g = 32 per group)
    (2, 128, 12, 20, 128, 3, 1, 4),
    # conv_gemm AM_CONV1: a 1x1 whose 48 input channels are not whole 32-channel K-steps (the ring needs Cin % 32 == 0)
    (2, 48, 12, 20, 128, 1, 1, 1),
])
def test_conv_gemm_output_overflow_raises_the_flag(case):
    N, Cin, H, W, Co, ks, st, groups = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin // groups, ks, ks, generator=g) / np.sqrt(Cin // groups * ks * ks)
    b = torch.zeros(Co)
    _three_calls(lambda dt, sa, sw: run_conv(x * sa, w * sw, b, ks, st, st, groups, 0, dt))


@pytest.mark.parametrize("case", [
    # conv_gemm AM_CONV1, 128 x 128 tile, the generic per-lane store (RES_UP2 clears epi_lds): packs through common.h's store4
    (3, 80, 10, 14, 256),
    # the ring GEMM (128-row tiles) with the half-resolution residual read in load_group: its own f16x2 epilogue pack
    (3, 64, 10, 14, 256),
])
def test_res_up2_output_overflow_raises_the_flag(case):
    N, Cin, H, W, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 1, 1, generator=g) / np.sqrt(Cin)
    res = torch.randn(N, Co, H // 2, W // 2, generator=g)          # in range at every scale: only the sum leaves it
    _three_calls(lambda dt, sa, sw: run_conv_res(x * sa, w * sw, torch.zeros(Co), res, 1, 2, 0, dt))


def test_conv3_halo_output_overflow_raises_the_flag():
    N, Cin, H, W, Co = 3, 256, 12, 16, 256          # HALO_CASES: neck.fpn[2]
    g = torch.Generator().manual_seed(21)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / np.sqrt(9 * Cin)
    _three_calls(lambda dt, sa, sw: run_conv(x * sa, w * sw, torch.zeros(Co), 3, 1, 1, 1, 0, dt))


def test_dcn_pipe_output_overflow_raises_the_flag():
    g = torch.Generator().manual_seed(22)
    N, C_, H, W = 2, 128, 14, 18
    x = torch.randn(N, C_, H, W, generator=g)
    off = torch.randn(N, 18, H, W, generator=g) * 3.0
    mask = torch.rand(N, 9, H, W, generator=g)
    w = torch.randn(C_, C_, 3, 3, generator=g) / np.sqrt(9 * C_)
    _three_calls(lambda dt, sa, sw: _run_dcn(x * sa, off, mask, w * sw, torch.zeros(C_), 1, dt))


def test_stem_pool_output_overflow_raises_the_flag():
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 3, 36, 52, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    b = torch.zeros(64)
    # (the fused kernel is the f16x2 form; f32 runs the conv + max-pool pair)
    _three_calls(lambda dt, sa, sw: _run_stem_pool(x * sa, w * sw, b, dt, dt == "f16x2")[0])


@pytest.mark.parametrize("D", [128, 384])
def test_mlp_x2_hidden_and_xn_overflow_raise_the_flag(D):
    """mlp_x2.hip packs twice: the hidden activations gelu(fc1(..)) it feeds to fc2, and the xn output.  (No f32 call: the fused MLP has no
    f32 form, ocrvi_test_mlp rejects it.)"""
    L = _L()
    g = torch.Generator().manual_seed(24 + D)
    M = 200
    x = torch.randn(M, D, generator=g)
    lg, lb = torch.ones(D), torch.zeros(D)
    w1, b1 = torch.randn(4 * D, D, generator=g) * np.sqrt(2.0 / D), torch.zeros(4 * D)
    w2, b2 = torch.randn(D, 4 * D, generator=g) * np.sqrt(0.5 / (4 * D)), torch.zeros(D)
    ng, nb = torch.ones(D), torch.zeros(D)

    def run(w1s, ngs):
        h = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float32)
        arrs = [h(lg), h(lb), h(w1 * w1s), h(b1), h(w2), h(b2), h(ng * ngs), h(nb)]
        xdev = x.cuda().clone()
        xn = torch.zeros((M, D), device="cuda")
        L.check(L.load().ocrvi_test_mlp(0, DT["f16x2"], xdev.data_ptr(), *[a.ctypes.data for a in arrs], 1, M, D, xn.data_ptr(), 0, None))
        return xdev.cpu(), xn.cpu()

    _reset()
    xo, xn = run(1.0, 1.0)
    assert _flag() == 0 and torch.isfinite(xo).all() and torch.isfinite(xn).all()
    _reset()
    run(2.0 ** 17, 1.0)                                   # hidden activations ~ 2^17
    assert _flag() == 1, "hidden activation past 65520 packed without raising the range flag"
    _reset()
    xo, _ = run(1.0, 2.0 ** 17)                           # xn = LayerNorm(x_new) * 2^17; the fp32 residual stream itself is fine
    assert _flag() == 1 and torch.isfinite(xo).all(), "xn past 65520 packed without raising the range flag"
    _reset()


@pytest.mark.parametrize("D", [128, 384, 1024])
def test_layernorm_output_overflow_raises_the_flag(D):
    from test_gpu_aux_kernels import run_layernorm
    g = torch.Generator().manual_seed(25)
    x = torch.randn(100, D, generator=g)
    gamma, beta = torch.ones(D), torch.zeros(D)
    _reset()
    assert torch.isfinite(run_layernorm(x, gamma, beta, "f16x2", 1, 0)).all() and _flag() == 0
    run_layernorm(x, gamma * 2.0 ** 17, beta, "f16x2", 1, 0)
    assert _flag() == 1
    _reset()
    assert torch.isfinite(run_layernorm(x, gamma * 2.0 ** 17, beta, "f16x2", 1, 1)).all() and _flag() == 0      # fp32 output: representable
    assert torch.isfinite(run_layernorm(x, gamma * 2.0 ** 17, beta, "f32", 1, 0)).all() and _flag() == 0
    _reset()


def test_convex_and_max_writers_do_not_raise_at_the_largest_fp16_magnitude():
    """Attention, FRM vertical, max-pool and ASF output convex combinations or maxima of in-range inputs and cannot overflow: with the
    blended / pooled values AT +-65504 the flag stays 0 and the output is finite (no false positive at the edge)."""
    from test_gpu_aux_kernels import run_asf, run_frm, run_maxpool
    L = _L()
    g = torch.Generator().manual_seed(26)
    BIG = 65504.0

    def edge(out, what):
        assert _flag() == 0, what + ": false positive"
        assert torch.isfinite(out).all(), what
        assert BIG * (1 - 1e-3) <= float(out.abs().max()) < 65520.0, (what, float(out.abs().max()))
        _reset()

    _reset()
    for B, N, heads in ((2, 100, 4), (1, 640, 2)):        # one pass, and the key-chunk merge of > 512 keys
        D = heads * 32
        qkv = torch.randn(B, N, 3 * D, generator=g)
        sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
        qkv[:, :, 2 * D:] = sign * BIG                    # v: every key holds +-65504 in every channel
        qkv[:, :, 2 * D + 1::2] = torch.randn(B, N, D // 2, generator=g) * 1000.0
        out = torch.empty((B, N, D), device="cuda")
        qd = qkv.cuda()
        L.check(L.load().ocrvi_test_attention(0, DT["f16x2"], qd.data_ptr(), B, N, heads, out.data_ptr(), 0, None))
        edge(out.cpu(), f"attention N={N}")
    for H in (1, 3, 8):
        B, W, D = 2, 40, 128
        kv = torch.randn(B * H * W, 2 * D, generator=g)
        kv[:, D:] = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0) * BIG
        edge(run_frm(kv, torch.randn(D, generator=g), B, H, W, D, "f16x2"), f"frm H={H}")
    x = torch.randn(2, 64, 17, 23, generator=g) * 1000.0
    x[torch.rand(x.shape, generator=g) < 0.05] = BIG
    x[torch.rand(x.shape, generator=g) < 0.05] = -BIG
    x[:, 3] = -BIG                                        # a channel whose every maximum is -65504
    edge(run_maxpool(x, "f16x2"), "maxpool")
    ps = [torch.relu(torch.randn(1, 256, 56 >> l, 40 >> l, generator=g)) for l in range(4)]
    for p in ps:
        p[:, 8:16] = BIG
        p[:, 16:24] = -BIG
    w = torch.randn(4, 1024, generator=g) * (4.0 / 1024) ** 0.5
    edge(run_asf(ps, w, torch.zeros(4), "f16x2"), "asf")
