"""GPU tests of the detector's other configurations -- ResNet-18 (BasicBlocks) with and without DCN, ResNet-50 without DCN -- and of
the kernel piece they needed: the residual epilogue of the pipelined deformable convolution (csrc/dcn_pipe.h, RES builds), through
ocrvi_test_deform_conv_res.  References: tests/backbone_refs.py (ResNet-18) and the oracle with dcn=False (ResNet-50)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1, "f16": 2, "f16x2": 3}
# the budgets of tests/test_gpu_kernels.py: max error relative to the output rms
TOL = {"f32": 2e-5, "f16x2": 2e-5, "bf16": 4e-2, "f16": 5e-3}
EXACT = ("f32", "f16x2")
STORE = {"bf16": torch.bfloat16, "f16": torch.float16}


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib


def _rel_err(a, b):
    return float((a - b).abs().max() / (b.pow(2).mean().sqrt() + 1e-12))


# ------------------------------------------------------------------ 1. the kernel
DCN_RES_CASES = [
    # (N, C = Co, H, W, stride)
    (2, 128, 14, 18, 1), (2, 128, 14, 18, 2),     # 128-column tile, ragged patches
    (2, 256, 14, 18, 1),                          # 256-column tile
    (1, 512, 8, 12, 1),                           # two 256-column tiles: the residual's column offset
]


@functools.lru_cache(maxsize=None)
def _dcn_res_case(case):
    """Inputs and the pre-residual fp32 result of one case, computed once for all dtypes (offsets scaled by 3: samples leave the image)."""
    from oracle import dbnet_cpu
    N, C_, H, W, stride = case
    g = torch.Generator().manual_seed(101 + sum(case))
    x = torch.randn(N, C_, H, W, generator=g)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    off = torch.randn(N, 18, Ho, Wo, generator=g) * 3.0
    mask = torch.rand(N, 9, Ho, Wo, generator=g)
    w = torch.randn(C_, C_, 3, 3, generator=g) / np.sqrt(9 * C_)
    b = torch.randn(C_, generator=g) * 0.1
    res = torch.randn(N, C_, Ho, Wo, generator=g)
    pre = dbnet_cpu.deform_conv2d_gather(x, off, mask, w, stride) + b.view(1, -1, 1, 1)
    return x, off, mask, w, b, res, pre


def _run(case, dt, res, relu=1):
    """res: a tensor -> ocrvi_test_deform_conv_res; None -> ocrvi_test_deform_conv."""
    L = _L()
    lib = L.load()
    N, C_, H, W, stride = case
    x, off, mask, w, b, _, pre = _dcn_res_case(case)
    out = torch.empty(pre.shape, device="cuda")
    wh, bh = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    xd, od, md = x.cuda(), off.cuda(), mask.cuda()
    ms = C.c_float(0)
    if res is None:
        L.check(lib.ocrvi_test_deform_conv(0, DT[dt], xd.data_ptr(), od.data_ptr(), md.data_ptr(), wh.ctypes.data, bh.ctypes.data,
                                           N, C_, H, W, C_, stride, relu, out.data_ptr(), 0, C.byref(ms)))
    else:
        rd = res.cuda()
        L.check(lib.ocrvi_test_deform_conv_res(0, DT[dt], xd.data_ptr(), od.data_ptr(), md.data_ptr(), wh.ctypes.data, bh.ctypes.data,
                                               rd.data_ptr(), N, C_, H, W, C_, stride, relu, out.data_ptr(), 0, C.byref(ms)))
    return out.cpu()


def _tol(case, dt):
    # K = 9 C: the fp32 budget grows like sqrt(K) beyond the K ~ 1000 it is sized for (test_deform_conv_kernel_detector_shapes)
    return TOL[dt] * (max(1.0, (9 * case[1] / 1152.0) ** 0.5) if dt in EXACT else 1.0)


@pytest.mark.parametrize("dt", ["f32", "f16x2", "bf16", "f16"])
@pytest.mark.parametrize("case", DCN_RES_CASES)
def test_deform_conv_residual_epilogue(case, dt):
    """relu(deform_conv2d + b + res): against the gather oracle (in the 16-bit modes on res as that type stores it), twice with equal bits,
    and with res = 0 equal to the kernel without a residual."""
    x, off, mask, w, b, res, pre = _dcn_res_case(case)
    res_seen = res.to(STORE[dt]).float() if dt in STORE else res       # the storage rounding of an input is not kernel error
    ref = F.relu(pre + res_seen)
    out = _run(case, dt, res)
    err = _rel_err(out, ref)
    print(f"\n[{dt}] {case}: rel err {err:.3e} (budget {_tol(case, dt):.1e})")
    assert out.shape == ref.shape
    assert err < _tol(case, dt), err
    assert torch.equal(out, _run(case, dt, res))
    assert torch.equal(_run(case, dt, torch.zeros_like(res)), _run(case, dt, None))


@pytest.mark.parametrize("dt", ["f32", "f16x2", "bf16", "f16"])
def test_deform_conv_residual_epilogue_without_relu(dt):
    case = DCN_RES_CASES[1]
    x, off, mask, w, b, res, pre = _dcn_res_case(case)
    ref = pre + (res.to(STORE[dt]).float() if dt in STORE else res)
    out = _run(case, dt, res, relu=0)
    assert float(out.min()) < -0.5                                     # nothing was clamped
    assert _rel_err(out, ref) < _tol(case, dt), _rel_err(out, ref)
    assert torch.equal(_run(case, dt, torch.zeros_like(res), relu=0), _run(case, dt, None, relu=0))


# ------------------------------------------------------------------ 2. the models
MODEL_CONFIGS = [("resnet18", True), ("resnet18", False), ("resnet50", False)]
WIDTHS = {"resnet18": (64, 128, 256, 512), "resnet50": (256, 512, 1024, 2048)}


@functools.lru_cache(maxsize=None)
def _state(backbone, dcn):
    from ocr_vi_invoice_amd import weights
    return weights.make_det_state_dict(seed=21, dcn_offset_std=1.5, backbone=backbone, dcn=dcn)


@functools.lru_cache(maxsize=None)
def _model_case(backbone, dcn, hw):
    """Input and fp32 reference of one configuration and size, computed once for all dtypes."""
    from ocr_vi_invoice_amd import synth
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    H, W = hw
    x = torch.from_numpy(np.stack([synth.normalize_chw(synth.make_invoice(s, H, W, lines=3)[0]) for s in (1, 2)]))
    fwd = R.forward18 if backbone == "resnet18" else R.forward50
    return x, fwd(_state(backbone, dcn), x, dcn=dcn, return_feats=True)


@pytest.mark.parametrize("dt", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(64, 96), (96, 64)])
@pytest.mark.parametrize("backbone,dcn", MODEL_CONFIGS)
def test_dbnet_configurations_match_their_reference(backbone, dcn, hw, dt):
    """The bounds of test_dbnet_f32_matches_oracle, for the configurations it does not cover."""
    from ocr_vi_invoice_amd import DBNetPP
    H, W = hw
    x, ref = _model_case(backbone, dcn, hw)
    m = DBNetPP(backbone=backbone, pretrained=False, dcn=dcn, state_dict=_state(backbone, dcn), dtype=dt)
    feats = m.debug_features(x.cuda())
    for i, k in enumerate(("c2", "c3", "c4", "c5")):
        assert feats[k].shape == (2, WIDTHS[backbone][i], H >> (i + 2), W >> (i + 2)), k
    for k in ("c2", "c3", "c4", "c5", "fused"):
        r = ref[k]
        scale = float(r.abs().max())
        print(f"\n[{backbone} dcn={dcn} {hw} {dt}] {k}: scale {scale:.2f} max-abs-err {float((feats[k].cpu() - r).abs().max()):.2e}")
        np.testing.assert_allclose(feats[k].cpu().numpy(), r.numpy(), atol=2e-4 * max(scale, 1.0), err_msg=k)
    out = m(x.cuda())
    for k in ("binary", "thresh", "thresh_binary"):
        assert out[k].shape == (2, 1, H, W)
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].numpy(), atol=1e-3, err_msg=k)
    for k in ("bin_logits", "thresh_logits"):
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].numpy(), atol=2e-3, rtol=1e-3, err_msg=k)
    only = m.forward(x.cuda(), binary_only=True)
    assert set(only) == {"binary"} and torch.equal(only["binary"], out["binary"])
    assert torch.equal(m.forward_binary(x.cuda()), out["binary"])
    m.check_range()                                                  # (f16x2: no activation left fp16's exponent range)


# The project's budgets for the binary map of the 16-bit modes (test_dbnet_lowp_error_budget: 0.033 / 0.0053, set on ResNet-50 with DCN)
# hold for three of the six new (configuration, type) pairs.  Measured on MI355X, max |binary - fp32 reference| on the page:
#
#   configuration        bf16: library  emulation      f16: library  emulation
#   resnet18, dcn=True         0.0530     0.0481              0.0045    0.0036
#   resnet18, dcn=False        0.0767     0.0700              0.0066    0.0093
#   resnet50, dcn=False        0.0241     0.0321              0.0043    0.0042
#
# "emulation" = tests/backbone_refs.py::forward_lowp_emulation on the CPU: the fp32 reference with the folded weights and every stored
# activation rounded to the 16-bit type, i.e. what 16-bit STORAGE alone costs on these weights (on ResNet-50 with DCN it gives 0.0293 / 0.0037
# where the library measures 0.0218 / 0.0035).  The three pairs over the project's budget are over it in the emulation too -- a BasicBlock adds
# the rounded identity to an output of the same size twice per layer with nothing in between to average it down --, so they are held to
# 1.5 x the emulation's error instead (the library's reduction order and fused epilogues differ from the emulation's), computed here from
# the emulation when the test runs and never from the library's output (on the MI355X host: 0.0715, 0.1015 and 0.0108; the emulation's
# own figure moves a little with the host's summation order, the table's were taken on another host).
EMULATION_BOUND = {("resnet18", True, "bf16"), ("resnet18", False, "bf16"), ("resnet18", False, "f16")}


@pytest.mark.parametrize("dt,tol", [("bf16", 0.033), ("f16", 0.0053)])
@pytest.mark.parametrize("backbone,dcn", MODEL_CONFIGS)
def test_dbnet_configurations_lowp_error_budget(backbone, dcn, dt, tol):
    from ocr_vi_invoice_amd import DBNetPP
    x, ref = _model_case(backbone, dcn, (64, 96))
    x, want = x[:1], ref["binary"][:1]
    if (backbone, dcn, dt) in EMULATION_BOUND:
        emu = R.forward_lowp_emulation(_state(backbone, dcn), x, STORE[dt])["binary"]
        emu_err = float((emu - want).abs().max())
        assert emu_err > tol / 1.5                                   # (else the project's budget would apply)
        tol = 1.5 * emu_err
    out = DBNetPP(backbone=backbone, pretrained=False, dcn=dcn, state_dict=_state(backbone, dcn), dtype=dt)(x.cuda())
    err = float((out["binary"].cpu() - want).abs().max())
    print(f"\n[{backbone} dcn={dcn} {dt}] binary map max-abs-err {err:.4f} mean {float((out['binary'].cpu() - want).abs().mean()):.5f} (budget {tol:.4f})")
    assert err < tol


# ------------------------------------------------------------------ 3. loading
def test_loading_the_wrong_architecture_raises():
    from ocr_vi_invoice_amd import DBNetPP, weights
    L = _L()
    sd50, sd18 = _state("resnet50", False), _state("resnet18", True)
    with pytest.raises(RuntimeError, match="unexpected key .*conv3"):
        DBNetPP(backbone="resnet18", pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f32")
    with pytest.raises(RuntimeError, match="missing key .*conv3"):
        DBNetPP(backbone="resnet50", pretrained=False, state_dict=sd18, dtype="f32")
    with pytest.raises(RuntimeError, match="unexpected key .*offset_mask_conv"):
        DBNetPP(backbone="resnet18", pretrained=False, dcn=False, state_dict=sd18, dtype="f32")        # DCN weights into a dcn=False model
    with pytest.raises(RuntimeError, match="missing key .*offset_mask_conv"):
        DBNetPP(backbone="resnet50", pretrained=False, dcn=True, state_dict=sd50, dtype="f32")
    m = DBNetPP(backbone="resnet18", pretrained=False, dtype="f32", seed=3)                            # seeds matching weights by itself
    assert weights.det_arch(m.state_dict()) == ("resnet18", True)
    with pytest.raises(RuntimeError, match="unexpected key .*conv3"):
        m.load_state_dict(weights.make_det_state_dict(seed=3))
    with pytest.raises(NotImplementedError):
        DBNetPP(backbone="resnet101")
    # the C ABI itself: a ResNet-18 blob under a ResNet-50 cfg (and the other three mismatches) is an argument error naming the tensor
    blob18 = weights.pack_blob(weights.fold_det(sd18))
    blob50 = weights.pack_blob(weights.fold_det(sd50))
    for blob, backbone, no_dcn, word in ((blob18, 0, 0, "layer1.0.conv3.w"), (blob50, 1, 1, "layer1.0.conv3.w"),
                                         (blob18, 1, 1, "layer2.0.conv2.off.w"), (blob50, 0, 0, "layer2.0.conv2.off.w")):
        cfg = L.DetCfg()
        cfg.dtype, cfg.k, cfg.backbone, cfg.no_dcn = 0, 50.0, backbone, no_dcn
        h = C.c_void_p()
        with pytest.raises(ValueError, match=word.replace(".", r"\.")):
            L.check(L.load().ocrvi_det_create(0, blob, len(blob), C.byref(cfg), C.byref(h)))
        assert not h.value
    with pytest.raises(ValueError):
        DBNetPP(backbone="resnet50", pretrained=False, blob=blob18, dtype="f32")


def test_resnet18_checkpoint_style_dict_loads_to_the_same_maps():
    from ocr_vi_invoice_amd import DBNetPP
    sd = _state("resnet18", True)
    x, _ = _model_case("resnet18", True, (64, 96))
    a = DBNetPP(backbone="resnet18", pretrained=False, state_dict=sd, dtype="f32")(x.cuda())
    b = DBNetPP(backbone="resnet18", pretrained=False, state_dict=R.as_reference_checkpoint(sd), dtype="f32")(x.cuda())
    assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ 4. end to end
def test_engine_with_a_resnet18_dcn_detector_equals_detect_and_recognize_per_page():
    """Three small pages of two sizes, f16x2, the smallest configuration tests/test_gpu_engine.py uses (320-pixel detector side, SVTRv2-tiny
    at 32x256); random weights give a map without text structure, so the rendered text boxes are blended in as there."""
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, pipeline, synth, weights
    from ocr_vi_invoice_amd.engine import plan_buckets
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det_size, sizes, seeds = 320, [(1000, 760), (760, 1000), (900, 700)], [11, 13, 12]
    pages, kern = [], []
    shapes, scales, _ = plan_buckets(sizes, det_size)
    for (h, w), seed, (H, W), (sh, sw) in zip(sizes, seeds, shapes, scales):
        img, boxes = synth.make_invoice(seed, h, w, lines=8)
        pages.append(img)
        k = np.zeros((1, H, W), np.float32)
        for x, y, bw, bh in boxes:
            x0, x1, y0, y1 = int(x * sw) + 2, int((x + bw) * sw) - 2, int(y * sh) + 1, int((y + bh) * sh) - 1
            if x1 - x0 >= 3 and y1 - y0 >= 2:
                k[0, y0:y1, x0:x1] = 0.75
        kern.append(torch.from_numpy(k).cuda())
    det = DBNetPP(backbone="resnet18", pretrained=False, dcn=True, state_dict=_state("resnet18", True), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")

    def pp():
        return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)

    det.reset_range()                                                # (the flag is per device and sticky: start from a clear one)
    torch.cuda.synchronize()
    want = []
    for i, p in enumerate(pages):
        def one(x, i=i):
            return {"binary": torch.add(kern[i][None], det(x)["binary"], alpha=0.25)}
        want.append(pipeline.detect_and_recognize(p, one, rec, pp(), "cuda:0", det_size=det_size, rec_size=(32, 256), rec_batch_size=64))
    assert all(len(w[0]) > 0 for w in want)

    def hook(prob, idx):
        torch.add(torch.stack([kern[i] for i in idx]), prob, alpha=0.25, out=prob)

    eng = Engine(det, rec, pp(), det_size=det_size, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=hook)
    got = eng.run(pages)
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(gb, wb)), i
        assert gs == ws and gt == wt, i
    det.check_range()                                                # the f16x2 range flag is clear
    rec.check_range()
    raised = C.c_int(-1)
    _L().check(_L().load().ocrvi_range_flag(0, C.byref(raised)))
    assert raised.value == 0
