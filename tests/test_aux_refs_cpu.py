"""CPU: the float64 references of tests/aux_refs.py, pinned -- against torch.nn.functional in float64, against the oracle on golden inputs,
and (ASF) against the reference-generated golden itself -- so that the GPU kernel tests compare with a known statement of each
operation and not with a third opinion."""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

import aux_refs as R
from ocr_vi_invoice_amd import weights
from oracle import dbnet_cpu, svtrv2_cpu

torch.set_num_threads(min(8, os.cpu_count() or 1))


def test_asf_reference_reproduces_the_golden_fused_map(golden_dir):
    """aux_refs.asf_ref fed the p2..p5 the oracle's FPN half computes from the golden c2..c5 gives the golden's `fused`, at the tolerance
    tests/test_oracle_cpu.py holds the oracle itself to."""
    g = np.load(os.path.join(golden_dir, "det_neckhead.npz"))
    sd = weights.make_det_state_dict(seed=int(g["seed"]))
    feats = [torch.from_numpy(g[k]) for k in ("c2", "c3", "c4", "c5")]
    fused, ps = dbnet_cpu.neck(sd, feats, return_levels=True)
    w = sd["neck.asf.conv_atten.weight"].reshape(4, 1024)
    out, att = R.asf_ref(*ps, w, sd["neck.asf.conv_atten.bias"])
    np.testing.assert_allclose(out.float().numpy(), g["fused"], atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(out.numpy(), fused.double().numpy(), atol=1e-5, rtol=1e-5)
    assert float((att.sum(1) - 1).abs().max()) < 1e-12


def test_bilinear_taps_are_those_of_fp32_interpolate():
    g = torch.Generator().manual_seed(1)
    for (h, w, H, W) in [(4, 4, 8, 8), (7, 5, 56, 40), (23, 30, 184, 240), (1, 1, 8, 8), (6, 1, 48, 8), (12, 41, 96, 328)]:
        p = torch.randn(2, 3, h, w, generator=g)
        want = F.interpolate(p.double(), size=(H, W), mode="bilinear", align_corners=True)
        got = R.bilinear_up_ref(p, H, W)
        # float64 interpolate differs from the fp32-coordinate form by the coordinate's rounding only: 2^-24 * in, times a tap difference
        assert float((got - want).abs().max()) < 2.0 ** -22 * max(h, w) * float(p.abs().max())
        want32 = F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True)
        assert float((got - want32.double()).abs().max()) < 1e-6 * float(p.abs().max())


def test_layernorm_log_softmax_and_maxpool_references_match_torch_in_float64():
    g = torch.Generator().manual_seed(2)
    for D in (4, 132, 1024):
        x = torch.randn(9, D, generator=g) * 1.5 + 0.3
        gm, bt = torch.rand(D, generator=g) * 0.4 + 0.8, torch.randn(D, generator=g) * 0.1
        y, sigma = R.layernorm_ref(x, gm, bt)
        assert float((y - F.layer_norm(x.double(), (D,), gm.double(), bt.double(), 1e-5)).abs().max()) < 1e-12
        assert float((sigma - x.double().std(-1, unbiased=False)).abs().max()) < 1e-12
    const = torch.full((2, 64), 3.25)
    bt = torch.randn(64, generator=g)
    assert torch.equal(R.layernorm_ref(const, torch.ones(64), bt)[0], bt.double().expand(2, 64))
    for Cn in (1, 2, 65, 1024):
        x = torch.randn(3, 5, Cn, generator=g) * 16
        x[0, 0, Cn // 2] = float("-inf")
        want = F.log_softmax(x.double(), -1)
        got = R.log_softmax_ref(x)
        fin = torch.isfinite(want)
        assert torch.equal(fin, torch.isfinite(got)) and torch.equal(got[~fin], want[~fin]) or Cn == 1
        assert float((got[fin] - want[fin]).abs().max()) < 1e-12
    bad = torch.randn(3, 7, generator=g)
    bad[0, 3], bad[1, 5], bad[2] = float("nan"), float("inf"), float("-inf")
    assert torch.isnan(R.log_softmax_ref(bad)).all() and torch.isnan(F.log_softmax(bad.double(), -1)).all()
    assert F.log_softmax(bad, -1).argmax(-1).tolist() == [0, 0, 0]        # what the decode kernels are held to on such rows
    for shape in [(1, 8, 2, 2), (2, 4, 7, 9), (1, 3, 16, 24), (2, 2, 33, 47)]:
        x = torch.randn(*shape, generator=g)
        for t in (x, -x.abs() - 0.5):
            assert torch.equal(R.maxpool_ref(t), F.max_pool2d(t.double(), 3, 2, 1))


def test_frm_vertical_reference_matches_the_oracle_on_a_golden_crop(golden_dir):
    """The vertical cross-attention inside oracle/svtrv2_cpu.frm (its lines for svtrv2.py:236-243), recomputed with the oracle's helpers on
    the golden 48x320 crop batch (H = 3 keys per column), against aux_refs.frm_vertical_ref on the same kv rows and query."""
    g = np.load(os.path.join(golden_dir, "rec_base_48x320.npz"))
    variant = str(g["variant"])
    sd = weights.make_rec_state_dict(variant, seed=int(g["seed"]))
    S = svtrv2_cpu
    with torch.no_grad():
        x, H, W, _ = S.extract_features(sd, torch.from_numpy(g["x"]), variant)
        B, N, D = x.shape
        h = D // 32
        rows = x.reshape(B * H, W, D)
        qkv = S._lin(sd, "frm.h_qkv", S._ln(sd, "frm.h_norm", rows)).reshape(B * H, W, 3, h, 32).permute(2, 0, 3, 1, 4)
        rows = rows + S._lin(sd, "frm.h_proj", S._mhsa(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B * H, W, D))
        rows = rows + S._mlp(sd, "frm.h_mlp", S._ln(sd, "frm.h_norm2", rows))
        xh = rows.reshape(B, H, W, D)
        cols = xh.permute(0, 2, 1, 3).reshape(B * W, H, D)
        tq = sd["frm.select_token"].expand(B, W, -1).reshape(B * W, 1, D)
        q = S._lin(sd, "frm.v_q", S._ln(sd, "frm.v_norm_q", tq)).reshape(B * W, 1, h, 32).permute(0, 2, 1, 3)
        kv = S._lin(sd, "frm.v_kv", S._ln(sd, "frm.v_norm_kv", cols)).reshape(B * W, H, 2, h, 32).permute(2, 0, 3, 1, 4)
        want = S._mhsa(q, kv[0], kv[1]).transpose(1, 2).reshape(B * W, D)
        # the kernel's operands: kv rows in token order h*W + w per image, and the one query vector every column shares
        kv_rows = S._lin(sd, "frm.v_kv", S._ln(sd, "frm.v_norm_kv", xh)).reshape(B * H * W, 2 * D)
        vq = q[0].reshape(D)
    assert H == 3 and float((q - q[:1]).abs().max()) == 0.0
    got = R.frm_vertical_ref(kv_rows, vq, B, H, W, D)
    assert float((got - want.double()).abs().max()) < 2e-6 * float(want.abs().max())


def test_db_and_ctc_collapse_references():
    g = torch.Generator().manual_seed(4)
    bl, tl = torch.randn(64, generator=g) * 4, torch.randn(64, generator=g) * 4
    b, t = R.db_maps_ref(bl, tl)
    assert float((b - torch.sigmoid(bl.double())).abs().max()) == 0.0
    want = torch.reciprocal(1 + torch.exp(-50.0 * (b - t)))          # oracle/dbnet_cpu.head
    assert float((R.db_step_ref(b, t, 50.0) - want).abs().max()) < 1e-15
    am = torch.randint(0, 5, (6, 40), generator=g)
    lp = torch.full((40, 6, 5), -10.0)
    lp.scatter_(2, am.t().unsqueeze(-1), -0.1)
    ids, lens = R.ctc_collapse_ref(am.numpy())
    want_ids = svtrv2_cpu.greedy_ids(lp)
    assert [list(ids[i, :lens[i]]) for i in range(6)] == want_ids and (ids[0, lens[0]:] == -1).all()


def test_f16x2_round_is_what_the_library_packs():
    from ocr_vi_invoice_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(5)
    w = (rng.standard_normal(4096) * np.exp2(rng.integers(-12, 3, 4096))).astype(np.float32)
    dst = np.zeros(4096 * 2, np.float16)
    ws = C.c_float(0)
    L.check(lib.ocrvi_test_pack_f16x2(w.ctypes.data, w.size, dst.ctypes.data, C.byref(ws)))
    scale = np.float32(1.0 / ws.value)                                # a power of two: w * scale is exact
    packed = dst.reshape(-1, 8)
    held = packed[:, :4].astype(np.float32) + packed[:, 4:].astype(np.float32)
    want = R.f16x2_round(torch.from_numpy(w * scale)).numpy().reshape(-1, 4)
    assert np.array_equal(held, want)
    # rounding twice changes nothing, and the error law of include/ocrvi.h holds
    x = torch.from_numpy(w * scale)
    r = R.f16x2_round(x)
    assert torch.equal(R.f16x2_round(r), r)
    # |err| <= max(2^-25, 2^-23 |x|): lo = fp16(x - hi) carries 11 bits of a remainder <= 2^-12 |x| while it is a normal fp16 number and is
    # a multiple of 2^-24 below 2^-14.  (ocrvi.h words this as "2^-23 relative from |x| = 2^-3 up"; in [2^-3, 2^-2) lo can still be
    # subnormal, e.g. x = -0.12743291 is held with 1.96 x 2^-23 relative error, so the absolute term is what holds there.)
    err = (r.double() - x.double()).abs()
    assert bool((err <= torch.clamp(x.double().abs() * 2.0 ** -23, min=2.0 ** -25)).all())
    assert bool((err[x.abs() >= 0.25] <= x.double().abs()[x.abs() >= 0.25] * 2.0 ** -23).all()) and float(err[x.abs() < 0.25].max()) <= 2.0 ** -25
    for dt in ("bf16", "f16", "f32"):
        assert torch.equal(R.round_to(R.round_to(x, dt), dt), R.round_to(x, dt))
