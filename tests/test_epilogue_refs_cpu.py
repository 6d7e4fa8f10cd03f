"""CPU: the float64 references of tests/epilogue_refs.py, pinned -- against torch.nn.functional in float64 and against the head of
oracle/dbnet_cpu.py on a generated state dict -- and the claims tests/test_gpu_conv_epilogues.py makes about its integer inputs, so that
the GPU tests compare with a known statement of each epilogue and not with a third opinion."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import epilogue_refs as R
from ocr_vi_invoice_amd import weights
from oracle import dbnet_cpu

torch.set_num_threads(min(8, os.cpu_count() or 1))


def test_conv_res_reference_matches_torch_in_float64():
    for i, (N, Ci, H, W, Co, k) in enumerate([(2, 8, 6, 10, 12, 1), (1, 5, 4, 2, 4, 1), (2, 6, 7, 5, 8, 3), (1, 16, 12, 22, 8, 1)]):
        for mode in (R.RES_SAME, R.RES_UP2):
            if mode == R.RES_UP2 and (H % 2 or W % 2):
                continue
            x, w, b, res = R.conv_res_gauss_case(N, Ci, H, W, Co, k, mode, 40 + i)
            y = F.conv2d(x.double(), w.double(), b.double(), 1, k // 2)
            up = F.interpolate(res.double(), size=(H, W), mode="nearest") if mode == R.RES_UP2 else res.double()
            for act in (R.ACT_NONE, R.ACT_RELU):
                want = F.relu(y + up) if act else y + up
                got = R.conv_res_ref(x, w, b, res, mode, act)
                assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12
            if k == 1 and mode == R.RES_UP2:
                assert torch.equal(R.up2_add(x, w, b, res, R.ACT_RELU), R.conv_res_ref(x, w, b, res, mode, R.ACT_RELU))
    # the upsample is an index map, not an interpolation: an odd half-width (11) and a ramp that names every source pixel
    res = torch.arange(2 * 3 * 6 * 11, dtype=torch.float32).reshape(2, 3, 6, 11)
    up = R.up2(res, 12, 22)
    assert torch.equal(up, F.interpolate(res, scale_factor=2, mode="nearest"))
    assert up[1, 2, 7, 21] == res[1, 2, 3, 10] and up[0, 1, 11, 0] == res[0, 1, 5, 0]


def test_db_tail_reference_matches_conv_transpose2d_in_float64():
    for i, (N, OH, OW) in enumerate(R.DB_TAIL_CASES[:3]):
        x, br = R.db_tail_gauss_case(N, OH, OW, 50 + i)
        for g, (w1, b1, w2, b2) in enumerate(br):
            xg = x[:, 64 * g:64 * g + 64].double()
            v = F.relu(F.conv_transpose2d(xg, w1.double(), b1.double(), 2))
            want = F.conv_transpose2d(v, w2.double(), b2.double(), 2)
            got = R.db_tail_ref(xg, w1, b1, w2, b2)
            assert got.shape == (N, 1, 4 * OH, 4 * OW) and float((R.db_tail_stage1(xg, w1, b1) - v).abs().max()) < 1e-12
            assert float((got - want).abs().max()) < 1e-12
    # one pixel, one channel pair, by hand: out[4 oh + 2 a + a', 4 ow + 2 b + b'] = b2 + relu(x W1[ci, co, a, b] + b1[co]) W2[co, a', b']
    x = torch.zeros(1, 64, 2, 3)
    x[0, 5, 1, 2] = 2.0
    w1, b1, w2, b2 = torch.zeros(64, 64, 2, 2), torch.zeros(64), torch.zeros(64, 1, 2, 2), torch.tensor([0.5])
    w1[5, 9, 1, 0] = 3.0      # (a, b) = (1, 0)
    w2[9, 0, 0, 1] = -1.5     # (a', b') = (0, 1)
    b1[9] = 1.0
    got = R.db_tail_ref(x, w1, b1, w2, b2)
    want = torch.full((1, 1, 8, 12), 0.5, dtype=torch.float64)
    want[0, 0, 0::2, 1::2] = 0.5 + 1.0 * -1.5                 # relu(b1[9]) W2[9, 0, 1] everywhere at (a', b') = (0, 1) ...
    want[0, 0, 4 * 1 + 2 * 1 + 0, 4 * 2 + 2 * 0 + 1] = 0.5 + (2.0 * 3.0 + 1.0) * -1.5      # ... and the one pixel that sees x
    assert torch.equal(got, want)


def test_db_tail_reference_and_branch_order_match_the_oracle_head():
    """The oracle's DBHead on a generated state dict against db_tail_ref fed the folded tensors in the hook's order: branch 0 must be the
    binarise branch (bin_logits) and branch 1 the threshold branch; swapped, the maps differ by far more than the tolerance."""
    sd = weights.make_det_state_dict(seed=7)
    folded = weights.fold_det(sd)
    g = torch.Generator().manual_seed(8)
    fused = torch.randn(1, 256, 5, 6, generator=g)
    with torch.no_grad():
        want = dbnet_cpu.head(sd, fused)
    hc = F.relu(F.conv2d(fused.double(), torch.from_numpy(folded["head.conv.w"]).double(), torch.from_numpy(folded["head.conv.b"]).double(), 1, 1))
    br = R.db_tail_branches_from_folded(folded)
    got = [R.db_tail_ref(hc[:, 64 * i:64 * i + 64], *br[i]) for i in range(2)]
    for i, key in enumerate(("bin_logits", "thresh_logits")):
        scale = float(want[key].abs().max())
        assert float((got[i] - want[key].double()).abs().max()) < 1e-4 * max(1.0, scale), key      # the bar test_oracle_cpu holds the oracle to
    assert float((got[1] - want["bin_logits"].double()).abs().max()) > 1e-2      # the two branches are told apart
    assert float((torch.sigmoid(got[0]) - want["binary"].double()).abs().max()) < 1e-5


def test_integer_routing_inputs_are_exact_in_every_element_type():
    """What the bit-exact GPU tests rely on: operands that bf16 and fp16 hold exactly, integer results, and no partial sum of either dot --
    in any order -- at or above 2^24 (so fp32 accumulation is exact)."""
    for i, (N, OH, OW) in enumerate(R.DB_TAIL_CASES):
        x, br = R.db_tail_int_case(N, OH, OW, 60 + i)
        for t in (x,) + br[0] + br[1]:
            assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t) and torch.equal(t, t.round())
        assert float(x.min()) == 0 and float(x.max()) == 3
        for g, b in enumerate(br):
            assert float(b[0].abs().max()) == 2      # the f16x2 packer's power-of-two layer scale is 2^12 for both groups: exact
            xg = x[:, 64 * g:64 * g + 64]
            ref = R.db_tail_ref(xg, *b)
            assert torch.equal(ref, ref.round()) and float(R.db_tail_stage1(xg, b[0], b[1]).max()) <= 392
            assert R.db_tail_partial_sum_bound(xg, *b) <= 5 + 64 * 392 * 3 < 2 ** 24
            # (f16x2 accumulates the first dot times the layer scale 2^12: multiples of 2^12 below 2^24, exact as well)
            assert (64 * 6 + 8) * 2 ** 12 < 2 ** 24
        assert not torch.equal(R.db_tail_ref(x[:, :64], *br[0]), R.db_tail_ref(x[:, :64], *br[1]))
    x, w, b, res = R.up2_int_case(3, 64, 10, 14, 256, 5)
    out = R.up2_add(x, w, b, res)
    assert float(x.abs().max()) == 0 and float(out.abs().max()) <= 120 and torch.equal(out, out.round())
    for t in (b, res, out.float()):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)
    assert torch.equal(out, (b.view(1, -1, 1, 1) + R.up2(res, 10, 14)).double())
