"""GPU: the convolution epilogues the detector's neck and head depend on, one kernel at a time through ocrvi_test_conv_res and
ocrvi_test_db_tail (include/ocrvi.h), against the float64 statements of tests/epilogue_refs.py (pinned by tests/test_epilogue_refs_cpu.py).

* RES_UP2 (neck.lat0..2: lateral + nearest-2x of the level above): gemm_ring.h's load_group and conv_gemm.h's generic store path;
* ST_DB_TAIL / ST_DB_BIN (the head's two deconvolutions in one GEMM, conv_gemm.h): both logit maps, and the binary-only view of the same
  packed weights with the sigmoid in the epilogue;
* RES_SAME on a plain 3x3 (conv2 of a ResNet-18 BasicBlock with dcn=False): conv_gemm.h's LDS-staged epilogue.

Two kinds of test, in all four compute modes.  ROUTING tests use small-integer data that every element type holds exactly and whose sums
fp32 accumulates exactly in any order, so the output must EQUAL the reference: a wrong image, row, half-pixel, sub-pixel or branch shows as
a mismatch, never as an error inside a budget.  VALUE tests use Gaussian data and the budgets of tests/test_gpu_kernels.py (the same
act(a W^T + b + res) GEMMs at K values that table already passes; the tail's second dot is fp32 FMAs on fp32 registers and adds no operand
rounding), scaled by sqrt(K / 1152) above K = 1152 in the exact modes as test_deform_conv_kernel_detector_shapes does; each runs twice and
must repeat bit for bit.

The shapes are the smallest that cross each boundary; the comment on a case names the kernel and tile launch_conv / launch_gemm_ring pick
for it (csrc/conv_launch.h, csrc/host_util.hip: gemm_ring_eligible).  The dispatch switches are read once per process, so shapes, not
switches, select conv_gemm here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import epilogue_refs as R
from test_gpu_kernels import DT, EXACT, TOL, _rel_err

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x2", "bf16", "f16"]


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _h(t):
    return np.ascontiguousarray(t.numpy(), dtype=np.float32)


def run_conv_res(x, w, b, res, ksize, res_mode, act, dt):
    """out = act(conv(x) + b + res) through ocrvi_test_conv_res; float32 CPU tensors in and out."""
    L = _L()
    N, Cin, H, W = x.shape
    Co = w.shape[0]
    xd = x.cuda().contiguous()
    rd = res.cuda().contiguous() if res is not None else None
    out = torch.full((N, Co, H, W), float("nan"), device="cuda")
    wh, bh = _h(w), (_h(b) if b is not None else None)
    L.check(L.load().ocrvi_test_conv_res(0, DT[dt], xd.data_ptr(), wh.ctypes.data, bh.ctypes.data if bh is not None else None,
                                         rd.data_ptr() if rd is not None else None, N, Cin, H, W, Co, ksize, res_mode, act, out.data_ptr(), 0,
                                         None))
    return out.cpu()


def run_db_tail(x, br, dt, binary_only=False, groups=None, with_out2=True):
    """The head's deconvolutions through ocrvi_test_db_tail.  br: [(W1, b1, W2, b2)] of the binarise and the threshold branch, in that order
    (epilogue_refs.db_tail_branches_from_folded).  Returns (bin_logits, thresh_logits), or the binary map for binary_only."""
    L = _L()
    N, Cx, OH, OW = x.shape
    groups = (1 if binary_only else 2) if groups is None else groups
    assert Cx == 64 * groups
    xd = x.cuda().contiguous()
    (w1a, b1a, w2a, b2a), (w1b, b1b, w2b, b2b) = [[_h(t) for t in b] for b in br]
    out = torch.full((2, N, 1, 4 * OH, 4 * OW), float("nan"), device="cuda")
    L.check(L.load().ocrvi_test_db_tail(0, DT[dt], xd.data_ptr(), w1a.ctypes.data, b1a.ctypes.data, w1b.ctypes.data, b1b.ctypes.data,
                                        w2a.ctypes.data, b2a.ctypes.data, w2b.ctypes.data, b2b.ctypes.data, N, OH, OW, groups, int(binary_only),
                                        out[0].data_ptr(), out[1].data_ptr() if with_out2 and not binary_only else None, 0, None))
    out = out.cpu()
    if binary_only:
        assert torch.isnan(out[1]).all()      # one map is written, nothing else
        return out[0]
    return out[0], out[1]


def run_db_binary_map(bin_logits, thresh_logits):
    """sigmoid(bin_logits) through the db_maps kernel (ocrvi_test_db_maps), the five-map path's way to the binary map."""
    L = _L()
    bd, td = bin_logits.cuda().contiguous(), thresh_logits.cuda().contiguous()
    out = torch.empty_like(bd)
    L.check(L.load().ocrvi_test_db_maps(0, bd.data_ptr(), td.data_ptr(), 50.0, out.data_ptr(), None, None, bd.numel()))
    return out.cpu()


# ---------------------------------------------------------------------------------------------------------------- RES_UP2 (1x1 laterals)
UP2_CASES = [
    # (N, Cin, OH, OW, Co).  Co = 256 is two 128-column ring tiles; K-steps are 32 channels in f32 / f16x2 and 64 in bf16 / f16.
    # gemm_ring<128 rows>, every mode: M = 96 is one partial row tile
    (2, 256, 6, 8, 256),
    # gemm_ring<128 rows>: M = 420, four row tiles that straddle rows and images, a 36-row tail; ONE K-step in the 16-bit modes (two in 4-byte)
    (3, 64, 10, 14, 256),
    # gemm_ring<128 rows>: M = 264; deep K (32 / 16 K-steps); odd half-width 11
    (1, 1024, 12, 22, 256),
    # M = 24800: cdiv(M, 256) x 2 column tiles = 194 >= 192, so f16x2 (8 K-steps) and bf16 / f16 (4 K-steps) take gemm_ring<256 rows, 4 slice
    # groups> with a 224-row tail; f32 stays on 128-row tiles (194 of them, a 96-row tail)
    (2, 256, 100, 124, 256),
    # the same M at K = 128: bf16 / f16 (2 K-steps) take the `mid256` build gemm_ring<256 rows, 2 slice groups>; f16x2 (4 K-steps) the
    # 4-group 256-row build; f32 128-row tiles
    (2, 128, 100, 124, 256),
    # Cin % 32 != 0: not ring-eligible in any mode -> conv_gemm<AM_CONV1, 128 x 128>, generic store path (RES_UP2 clears epi_lds); K padded
    # from 80 to 96 / 128 with zero-filled chunks
    (3, 80, 10, 14, 256),
    # N_g = 32 < 64: conv_gemm<AM_CONV1, 128 x 32>, generic store path; M = 120
    (2, 64, 6, 10, 32),
]


@functools.lru_cache(maxsize=None)
def _up2_value_case(case):
    N, Cin, OH, OW, Co = case
    x, w, b, res = R.conv_res_gauss_case(N, Cin, OH, OW, Co, 1, R.RES_UP2, 100 + sum(case))
    return x, w, b, res, R.up2_add(x, w, b, res, R.ACT_NONE)      # pre-activation, float64; never modified


@pytest.mark.parametrize("dt", MODES)
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU])
@pytest.mark.parametrize("case", UP2_CASES)
def test_res_up2_routing_is_exact(case, act, dt):
    """x = 0: the output is act(bias + res[:, :, oh // 2, ow // 2]), integers of magnitude <= 120 that every element type holds.  A wrong
    image, half-row or half-column changes ~99 % of a pixel's channels."""
    N, Cin, OH, OW, Co = case
    x, w, b, res = R.up2_int_case(N, Cin, OH, OW, Co, 200 + sum(case))
    want = b.view(1, -1, 1, 1) + R.up2(res, OH, OW)
    want = torch.relu(want) if act == R.ACT_RELU else want
    out = run_conv_res(x, w, b, res, 1, R.RES_UP2, act, dt)
    assert torch.equal(out, want), f"{int((out != want).sum())} of {out.numel()} elements differ"


@pytest.mark.parametrize("dt", MODES)
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU])
@pytest.mark.parametrize("case", UP2_CASES)
def test_res_up2_values(case, act, dt):
    x, w, b, res, pre = _up2_value_case(case)
    ref = (torch.relu(pre) if act == R.ACT_RELU else pre).float()
    out = run_conv_res(x, w, b, res, 1, R.RES_UP2, act, dt)
    err = _rel_err(out, ref)
    print(f"\n[res_up2 {case} act={act} {dt}] rel err {err:.3e} (TOL {TOL[dt]:.0e})")
    assert err < TOL[dt], err
    assert torch.equal(out, run_conv_res(x, w, b, res, 1, R.RES_UP2, act, dt))


# ---------------------------------------------------------------------------------------------------- RES_SAME on a plain 3x3 (BasicBlock conv2)
RES3_CASES = [
    # (N, C, H, W), C -> C, ReLU.  A residual keeps the layer off conv3_halo (packed without quartets) and off the ring's 3x3 mode:
    # conv_gemm<AM_CONV3>, LDS-staged epilogue (epi_lds) with the residual read in registers
    (2, 64, 13, 17),      # 128 x 64 tile; ragged M = 442; K = 576
    (1, 128, 16, 16),     # 128 x 128 tile; M = 256, two full tiles; K = 1152
    (2, 256, 6, 10),      # 128 x 128 tile, two column tiles; M = 120; K = 2304
]


@pytest.mark.parametrize("dt", MODES)
@pytest.mark.parametrize("case", RES3_CASES)
def test_res_same_conv3x3_values(case, dt):
    N, Cc, H, W = case
    x, w, b, res = R.conv_res_gauss_case(N, Cc, H, W, Cc, 3, R.RES_SAME, 300 + sum(case))
    ref = R.conv_res_ref(x, w, b, res, R.RES_SAME, R.ACT_RELU).float()
    out = run_conv_res(x, w, b, res, 3, R.RES_SAME, R.ACT_RELU, dt)
    tol = TOL[dt] * (max(1.0, (9 * Cc / 1152.0) ** 0.5) if dt in EXACT else 1.0)
    err = _rel_err(out, ref)
    print(f"\n[res_same 3x3 {case} {dt}] rel err {err:.3e} (tol {tol:.2e})")
    assert err < tol, err
    assert torch.equal(out, run_conv_res(x, w, b, res, 3, R.RES_SAME, R.ACT_RELU, dt))
    # and the residual is what makes the difference: the same call without it is far from the reference
    plain = run_conv_res(x, w, b, None, 3, R.RES_NONE, R.ACT_RELU, dt)
    assert _rel_err(plain, ref) > 0.5


# ------------------------------------------------------------------------------------------------------------ ST_DB_TAIL / ST_DB_BIN
# every case: conv_gemm<AM_CONV1, 128 x 128, 2 x 2 waves> (N_g = 256: four 64-column sub-pixels, one per wave column and column tile), one
# K-step in the 16-bit modes and two in the 4-byte ones; grid (row tiles x 2 column tiles, groups)
@pytest.mark.parametrize("dt", MODES)
@pytest.mark.parametrize("case", R.DB_TAIL_CASES)
def test_db_tail_routing_is_exact(case, dt):
    """Integer operands (epilogue_refs.db_tail_int_case): both logit maps must equal the reference, and the binary-only view's map must
    be the db_maps kernel's sigmoid of those logits, bit for bit."""
    N, OH, OW = case
    x, br = R.db_tail_int_case(N, OH, OW, 400 + sum(case))
    want = [R.db_tail_ref(x[:, 64 * g:64 * g + 64], *br[g]) for g in range(2)]
    bl, tl = run_db_tail(x, br, dt)
    for name, got, ref in (("bin_logits", bl, want[0]), ("thresh_logits", tl, want[1])):
        assert torch.equal(got.double(), ref), f"{name}: {int((got.double() != ref).sum())} of {ref.numel()} pixels differ"
    assert not torch.equal(bl, tl)
    binary = run_db_tail(x[:, :64].contiguous(), br, dt, binary_only=True)
    assert torch.equal(binary, run_db_binary_map(bl, tl))
    assert float((binary.double() - torch.sigmoid(want[0])).abs().max()) <= 2e-6


@pytest.mark.parametrize("dt", MODES)
@pytest.mark.parametrize("case", R.DB_TAIL_CASES)
def test_db_tail_values(case, dt):
    N, OH, OW = case
    x, br = R.db_tail_gauss_case(N, OH, OW, 500 + sum(case))
    bl, tl = run_db_tail(x, br, dt)
    for g, (name, got) in enumerate((("bin_logits", bl), ("thresh_logits", tl))):
        ref = R.db_tail_ref(x[:, 64 * g:64 * g + 64], *br[g]).float()
        err = _rel_err(got, ref)
        print(f"\n[db_tail {case} {name} {dt}] rel err {err:.3e} (TOL {TOL[dt]:.0e})")
        assert err < TOL[dt], (name, err)
    bl2, tl2 = run_db_tail(x, br, dt)
    assert torch.equal(bl, bl2) and torch.equal(tl, tl2)
    # ST_DB_BIN on the one-group view of the same pack: common.h promises the bits of db_maps' sigmoid of the tail's own logits
    binary = run_db_tail(x[:, :64].contiguous(), br, dt, binary_only=True)
    assert torch.equal(binary, run_db_binary_map(bl, tl))
    assert torch.equal(binary, run_db_tail(x[:, :64].contiguous(), br, dt, binary_only=True))
    eb = float((binary.double() - torch.sigmoid(bl.double())).abs().max())
    assert eb <= 2e-6 and float(binary.min()) >= 0.0 and float(binary.max()) <= 1.0, eb


# ------------------------------------------------------------------------------------------------------------------- argument checks
def test_res_up2_rejects_odd_output_sizes():
    for (OH, OW) in ((5, 8), (6, 9)):
        x, w, b = torch.zeros(1, 64, OH, OW), torch.zeros(256, 64, 1, 1), torch.zeros(256)
        res = torch.zeros(1, 256, OH // 2, OW // 2)
        for dt in MODES:
            with pytest.raises(ValueError, match="even"):
                run_conv_res(x, w, b, res, 1, R.RES_UP2, R.ACT_NONE, dt)


def test_conv_res_hook_rejects_inconsistent_residual_arguments():
    x, w, b = torch.zeros(1, 64, 4, 4), torch.zeros(64, 64, 1, 1), torch.zeros(64)
    with pytest.raises(ValueError):
        run_conv_res(x, w, b, None, 1, R.RES_UP2, R.ACT_NONE, "f32")          # a mode without a residual
    with pytest.raises(ValueError):
        run_conv_res(x, w, b, torch.zeros(1, 64, 4, 4), 1, R.RES_NONE, R.ACT_NONE, "f32")
    with pytest.raises(ValueError):
        run_conv_res(x, torch.zeros(64, 64, 5, 5), b, None, 5, R.RES_NONE, R.ACT_NONE, "f32")


def test_db_tail_rejects_a_missing_second_map_and_a_two_group_binary_launch():
    x, br = R.db_tail_int_case(1, 2, 3, 1)
    for dt in MODES:
        with pytest.raises(ValueError, match="db-tail"):
            run_db_tail(x, br, dt, with_out2=False)                            # ST_DB_TAIL without out2
        with pytest.raises(ValueError, match="db-bin"):
            run_db_tail(x, br, dt, binary_only=True, groups=2)                 # ST_DB_BIN on the whole two-group pack
        with pytest.raises(ValueError, match="db-tail"):
            run_db_tail(x[:, :64].contiguous(), br, dt, groups=1)              # ST_DB_TAIL on the one-group view
    with pytest.raises(ValueError):
        run_db_tail(torch.zeros(1, 192, 2, 3), br, "f32", groups=3)
