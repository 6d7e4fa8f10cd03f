"""GPU: the memory-bound kernels of csrc/kernels.hip -- LayerNorm, adaptive scale fusion, FRM vertical attention, max-pool, the DB maps and
the CTC log-softmax / argmax -- each called on its own through its C ABI test hook (include/ocrvi.h) and compared element by element with
the float64 references of tests/aux_refs.py (pinned on the CPU by tests/test_aux_refs_cpu.py).

Every input is first rounded to something the kernel's element type holds exactly (aux_refs.round_to), so that only the kernel's own fp32
arithmetic and its one output rounding are left; every case runs twice and must be bit-identical.  Bounds:

* output rounding: half an ulp of the element type at the value (`_half_ulp`).  That is between 2^-9 |y| and 2^-8 |y| for bf16 and between
  2^-12 |y| and 2^-11 |y| for fp16 (the smaller figure holds at the top of a binade only, the larger at its bottom); for f16x2,
  max(2^-25, 2^-23 |y|) (the lo half carries 11 bits of a remainder <= 2^-12 |y|, and is a multiple of 2^-24 below 2^-14); 0 for fp32;
* LayerNorm's fp32 arithmetic: the formula in `_ln_bound`, derived from the number of roundings in the kernel;
* CTC log-probs: atol 1e-5 (one rounding of |v - mx| <= 64, a sum of <= 1024 expf terms, a logf); argmax and max-pool are exact;
* DB maps: atol 2e-6, the bound tests/test_gpu_fullsize.py asserts for the same expressions, stage by stage;
* ASF and FRM (__expf and a reciprocal: not derivable from the source): the suite's per-type budgets relative to the output rms, TOL of
  tests/test_gpu_kernels.py, unscaled for ASF and times 3 for FRM (an average over keys, as the attention test does); the two largest ASF
  maps exceed it in the 4-byte types and carry 1.5 x their measured error instead (ASF_MEASURED_4BYTE, with the cause).
No test skips or excludes elements."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_refs as R
from test_gpu_kernels import DT, TOL, _rel_err

pytestmark = pytest.mark.gpu

DTS = ["f32", "f16x2", "bf16", "f16"]
INF, NAN = float("inf"), float("nan")


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _h(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


_half_ulp = R.half_ulp


# ------------------------------------------------------------------------------------------------ LayerNorm
def run_layernorm(x, gamma, beta, dt, x_f32=1, out_f32=1):
    L = _L()
    rows, D = x.shape
    xd = x.cuda().contiguous()
    out = torch.full((rows, D), NAN, device="cuda")
    gh, bh = _h(gamma), _h(beta)
    L.check(L.load().ocrvi_test_layernorm(0, DT[dt], xd.data_ptr(), x_f32, out_f32, gh.ctypes.data, bh.ctypes.data, rows, D, out.data_ptr()))
    return out.cpu()


def _ln_A(D):
    """fp32 roundings between an element and its row's mean: A = 4 NV + log2(LPR) -- the in-lane additions (4 per float4, NV float4 per
    lane), the shuffle steps over LPR lanes and the division."""
    return 9 if D <= 128 else (10 if D <= 256 else (14 if D <= 512 else 22))


def _ln_bound(x, gamma, beta, y, sigma, D):
    """|err| <= A 2^-24 (max|x| / sigma) |gamma| + (A + 4) 2^-24 |y - beta|: the error of the mean (a common shift of the row, scaled by
    rstd and gamma) plus the variance sum, the rsqrt and the affine step.  A constant row has sigma = 0: sqrt(1e-5) there, which is what
    the kernel divides by."""
    A = _ln_A(D)
    s = torch.where(sigma > 0, sigma, torch.full_like(sigma, 1e-5 ** 0.5)).unsqueeze(-1)
    mx = x.double().abs().max(-1, keepdim=True).values
    return A * 2.0 ** -24 * (mx / s) * gamma.double().abs() + (A + 4) * 2.0 ** -24 * (y - beta.double()).abs()


def _ln_check(x, gamma, beta, dt, x_f32, out_f32, tag):
    xin = x.float() if x_f32 else R.round_to(x, dt)
    y, sigma = R.layernorm_ref(xin, gamma, beta)
    got = run_layernorm(xin, gamma, beta, dt, x_f32, out_f32)
    assert torch.equal(got, run_layernorm(xin, gamma, beta, dt, x_f32, out_f32)), tag
    arith = _ln_bound(xin, gamma, beta, y, sigma, x.shape[1])
    bound = arith + (_half_ulp(y.abs() + arith, dt) if not out_f32 else 0.0)
    err = (got.double() - y).abs()
    assert torch.isfinite(got).all(), tag
    ratio = float((err / bound.clamp(min=1e-300)).max())
    worst = float(err.max())
    print(f"\n[layernorm {tag}] max |err| {worst:.3e}, max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (tag, worst, ratio)
    return worst, ratio


def _ln_params(D, g):
    return torch.rand(D, generator=g) * 0.4 + 0.8, torch.randn(D, generator=g) * 0.1


LN_DIMS = [4, 64, 96, 128, 132, 192, 256, 260, 384, 512, 516, 768, 1024]
LN_ALL_COMBOS = (128, 260, 1024)      # every (x_f32, out_f32) combination at one D per lane layout that differs; (1, 1) elsewhere


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", LN_DIMS)
def test_layernorm_kernel(D, dt):
    g = torch.Generator().manual_seed(1000 + D)
    gamma, beta = _ln_params(D, g)
    combos = [(1, 1), (1, 0), (0, 1), (0, 0)] if D in LN_ALL_COMBOS else [(1, 1)]
    for rows in (1, 2, 3, 9, 1000):
        x = torch.randn(rows, D, generator=g) * 1.5 + 0.3
        for xf, of in combos:
            _ln_check(x, gamma, beta, dt, xf, of, f"D={D} rows={rows} {dt} x_f32={xf} out_f32={of}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,D", [(16384 + 5, 128), (8192 + 3, 256), (8192 + 3, 384), (8192 + 3, 1024)])
def test_layernorm_kernel_second_grid_sweep(rows, D, dt):
    """One row count past a full grid sweep per build (2048 workgroups x 4 waves x 1 or 2 rows): the prefetched row, the second trip of
    the grid-stride loop and, with two rows per wave and an odd count, the wave whose second half has no row."""
    g = torch.Generator().manual_seed(rows + D)
    gamma, beta = _ln_params(D, g)
    x = torch.randn(rows, D, generator=g) * 1.5 + 0.3
    _ln_check(x, gamma, beta, dt, 1, 1, f"D={D} rows={rows} {dt}")
    _ln_check(x, gamma, beta, dt, 0, 0, f"D={D} rows={rows} {dt} x_f32=0 out_f32=0")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", [4, 128, 132, 384, 516, 1024])
def test_layernorm_kernel_large_mean_constant_rows_and_signed_gamma(D, dt):
    """Rows with |mean| >> std (mean 1000, std 1: what separates a two-pass variance from E[x^2] - mean^2, which loses ulp(1e6) ~ 0.06
    against a variance of 1), read as fp32 as the residual stream is; a constant row, whose output is beta; a negative and a zero gamma."""
    g = torch.Generator().manual_seed(77 + D)
    gamma, beta = _ln_params(D, g)
    x = torch.randn(37, D, generator=g) + 1000.0
    for of in (1, 0):
        _ln_check(x, gamma, beta, dt, 1, of, f"mean-1000 D={D} {dt} out_f32={of}")
    x = torch.randn(9, D, generator=g) * 1.5 + 0.3
    x[2], x[5], x[8] = 0.7, -3.25, 0.0
    for xf, of in ((1, 1), (0, 0)):
        _ln_check(x, gamma, beta, dt, xf, of, f"constant rows D={D} {dt} x_f32={xf} out_f32={of}")
        xin = x.float() if xf else R.round_to(x, dt)
        assert torch.equal(R.layernorm_ref(xin, gamma, beta)[0][[2, 5, 8]], beta.double().expand(3, D))     # the expected output is beta
    gs = gamma.clone()
    gs[0::3], gs[1] = -gs[0::3], 0.0
    for xf, of in ((1, 1), (0, 0)):
        _ln_check(x, gs, beta, dt, xf, of, f"signed gamma D={D} {dt} x_f32={xf} out_f32={of}")


def test_layernorm_rejects_bad_shapes():
    L = _L()
    for rows, D in ((2, 6), (4, 1028), (1, 2048)):
        x = torch.zeros(rows, D, device="cuda")
        out = torch.zeros(rows, D, device="cuda")
        gh = np.ones(D, np.float32)
        for dt in DTS:
            rc = L.load().ocrvi_test_layernorm(0, DT[dt], x.data_ptr(), 1, 1, gh.ctypes.data, gh.ctypes.data, rows, D, out.data_ptr())
            assert rc == -1, (rows, D, dt, rc)                    # OCRVI_EINVAL


# ------------------------------------------------------------------------------------------------ adaptive scale fusion
def run_asf(ps, w, b, dt):
    L = _L()
    N, _, H, W = ps[0].shape
    dev = [p.cuda().contiguous() for p in ps]
    out = torch.full((N, 256, H, W), NAN, device="cuda")
    wh, bh = _h(w), _h(b)
    L.check(L.load().ocrvi_test_asf(0, DT[dt], *[d.data_ptr() for d in dev], wh.ctypes.data, bh.ctypes.data, N, H, W, out.data_ptr()))
    return out.cpu()


ASF_SIZES = [(1, 8, 8), (2, 16, 24), (1, 56, 40), (2, 104, 72), (1, 184, 240), (1, 48, 8), (1, 96, 328)]
# Measured on the MI355X against the float64 reference, max |err| / rms over both weight sets, f32 and f16x2 alike (the two agree to three
# digits: the error is in the tap weights, not in the arithmetic on the maps):
#   (1, 8, 8) 8.1e-7   (2, 16, 24) 2.7e-6   (1, 56, 40) 4.3e-6   (2, 104, 72) 1.23e-5   (1, 48, 8) 1.9e-6
#   (1, 184, 240) 2.496e-5   (1, 96, 328) 5.715e-5
# The error grows with the map because it grows with the tap COORDINATE.  The column kernel forms fx = scale * x and lx = fx - (float)x0,
# and the compiler contracts the pair into fma(scale, x, -x0): lx comes from the unrounded product, while ATen's fp32 interpolate (and the
# reference here) rounds scale * x first.  The two differ by up to half an ulp of the coordinate, 2^-25 * in ~ 5e-6 at in = 164, times a
# tap difference of several rms.  Checked on the MI355X: against the same float64 reference with the x fraction taken from the unrounded
# product (y as ATen) the f32 kernel is within 1.5e-6 / 1.9e-6 / 2.0e-6 at (1, 184, 240) / (1, 96, 328) / (2, 104, 72).  That is the
# fp32 coordinate's own precision -- the kernel is as close to the real-number interpolation as ATen is -- so the kernel stays as it
# is, and the two sizes that pass the 2e-5 budget of the 4-byte types get 1.5 x their measured error (the suite's convention); every other
# size and the 16-bit types (measured <= 2.4e-2 bf16, <= 3.0e-3 f16) keep TOL.
ASF_MEASURED_4BYTE = {(1, 184, 240): 2.496e-5, (1, 96, 328): 5.715e-5}


def _asf_budget(size, dt):
    return max(TOL[dt], 1.5 * ASF_MEASURED_4BYTE.get(size, 0.0)) if dt in ("f32", "f16x2") else TOL[dt]


def _asf_inputs(size, weights, signed, dt, seed):
    N, H, W = size
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(N, 256, H >> l, W >> l, generator=g) for l in range(4)]
    if not signed:
        ps = [F.relu(p) for p in ps]                               # post-ReLU maps, as the FPN's are
    w = torch.randn(4, 1024, generator=g) * (4.0 / 1024) ** 0.5   # weights.make_det_state_dict: neck.asf.conv_atten, gain 4
    b = torch.randn(4, generator=g) * 0.1
    if weights == "steered":
        # every level is the dominant one on a quarter of the map, in 2 x 2-pixel blocks that cross every segment and tile boundary: channel
        # i of p2 is the indicator of block class i and only score i sees it, with weight 20
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        cls = (yy // 2 + xx // 2) % 4
        for i in range(4):
            ps[0][:, i] = (cls == i).float()
            w[:, i] = 0.0
            w[i, i] = 20.0
    return [R.round_to(p, dt) for p in ps], w, b


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("weights", ["plain", "steered"])
@pytest.mark.parametrize("size", ASF_SIZES)
def test_asf_kernel(size, weights, dt):
    """neck.py:57-79 against its literal float64 form.  f32 / f16x2 run the column kernel (48-row segments, a sliding window of three tap
    rows per level), bf16 / f16 the 8 x 8 tile kernel.  With the steered weights a wrong tap of a coarse level enters at full weight."""
    ps, w, b = _asf_inputs(size, weights, False, dt, sum(size))
    ref, att = R.asf_ref(*ps, w, b)
    if weights == "steered":
        for i in range(4):
            share = float((att[:, i] > 0.5).double().mean())
            assert share >= 0.20, (i, share)                       # each level wins on its quarter of the pixels
    got = run_asf(ps, w, b, dt)
    err = _rel_err(got.double(), ref)
    print(f"\n[asf {size} {weights} {dt}] max |err| / rms {err:.3e}")
    assert torch.isfinite(got).all() and err < _asf_budget(size, dt), err
    assert torch.equal(got, run_asf(ps, w, b, dt))


@pytest.mark.parametrize("dt", DTS)
def test_asf_kernel_signed_inputs(dt):
    ps, w, b = _asf_inputs((2, 104, 72), "plain", True, dt, 5)
    ref, _ = R.asf_ref(*ps, w, b)
    got = run_asf(ps, w, b, dt)
    err = _rel_err(got.double(), ref)
    print(f"\n[asf signed {dt}] max |err| / rms {err:.3e}")
    assert err < TOL[dt], err
    assert torch.equal(got, run_asf(ps, w, b, dt))


def test_asf_rejects_heights_that_are_not_multiples_of_8():
    L = _L()
    ps = [torch.zeros(1, 256, 12 >> l, 16 >> l, device="cuda") for l in range(4)]
    out = torch.zeros(1, 256, 12, 16, device="cuda")
    w, b = np.zeros((4, 1024), np.float32), np.zeros(4, np.float32)
    for dt in DTS:
        rc = L.load().ocrvi_test_asf(0, DT[dt], *[p.data_ptr() for p in ps], w.ctypes.data, b.ctypes.data, 1, 12, 16, out.data_ptr())
        assert rc == -1, (dt, rc)


# ------------------------------------------------------------------------------------------------ FRM vertical attention
def run_frm(kv, vq, B, H, W, D, dt):
    L = _L()
    kd = kv.cuda().contiguous()
    out = torch.full((B * W, D), NAN, device="cuda")
    vh = _h(vq)
    L.check(L.load().ocrvi_test_frm_vertical(0, DT[dt], kd.data_ptr(), vh.ctypes.data, B, H, W, D, out.data_ptr()))
    return out.cpu()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("peak", [1.0, 8.0])
@pytest.mark.parametrize("D", [96, 128, 192, 256, 384])
def test_frm_vertical_kernel(D, peak, dt):
    """svtrv2.py:236-243 for every key count the kernel is written for (H = 1 .. 8), ragged and single columns, one and three images;
    vq * 8 gives a peaked softmax over the H keys."""
    g = torch.Generator().manual_seed(D + int(peak))
    vq = torch.randn(D, generator=g) * peak
    worst = 0.0
    for H in range(1, 9):
        for W in (1, 7, 64, 80):
            for B in (1, 3):
                kv = R.round_to(torch.randn(B * H * W, 2 * D, generator=g), dt)
                ref = R.frm_vertical_ref(kv, vq, B, H, W, D)
                got = run_frm(kv, vq, B, H, W, D, dt)
                err = _rel_err(got.double(), ref)
                worst = max(worst, err)
                assert torch.isfinite(got).all() and err < 3 * TOL[dt], (H, W, B, err)
                assert torch.equal(got, run_frm(kv, vq, B, H, W, D, dt)), (H, W, B)
    print(f"\n[frm D={D} vq x {peak} {dt}] max |err| / rms {worst:.3e}")


def test_frm_vertical_rejects_nine_keys_and_partial_heads():
    L = _L()
    for H, D in ((9, 128), (3, 48), (0, 128)):
        kv = torch.zeros(max(H, 1) * 4, 2 * D, device="cuda")
        out = torch.zeros(4, D, device="cuda")
        vq = np.zeros(D, np.float32)
        for dt in DTS:
            rc = L.load().ocrvi_test_frm_vertical(0, DT[dt], kv.data_ptr(), vq.ctypes.data, 1, H, 4, D, out.data_ptr())
            assert rc == -1, (H, D, dt, rc)


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / 2
def run_maxpool(x, dt):
    L = _L()
    N, Cn, H, W = x.shape
    xd = x.cuda().contiguous()
    out = torch.full((N, Cn, (H - 1) // 2 + 1, (W - 1) // 2 + 1), NAN, device="cuda")
    L.check(L.load().ocrvi_test_maxpool(0, DT[dt], xd.data_ptr(), N, Cn, H, W, out.data_ptr()))
    return out.cpu()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (2, 64, 7, 9), (1, 64, 16, 24), (3, 128, 33, 47), (1, 64, 480, 8)])
def test_maxpool_kernel(shape, dt):
    """MaxPool2d(3, 2, 1) on signed and on all-negative tensors (in the detector the input follows a ReLU, where a zero padding or an
    error on negative values is invisible).  Max-pool rounds nothing -- outputs are inputs -- so the comparison is exact in every type."""
    g = torch.Generator().manual_seed(sum(shape))
    x = R.round_to(torch.randn(*shape, generator=g) * 3.0, dt)
    for t in (x, R.round_to(-x.abs() - 0.125, dt)):
        want = F.max_pool2d(t, 3, 2, 1)
        assert float(t.max()) < 0 or t is x
        assert torch.equal(R.maxpool_ref(t).float(), want)
        got = run_maxpool(t, dt)
        assert torch.equal(got, want), float((got - want).abs().max())
        assert torch.equal(got, run_maxpool(t, dt))


def test_maxpool_rejects_channel_counts_that_are_not_multiples_of_8():
    L = _L()
    x = torch.zeros(1, 12, 6, 6, device="cuda")
    out = torch.zeros(1, 12, 3, 3, device="cuda")
    for dt in DTS:
        assert L.load().ocrvi_test_maxpool(0, DT[dt], x.data_ptr(), 1, 12, 6, 6, out.data_ptr()) == -1, dt


# ------------------------------------------------------------------------------------------------ DB maps
@pytest.mark.parametrize("k", [1.0, 50.0])
@pytest.mark.parametrize("outputs", ["all", "no_thresh", "binary_only"])
@pytest.mark.parametrize("n", [4, 1024, 4 * 100003])
def test_db_maps_kernel(n, outputs, k):
    """head.py:28-40.  binary / thresh against the float64 sigmoid of the logits; thresh_binary against the float64 step function of the
    kernel's OWN fp32 binary and thresh (with k = 50 one ulp in either moves the step by up to k / 4 ulps: that is the inputs' error,
    bounded by the first comparison, not the step's).  An output passed as NULL is not written: its place stays a canary."""
    L = _L()
    g = torch.Generator().manual_seed(n + int(k))
    bl, tl = torch.randn(n, generator=g) * 2.0, torch.randn(n, generator=g) * 2.0      # N(0, 4)
    special = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0])
    idx = torch.randperm(n, generator=g)[:min(n, 40)]
    bl[idx] = special.repeat(8)[:len(idx)]
    tl[idx] = special.repeat(8).roll(1)[:len(idx)]
    if n > 8:
        tl[idx[:5]] = bl[idx[:5]]                                   # binary == thresh: the step function at its centre
    bd, td = bl.cuda(), tl.cuda()
    CANARY = -12345.0
    outs = []
    for _ in range(2):
        buf = torch.full((3, n), CANARY, device="cuda")
        th = buf[1].data_ptr() if outputs == "all" else None
        tb = buf[2].data_ptr() if outputs in ("all", "no_thresh") else None
        L.check(L.load().ocrvi_test_db_maps(0, bd.data_ptr(), td.data_ptr(), k, buf[0].data_ptr(), th, tb, n))
        outs.append(buf.cpu())
    got = outs[0]
    assert torch.equal(outs[0], outs[1])
    rb, rt = R.db_maps_ref(bl, tl)
    eb = float((got[0].double() - rb).abs().max())
    assert torch.isfinite(got[0]).all() and float(got[0].min()) >= 0.0 and float(got[0].max()) <= 1.0 and eb <= 2e-6, eb
    if outputs == "all":
        et = float((got[1].double() - rt).abs().max())
        assert float(got[1].min()) >= 0.0 and float(got[1].max()) <= 1.0 and et <= 2e-6, et
        own_t = got[1]
    else:
        assert bool((got[1] == CANARY).all())
        own_t = torch.sigmoid(tl)      # not used below
    if outputs in ("all", "no_thresh"):
        # the kernel steps its own fp32 binary and thresh; thresh is not stored when NULL, so take it from a second call that stores it
        if outputs == "no_thresh":
            buf = torch.full((3, n), CANARY, device="cuda")
            L.check(L.load().ocrvi_test_db_maps(0, bd.data_ptr(), td.data_ptr(), k, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), n))
            assert torch.equal(buf[0].cpu(), got[0]) and torch.equal(buf[2].cpu(), got[2])
            own_t = buf[1].cpu()
        es = float((got[2].double() - R.db_step_ref(got[0], own_t, k)).abs().max())
        print(f"\n[db maps n={n} k={k} {outputs}] binary {eb:.2e} step {es:.2e}")
        assert torch.isfinite(got[2]).all() and float(got[2].min()) >= 0.0 and float(got[2].max()) <= 1.0 and es <= 2e-6, es
    else:
        assert bool((got[2] == CANARY).all())


# ------------------------------------------------------------------------------------------------ CTC log-softmax + argmax
def run_ctc(x, B, T, Cn, want_lp=True, want_am=True):
    """x: [B*T][ld] float32 (row = b*T + t) -> (log_probs [T][B][C], argmax_ids [B][T])."""
    L = _L()
    ld = x.shape[1]
    xd = x.cuda().contiguous()
    lp = torch.full((T, B, Cn), 12345.0, device="cuda")
    am = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    L.check(L.load().ocrvi_test_ctc_logsoftmax(0, xd.data_ptr(), ld, B, T, Cn, lp.data_ptr() if want_lp else None, am.data_ptr() if want_am else None))
    return lp.cpu(), am.cpu()


def _ctc_logits(B, T, Cn, pad, seed):
    """Logits with a spread of up to +-32, an untied maximum (float64 top-2 margin >= 1e-3) in the plain rows, and -- where there are
    rows enough -- engineered rows: the row maximum copied to 2 - 4 other positions (same lane = same class mod 64, another lane, another
    64-class block), -inf entries beside finite ones, and the three non-finite kinds (a NaN, a +inf, nothing but -inf)."""
    g = torch.Generator().manual_seed(seed)
    rows = B * T
    x = (torch.randn(rows, Cn, generator=g) * 10.0).clamp(-31.0, 31.0)
    if Cn > 1:
        top = x.topk(2, -1)
        close = (top.values[:, 0] - top.values[:, 1]) < 4e-3
        x[close, top.indices[close, 0]] += 0.5                      # (a clamped pair, or a draw too close to call in fp32)
    kinds = {}
    if rows >= 15:
        def tie(r, pos):
            pos = [p for p in pos if p < Cn]
            x[r, pos] = x[r].max()
            kinds[r] = "tie"
        m1, m2, m4 = int(x[1].argmax()), int(x[2].argmax()), int(x[4].argmax())
        tie(1, [m1 % 64 + 64 * j for j in range(1, 5)] + [m1 % 64])            # the same lane, other 64-class blocks
        tie(2, [(m2 + 1) % Cn, (m2 + 17) % Cn, Cn - 1])                        # other lanes
        tie(4, [(m4 + 64) % Cn, (m4 + 200) % Cn, (m4 + 777) % Cn, 0][:3 if Cn < 4 else 4])
        tie(3, list(range(Cn)))                                                # every class tied: index 0
        x[6, 1::3] = -INF
        kinds[6] = "neginf"
        x[8, min(3, Cn - 1)] = NAN
        x[10, Cn // 2] = INF
        x[12] = -INF
        kinds.update({8: "nonfinite", 10: "nonfinite", 12: "nonfinite"})
    full = torch.full((rows, Cn + pad), 1e30)                       # padding columns the kernel must not read
    full[:, :Cn] = x
    return full, kinds


def _ctc_expect(full, kinds, B, T, Cn):
    """Reference side of a case: float64 log-probs [B*T][C], the mask of non-finite rows and the expected argmax, with the margins the
    case was built for asserted on the reference (a too-close draw fails loudly here instead of being ignored)."""
    x = full[:, :Cn]
    ref = R.log_softmax_ref(x)
    bad = torch.tensor([kinds.get(r) == "nonfinite" for r in range(B * T)])
    assert bool(torch.isnan(ref[bad]).all()) and not bool(torch.isnan(ref[~bad]).any())
    # expected argmax: the first index of the row maximum (tied logits are bit-equal, so their log-probs are too); 0 for a NaN row, as
    # torch.log_softmax(..).argmax(-1) and ocrvi_ctc_greedy give
    top = x.max(-1, keepdim=True).values
    want = (x == top).int().argmax(-1)
    want[bad] = 0
    if Cn > 1:
        t2 = ref[~bad].topk(2, -1).values
        margin = t2[:, 0] - t2[:, 1]
        tied = ((x == top).sum(-1) > 1)[~bad]
        assert float(margin[~tied].min()) >= 1e-3                    # untied rows: a margin fp32 resolves
        assert not bool(tied.any()) or float(margin[tied].max()) == 0.0
        if B * T >= 15 and Cn >= 3:
            assert int(tied.sum()) >= 3
    return ref, bad, want


def _ctc_check(B, T, Cn, pad, seed):
    full, kinds = _ctc_logits(B, T, Cn, pad, seed)
    ref, bad, want = _ctc_expect(full, kinds, B, T, Cn)
    lp, am = run_ctc(full, B, T, Cn)
    lp2, am2 = run_ctc(full, B, T, Cn)
    assert torch.equal(am, am2) and torch.equal(torch.nan_to_num(lp, nan=7.0), torch.nan_to_num(lp2, nan=7.0)) and torch.equal(torch.isnan(lp), torch.isnan(lp2))
    got = lp.permute(1, 0, 2).reshape(B * T, Cn).double()            # log_probs is laid out [T][B][C]
    assert bool(torch.isnan(got[bad]).all()), "a non-finite row's log-probs are NaN"
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[~fin & ~bad.unsqueeze(-1)], ref[~fin & ~bad.unsqueeze(-1)])    # -inf entries
    err = float((got[fin] - ref[fin]).abs().max())
    assert err <= 1e-5, err
    ids = am.reshape(-1).long()
    assert bool(((ids >= 0) & (ids < Cn)).all()), ids[(ids < 0) | (ids >= Cn)]
    assert torch.equal(ids, want), (ids != want).nonzero().reshape(-1)[:8]
    return err, lp, am


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (7, 80), (256, 80)])
@pytest.mark.parametrize("Cn", [1, 2, 63, 64, 65, 232, 1000, 1024])
def test_ctc_logsoftmax_argmax_kernel(Cn, B, T, pad):
    err, _, _ = _ctc_check(B, T, Cn, pad, Cn * 7 + B + pad)
    print(f"\n[ctc C={Cn} B={B} T={T} ld=C+{pad}] max |err| {err:.2e}")


@pytest.mark.parametrize("Cn", [5, 232, 1024])
def test_ctc_fused_and_standalone_decodes_agree_on_non_finite_rows(Cn):
    """The two decode entry points on the same rows, NaN / +inf / all -inf rows among them: the fused kernel's argmax_ids equal
    ocrvi_ctc_greedy's on the fused kernel's own log-probs, and the greedy path (ids, lens) is the collapse of either."""
    L = _L()
    B, T = 3, 5
    _, lp, am = _ctc_check(B, T, Cn, 0, 99 + Cn)
    lpd = lp.cuda()
    am2 = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    L.check(L.load().ocrvi_ctc_greedy(0, lpd.data_ptr(), T, B, Cn, 0, am2.data_ptr(), ids.data_ptr(), lens.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(am2.cpu(), am)
    want_ids, want_lens = R.ctc_collapse_ref(am.numpy(), 0)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(lens.cpu().numpy(), want_lens)


def test_ctc_logsoftmax_outputs_are_nullable_and_bad_shapes_rejected():
    L = _L()
    full, _ = _ctc_logits(3, 5, 65, 0, 1)
    lp, am = run_ctc(full, 3, 5, 65)
    lp_only, am_none = run_ctc(full, 3, 5, 65, want_am=False)
    lp_none, am_only = run_ctc(full, 3, 5, 65, want_lp=False)
    assert torch.equal(am_only, am) and bool((am_none == -7).all()) and bool((lp_none == 12345.0).all())
    assert torch.equal(torch.nan_to_num(lp_only, nan=7.0), torch.nan_to_num(lp, nan=7.0))
    x = torch.zeros(4, 1025, device="cuda")
    out = torch.zeros(4 * 1025, device="cuda")
    am = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert L.load().ocrvi_test_ctc_logsoftmax(0, x.data_ptr(), 1025, 2, 2, 1025, out.data_ptr(), am.data_ptr()) == -1      # C > 1024
    assert L.load().ocrvi_test_ctc_logsoftmax(0, x.data_ptr(), 63, 2, 2, 64, out.data_ptr(), am.data_ptr()) == -1          # ld < C
