"""GPU: lin_x2_kernel (csrc/lin_x2.hip), the token-stationary f16x2 Linear of the recogniser's qkv-type layers, through ocrvi_test_lin_x2.
References, bounds and input families are those of the ring GEMM (tests/gemm_refs.py, imported unchanged): the kernel has to compute what
the ring computes, bit for bit.  Every launch writes into a buffer of M + 128 rows prefilled with a NaN payload: rows >= M must come back
untouched and every one of the M x N elements finite.

  routing       routed_int_case without a residual (integers: exact in every format, summed exactly in any order): output == float64
                reference for K in {256, 384} x N in {32, 160, 768, 1152} x M in {1, 16, 17, 127, 128, 129, 300}
  value         value_case rows (randn, cancel, small, outlier) against gemm_bound(.., "f16x2", out_f32=False); the largest ratio is printed
  same bits     ocrvi_test_gemm (f16x2, no activation, no residual: the ring) and the new hook on the same inputs: torch.equal
  later tiles   max_workgroups 1 and 2 at M = 2 * 128 + 37 and 4 * 128: a workgroup walks 3 then 2 (or 3 / 4 then 2) tiles, the weight ring
                runs across the tile boundaries; rows of period 97, every later row bit-equal to its first occurrence; repeated launch
  independence  the first 17 rows at M = 17 and at M = 300 are equal
  guard         rows >= M of the caller's buffer untouched at M = 1, 127, 129
  range flag    an output of magnitude 65536 raises the device's flag as the ring does on the same inputs; 65280 does not
  model path    an 8-crop SVTRv2-base forward in f16x2, against a child process with OCRVI_MLP_X2=0.  That switch takes the fused MLP
                (mlp_x2) out together with this kernel, and the unfused MLP rounds differently, so the two forwards cannot be bit-equal
                whatever this kernel does: log-probs within 1e-4 (the bar tests/test_gpu_parity_modes.py holds f16x2 to) and equal ids.

Measured on the MI355X (256 CUs): 32 tests, 5.9 s for the file; largest err / bound 0.016 (value, K = 256, N = 768), 0.007-0.011 elsewhere;
the model path differs from the OCRVI_MLP_X2=0 child by 1.7e-5 at most, ids equal.  A build with the two k-groups of the weight fragments
exchanged fails the routing and value tests (profiles/r25_lin_x2.md).

routed_weights of gemm_refs puts one weight on every k of a column tile and refuses a tile that would need more than 8 per row; a 32-column
tile at K = 384 needs 12 (still integers of magnitude <= 12 x 7 + 8), so those shapes build their weights with the same rule here.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu

GUARD = 128
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
KS = (256, 384)
NS = (32, 160, 768, 1152)
MS = (1, 16, 17, 127, 128, 129, 300)
WORST = {}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def run_lin(a, w, b, max_wg=0):
    """One launch: out [M, N] float32 on the GPU.  Guard rows and NaNs are checked here."""
    L = _L()
    M, K = a.shape
    N = w.shape[0]
    raw = torch.full(((M + GUARD) * N,), X_GUARD, dtype=torch.int32, device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda")
    ad = a.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_lin_x2(0, ad.data_ptr(), wh.ctypes.data, bh.ctypes.data, M, K, N, max_wg, raw.data_ptr(), out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert bool((raw[M * N:] == X_GUARD).all()), "the guard rows behind the output changed"
    assert bool(torch.isfinite(out).all()), "an element of the output was not written (or is not finite)"
    return out


def run_ring(a, w, b):
    L = _L()
    M, K = a.shape
    N = w.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda")
    ad = a.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_gemm(0, R.DT_CODE["f16x2"], ad.data_ptr(), wh.ctypes.data, bh.ctypes.data, None, M, K, N, R.ACT_NONE, 0, 0,
                                     out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    return out


def _routed_weights_12(N, K, seed):
    """gemm_refs.routed_weights with up to 12 covering entries per row (a 32-column tile at K = 384): same cover rule, same seeded signs."""
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(N)
    tile0 = n // 128 * 128
    nc = torch.clamp(N - tile0, max=128)
    c = n - tile0
    cover = (torch.arange(K)[None, :] % nc[:, None]) == c[:, None]
    ncover = cover.sum(1)
    assert int(ncover.max()) <= 12
    want = 8 + (n * 7 + seed) % 5
    score = torch.rand(N, K, generator=g)
    score[cover] = -1.0
    rank = score.argsort(1, descending=True).argsort(1)
    mask = cover | (rank < (want - ncover)[:, None])
    sign = torch.randint(0, 2, (N, K), generator=g) * 2.0 - 1.0
    return torch.where(mask, sign, torch.zeros(()))


_ROUTED = {}


def routed(M, K, N, seed):
    """routed_int_case(M, K, N, seed, with_res=False); the reference of the largest M is computed once per (K, N) and sliced."""
    key = (K, N, seed)
    if key not in _ROUTED:
        Mx = max(MS)
        if K // min(128, N - N // 128 * 128 or 128) <= 8:
            a, w, b, _ = R.routed_int_case(Mx, K, N, seed, with_res=False)
        else:
            a, _, b, _ = R.routed_int_case(Mx, K, 128, seed, with_res=False)
            w = _routed_weights_12(N, K, seed)
            b = b[:N] if N <= 128 else torch.cat([b] * (N // 128 + 1))[:N]
        assert float((a.abs() @ w.abs().t()).max()) + 8 <= 256 and bool((w.abs().sum(0) > 0).all())
        _ROUTED[key] = (a, w, b, R.gemm_ref(a, w, b, None, R.ACT_NONE, 0))
    a, w, b, ref = _ROUTED[key]
    return a[:M], w, b, ref[:M]


def _equal(out, ref, tag):
    bad = (out.cpu().double() != ref).nonzero()
    assert bad.numel() == 0, (tag, int(bad.shape[0]), [(r, c, float(out[r, c]), float(ref[r, c])) for r, c in bad[:8].tolist()])


def _hold(out, ref, bound, tag):
    q = R.err_ratio(out.cpu(), ref, bound)
    worst = float(q.max())
    print(f"\n[lin_x2 {tag}] max err / bound {worst:.3f}")
    WORST[tag] = worst
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (tag, worst, bad[:8].tolist())


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_routing(K, N):
    for M in MS:
        a, w, b, ref = routed(M, K, N, 11 + N % 7)
        _equal(run_lin(a, w, b), ref, (M, K, N))


@pytest.mark.parametrize("K,N", [(256, 160), (384, 160), (256, 768), (384, 1152)])
def test_values(K, N):
    a, w, b, _ = R.value_case(200, K, N, "f16x2", 0, 5)
    ref = R.gemm_ref(a, w, b, None, R.ACT_NONE, 0)
    bound = R.gemm_bound(a, w, b, None, R.ACT_NONE, 0, "f16x2", False)
    _hold(run_lin(a, w, b), ref, bound, f"value K={K} N={N}")


@pytest.mark.parametrize("M,K,N", [(300, 256, 768), (300, 384, 1152), (257, 384, 768)])
def test_same_bits_as_the_ring(M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    a = R.round_to(torch.randn(M, K, generator=g), "f16x2")
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    new, ring = run_lin(a, w, b), run_ring(a, w, b)
    assert torch.equal(new, ring), (int((new != ring).sum()), float((new - ring).abs().max()))


def test_same_bits_as_the_ring_value_case():
    a, w, b, _ = R.value_case(200, 384, 1152, "f16x2", 0, 6)
    new, ring = run_lin(a, w, b), run_ring(a, w, b)
    assert torch.equal(new, ring), (int((new != ring).sum()), float((new - ring).abs().max()))


@pytest.mark.parametrize("M", [2 * 128 + 37, 4 * 128])
@pytest.mark.parametrize("max_wg", [1, 2])
@pytest.mark.parametrize("K", KS)
def test_later_tiles(K, max_wg, M):
    N = 160                      # 5 units: more than the ring's slots, and no multiple of them -- a tile starts in a different slot each time
    a1, w, b, _ = R.periodic_case(K, N, "f16x2", 0, 21)
    reps = -(-M // R.PERIOD)
    a = torch.cat([a1] * reps)[:M]
    out = run_lin(a, w, b, max_wg)
    ref = R.gemm_ref(a1, w, b, None, R.ACT_NONE, 0)
    _hold(out[:R.PERIOD], ref, R.gemm_bound(a1, w, b, None, R.ACT_NONE, 0, "f16x2", False), f"later K={K} wg={max_wg} M={M}")
    first = torch.cat([out[:R.PERIOD]] * reps)[:M]
    assert torch.equal(out, first), "a later row differs from its first occurrence"
    assert torch.equal(out, run_lin(a, w, b, max_wg)), "two runs differ"
    assert torch.equal(out, run_lin(a, w, b)), "the capped grid and the full grid differ"


@pytest.mark.parametrize("K", KS)
def test_independent_of_M(K):
    a, w, b, _ = R.value_case(300, K, 768, "f16x2", 0, 8)
    assert torch.equal(run_lin(a[:17], w, b), run_lin(a, w, b)[:17])


@pytest.mark.parametrize("M", [1, 127, 129])
def test_rows_past_M_are_not_written(M):
    a, w, b, _ = R.value_case(M, 384, 1152, "f16x2", 0, 9)
    run_lin(a, w, b)             # (the guard is checked in run_lin)
    run_lin(a, w, b, 1)


def _flag():
    L = _L()
    v = C.c_int(0)
    L.check(L.load().ocrvi_range_flag(0, C.byref(v)))
    return v.value


def _reset():
    L = _L()
    L.check(L.load().ocrvi_range_reset(0, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", KS)
def test_range_flag_raised_as_by_the_ring(K):
    """Row 5, column 3: 256 weights of 1 against activations of 256 (or 255) = 65536 (65280); every other output is small."""
    M, N = 40, 128               # (a multiple of 128 columns: ocrvi_test_gemm runs the ring)
    w = torch.zeros(N, K)
    w[3, :256] = 1.0
    w[7, 0] = 0.5
    b = torch.zeros(N)
    try:
        for v, want in ((256.0, 1), (255.0, 0)):
            a = torch.ones(M, K)
            a[5, :256] = v
            seen = []
            for run in (run_ring, run_lin_unchecked):
                _reset()
                assert _flag() == 0
                out = run(a, w, b)
                seen.append(_flag())
                if not want:
                    assert float(out[5, 3]) == 65280.0
            assert seen == [want, want], (v, seen)
    finally:
        _reset()


def run_lin_unchecked(a, w, b):
    """run_lin without the finiteness check (an element past fp16's range decodes to NaN, like the ring's)."""
    L = _L()
    M, K = a.shape
    N = w.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda")
    ad = a.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_lin_x2(0, ad.data_ptr(), wh.ctypes.data, bh.ctypes.data, M, K, N, 0, None, out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    return out


_CHILD = """
import sys, numpy as np, torch
from ocr_vi_invoice_amd import SVTRv2
x = torch.from_numpy(np.load(sys.argv[1])).cuda()
m = SVTRv2("base", dtype="f16x2", seed=1234)
lp = m(x)
np.save(sys.argv[2], lp.cpu().numpy())
"""


def test_model_path_against_the_ring_launches(tmp_path):
    from ocr_vi_invoice_amd import SVTRv2, synth
    x = synth.pad_crop_batch(synth.make_crops(5, 8, height=32, max_width=128), 32, 128)
    np.save(tmp_path / "x.npy", x)
    m = SVTRv2("base", dtype="f16x2", seed=1234)
    lp = m(torch.from_numpy(x).cuda()).cpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OCRVI_MLP_X2="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "x.npy"), str(tmp_path / "lp.npy")], env=env, cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ring = torch.from_numpy(np.load(tmp_path / "lp.npy"))
    diff = float((lp - ring).abs().max())
    print(f"\n[lin_x2 model] 8 crops, SVTRv2-base f16x2: max |dlog-prob| vs OCRVI_MLP_X2=0 {diff:.2e}; bit-equal {torch.equal(lp, ring)}")
    assert diff < 1e-4, diff
    assert torch.equal(lp.argmax(-1), ring.argmax(-1))
