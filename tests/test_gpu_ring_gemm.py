"""GPU: gemm_ring_kernel (csrc/gemm_ring.h) in all four element types through ocrvi_test_gemm_raw and ocrvi_test_conv, every element held to
the float64 reference of tests/gemm_refs.py: equal to it on routed integer data, within gemm_bound (derivation there) on value data.
tests/test_gemm_refs_cpu.py shows on the CPU that an fp32 emulation of the kernel stays inside the bound on exactly these cases and that
fourteen wrong kernels land outside it.  Every GEMM case first asserts the build it reaches (BM, BN, SPS, F32O) through
ocrvi_test_ring_plan with the device's CU count, then runs twice into a NaN-filled output with 128 guard rows of a NaN payload behind it:
the two runs must be bit-identical, all M x N elements finite, the guard rows untouched.  No element is excluded from any comparison.

  routing       routed_int_case (integers, 8 to 12 weights of +-1 per column, every k used in every column tile): output == reference.
                N = 128, 232 (N tail, fp32 output and residual), 64 (the 256x64 build); plain, residual before and after the
                activation; none and ReLU; the strided 1x1 mode and the 3x3 mode through ocrvi_test_conv
  value         value_case (Gaussian, cancelling, 2^-10-scaled and one-outlier rows; the bias sweeps GELU over [-12, 12]): three activations,
                no residual and both orders
  tail          every M of gemm_refs.tail_M at one to four K-steps, N = 128 (T output, residual, ReLU) and 232 (fp32 output); M <= 128
                at one K-step is a launch of a single step
  builds        routed data on the smallest shape of every build the type has: 128x128, 256x128 at 4, 5, 6 K-steps, mid256 at 2 and 3,
                256x64 at 1 and 4; 16-bit and fp32 output where both exist
  later tiles   rows and residual of period 97 on launches whose workgroups walk 1 and 2, or 3 and 4, row tiles in every build: the first 97
                rows are held to the bound, every later row is bit-equal to its first occurrence (compared on the device)
  independence  one row of a changed: every other row keeps its bits; one row of w and its bias changed: every other column does

Largest err / bound per family and type, measured on the MI355X (256 CUs; 106 tests, 7.2 s for the file; the slowest test 0.61 s, the first,
which loads the library):
                f32      f16x2    bf16     f16
  value         0.687    0.514    1.000    1.000
  tail          0.378    0.155    1.000    1.000
  later tiles   0.690    0.748    1.000    1.000
(routing, builds and independence are equalities.  The CPU emulation gives 0.689 / 0.515 / 1.000 / 1.000, 0.206 / 0.155 / 1.000 / 1.000 and
0.690 / 0.748 / 1.000 / 1.000: the 16-bit figures at 1 are elements whose whole error is the last rounding to T next to a tie.  Nothing was
found wrong in the kernel or in the launcher.  profiles/r16_ring_gemm.md has the CPU tables.)
"""
import os
import time

import numpy as np
import pytest
import torch

import gemm_refs as R
from test_gpu_kernels import DT, run_conv

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

GUARD = 128                      # rows behind the output
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
WORST = {}
WALKED = {}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_plan(dt, amode, M, K, N, of, has_res, build, tiles=None):
    plan = R.plan_of(_L().load(), dt, amode, M, K, N, of, has_res, _n_cu())
    assert plan[:5] == (1, *R.expect(build, dt, of)), (dt, M, K, N, of, build, plan)
    if tiles is not None:
        assert plan[6:] == tiles, (dt, M, K, N, build, plan)
    return plan


def run_gemm(a, w, b, res, act, res_post, dt, of):
    """One launch on a [M, K] and res [M, N] (CPU or GPU float32 tensors): out [M, N] float32 on the GPU.  Guards and NaNs are checked here."""
    L = _L()
    M, K = a.shape
    N = w.shape[0]
    esz = 4 if (of or dt in ("f32", "f16x2")) else 2
    raw = torch.full(((M + GUARD) * N * esz,), 0xFF, dtype=torch.uint8, device="cuda")        # every element a NaN
    guard = raw[M * N * esz:].view(torch.int32)
    guard.fill_(X_GUARD)
    out = torch.full((M, N), float("nan"), device="cuda")
    ad = a.cuda().contiguous()
    rd = None if res is None else res.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_gemm_raw(0, DT[dt], ad.data_ptr(), wh.ctypes.data, bh.ctypes.data, None if rd is None else rd.data_ptr(),
                                         M, K, N, act, int(res_post), int(of), raw.data_ptr(), out.data_ptr()))
    torch.cuda.synchronize()
    assert bool((guard == X_GUARD).all()), "the guard rows behind the output changed"
    assert bool(torch.isfinite(out).all()), "an element of the output was not written (or is not finite)"
    return out


def run_twice(a, w, b, res, act, res_post, dt, of):
    out = run_gemm(a, w, b, res, act, res_post, dt, of)
    assert torch.equal(out, run_gemm(a, w, b, res, act, res_post, dt, of)), "two runs differ"
    return out


def _hold(out, ref, bound, family, dt, tag):
    q = R.err_ratio(out.cpu(), ref, bound)
    worst = float(q.max())
    print(f"\n[ring {family} {dt} {tag}] max err / bound {worst:.3f}")
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), worst)
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (family, dt, tag, worst, bad[:8].tolist())


def _equal(out, ref, tag):
    bad = (out.cpu().double() != ref).nonzero()
    assert bad.numel() == 0, (tag, int(bad.shape[0]), [(r, c, float(out[r, c]), float(ref[r, c])) for r, c in bad[:8].tolist()])


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[ring summary] {time.time() - t0:.0f} s; largest err / bound per family and type")
    for fam in ("value", "tail", "later"):
        print(f"[ring summary] {fam:6s} " + "   ".join(f"{dt} {WORST.get((fam, dt), float('nan')):.3f}" for dt in R.DTS))
    print(f"[ring summary] tiles per workgroup walked in the later-tiles family: { {k: sorted(v) for k, v in WALKED.items()} }")


@pytest.mark.parametrize("dt", R.DTS)
def test_ring_routing(dt):
    for i, (M, K, N, of, rp, act) in enumerate(R.routing_cases(dt)):
        _assert_plan(dt, 0, M, K, N, of, rp is not None, "256x64" if N == 64 else "128x128")
        a, w, b, res = R.routed_int_case(M, K, N, 11 + i % 7, rp is not None)
        out = run_twice(a, w, b, res, act, rp or 0, dt, of)
        _equal(out, R.gemm_ref(a, w, b, res, act, rp or 0), (dt, M, K, N, of, rp, act))


CONV_PARAMS = [(dt, c) for dt in R.DTS for c in R.CONV_ROUTED if c[5] == 1 or dt in ("bf16", "f16")]


@pytest.mark.parametrize("dt,case", CONV_PARAMS)
def test_ring_routing_strided_and_3x3(dt, case):
    """The strided 1x1 mode (per-lane offsets from the tensor base) and the 3x3 mode (tap masks, zero page) on routed integers, through
    ocrvi_test_conv (whose output lives in the hook's own allocation: no guard rows here)."""
    n, Cin, H, W, Co, ks, stride, build = case
    M = n * ((H - 1) // stride[0] + 1) * ((W - 1) // stride[1] + 1)
    _assert_plan(dt, 1 if ks == 3 else 0, M, ks * ks * Cin, Co, 0, False, build)
    x, w, b = R.routed_conv_case(n, Cin, H, W, Co, ks, 17)
    for act in (R.ACT_NONE, R.ACT_RELU):
        ref = R.conv_ref(x, w, b, stride, act)
        out = run_conv(x, w, b, ks, stride[0], stride[1], 1, act, dt)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, run_conv(x, w, b, ks, stride[0], stride[1], 1, act, dt))
        bad = (out.double() != ref).nonzero()
        assert bad.numel() == 0, (dt, case, act, int(bad.shape[0]), bad[:8].tolist())


@pytest.mark.parametrize("dt", R.DTS)
def test_ring_value(dt):
    for (M, K, N, of, rp, act) in R.value_cases(dt):
        _assert_plan(dt, 0, M, K, N, of, rp is not None, "128x128")
        a, w, b, res = R.value_case(M, K, N, dt, of, 5)
        res = res if rp is not None else None
        out = run_twice(a, w, b, res, act, rp or 0, dt, of)
        _hold(out, R.gemm_ref(a, w, b, res, act, rp or 0), R.gemm_bound(a, w, b, res, act, rp or 0, dt, of), "value", dt, f"act {act} res {rp} out_f32 {of}")


@pytest.mark.parametrize("nk", (1, 2, 3, 4))
@pytest.mark.parametrize("dt", R.DTS)
def test_ring_tail(dt, nk):
    for (nk_, K, N, of, rp, act) in R.tail_cases(dt):
        if nk_ != nk:
            continue
        a, w, b, res = R.tail_case(dt, nk, N, of)
        res = res if rp is not None else None
        ref, bound = R.gemm_ref(a, w, b, res, act, rp or 0), R.gemm_bound(a, w, b, res, act, rp or 0, dt, of)
        for M in R.tail_M:
            _assert_plan(dt, 0, M, K, N, of, rp is not None, "128x128", (1, 1))
            out = run_twice(a[:M], w, b, None if res is None else res[:M], act, rp or 0, dt, of)
            _hold(out, ref[:M], bound[:M], "tail", dt, f"M {M} nk {nk} N {N}")


BUILD_PARAMS = [(dt, build, of, nk) for dt in R.DTS for build, of in R.build_variants(dt) for nk in R.build_nks(build)]


@pytest.mark.parametrize("dt,build,of,nk", BUILD_PARAMS)
def test_ring_builds(dt, build, of, nk):
    M, K, N = R.build_shape(build, nk, dt)
    _assert_plan(dt, 0, M, K, N, of, True, build)
    a, w, b, res = R.routed_int_case(M, K, N, 23 + nk)
    out = run_twice(a, w, b, res, R.ACT_RELU, 0, dt, of)
    _equal(out, R.gemm_ref(a, w, b, res, R.ACT_RELU, 0), (dt, build, of, nk))


LATER_PARAMS = [(dt, build, of, t) for dt in R.DTS for build, of in R.build_variants(dt) for t in (2, 4)]


@pytest.mark.parametrize("dt,build,of,t", LATER_PARAMS)
def test_ring_later_tiles_equal_the_first(dt, build, of, t):
    M, K, N, gm, lo, hi = R.later_shape(build, dt, _n_cu(), t)
    _assert_plan(dt, 0, M, K, N, of, True, build, (lo, hi))
    assert hi == lo + 1                                       # an odd and an even number of tiles in this launch: drain(accA) and drain(accB)
    WALKED.setdefault((dt, build, of), set()).update((lo, hi))
    a, w, b, res = R.periodic_case(K, N, dt, of, 21)
    idx = torch.arange(M, device="cuda") % R.PERIOD
    out = run_twice(a.cuda()[idx], w, b, res.cuda()[idx], R.ACT_GELU, 1, dt, of)
    _hold(out[:R.PERIOD], R.gemm_ref(a, w, b, res, R.ACT_GELU, 1), R.gemm_bound(a, w, b, res, R.ACT_GELU, 1, dt, of), "later", dt,
          f"{build} out_f32 {of} M {M} tiles {lo}/{hi}")
    bad = (out != out[:R.PERIOD][idx]).any(-1).nonzero().flatten()
    assert bad.numel() == 0, (dt, build, of, t, int(bad.numel()), bad[:8].tolist())


def test_ring_later_tiles_walk_one_to_four():
    """Over the family the workgroups walk 1, 2, 3 and 4 row tiles, and every build sees an odd and an even count (from the plan: no launch)."""
    every = set()
    for (dt, build, of, t) in LATER_PARAMS:
        _, _, _, _, lo, hi = R.later_shape(build, dt, _n_cu(), t)
        assert hi == lo + 1
        every |= {lo, hi}
    assert every >= {1, 2, 3, 4}, every


@pytest.mark.parametrize("dt", R.DTS)
def test_ring_independence(dt):
    M, K, N, of = 300, 128, 232, 0
    a, w, b, res = R.value_case(M, K, N, dt, of, 7)
    out = run_twice(a, w, b, res, R.ACT_GELU, 0, dt, of)
    a2 = a.clone()
    a2[77] = R.round_to(a[77] * 1.5 + 0.25, dt)
    out2 = run_gemm(a2, w, b, res, R.ACT_GELU, 0, dt, of)
    keep = torch.arange(M, device="cuda") != 77
    assert torch.equal(out[keep], out2[keep]) and not torch.equal(out[77], out2[77])
    n = 100
    assert float(w[n].abs().max()) < float(w.abs().max())     # (f16x2: the layer's weight scale, a function of max |w|, stays)
    w2, b2 = w.clone(), b.clone()
    w2[n] = R.round_to(w[n] * 0.5, dt)
    b2[n] = b[n] + 1.0
    out3 = run_gemm(a, w2, b2, res, R.ACT_GELU, 0, dt, of)
    keep = torch.arange(N, device="cuda") != n
    assert torch.equal(out[:, keep], out3[:, keep]) and not torch.equal(out[:, n], out3[:, n])
