"""GPU: LocalMixing's grouped 3x3 convolutions -- gconv32_kernel (csrc/gconv32.h; bf16, f16; both output builds) and
conv_gemm_kernel<T, AM_CONV3, 128, 32, 4, 1> (f32, f16x2; the 16-bit types with a 16-bit residual, or with OCRVI_GCONV32=0) -- and the
recogniser's strided conv_gemm 3x3 layers (PatchMerging, stem2) through ocrvi_test_conv_raw, every element held to the float64 reference
of tests/conv_refs.py: equal to it on routed integer data, within conv_bound (gemm_refs.gemm_bound on each group's im2col matrix) on value
data.  tests/test_conv_refs_cpu.py shows on the CPU that an fp32 emulation of either kernel stays inside the bound on exactly these cases
and that wrong kernels leave it.  Every case first asserts the kernel and the tiling it reaches through ocrvi_test_gconv_plan with the
device's CU count, then runs twice into a NaN-filled output with 128 guard rows of a NaN payload behind it: the two runs must be
bit-identical, all elements finite, the guard rows untouched.  No element is excluded from any comparison.

  routing       routed_case (integers, 9 to 12 weights of +-1 per output channel, every (tap, channel) of every group used, no two weight
                rows alike): output == reference.  The nine shapes of conv_refs.ROUTE_SHAPES (th = 1, 2, 3, 4; one fragment; a last block, a
                last band and a last column band of one pixel; 4, 8 and 12 groups) x ROUTE_VARIANTS (both output builds; no residual, after
                and before the ReLU; a 16-bit residual; a residual without activation)
  value         value_case (Gaussian, cancelling, 2^-10-scaled and one-outlier image rows; the bias sweeps GELU over [-12, 12]) on 2x6x80 and
                1x7x100: three activations, no residual and both orders
  in place      LocalMixing's conv2 call (fp32 output, fp32 residual, GELU, res_post) with residual and output in ONE buffer: bit-equal to
                the call with separate buffers (and held to the bound)
  later tiles   identical 9x16 images of 384 channels on launches whose workgroups walk 1 and 2, then 3 and 4 tiles (a workgroup's consecutive
                tiles lie at different heights of the image): image 0 is held to the bound, every later image is bit-equal to it (compared
                on the device)
  independence  one input element changed: only its 3x3 reach in its group changes bits; one output channel's weights and bias changed:
                only that channel does
  strided       128 -> 256 at stride (2, 1) (fp32 and T output, none / ReLU) and 64 -> 128 at stride 2: routing (none and ReLU: the GELU of
                an integer is none) and value (PatchMerging: no activation, fp32 output; stem2: GELU, fp32 output)
  fallback      one fresh child process with OCRVI_GCONV32=0: the routing shapes and variants in bf16 and f16 on conv_gemm's 64-element
                K-step with its half-padded last step: output == reference

Largest err / bound per family and type, measured on the MI355X (256 CUs; 98 tests, 9.4 s for the file; the slowest test 3.3 s, the child
process of the fallback, which loads torch and the library again; then 0.63 s, the first, which loads the library):
                f32      f16x2    bf16     f16
  value         0.315    0.456    0.999    0.996
  in place      0.328    0.238    0.302    0.259
  later tiles   -        -        0.992    0.963
  strided       0.148    0.055    0.125    0.125
(routing, independence, the in-place comparison, the later images and the fallback are equalities; the later-tiles family is gconv32's.
The CPU emulation gives 0.315 / 0.456 / 0.999 / 0.996, 0.328 / 0.238 / 0.302 / 0.259, 0.289 / 0.220 / 0.992 / 0.963 and 0.150 / 0.051 / 0.125 /
0.125: the 16-bit figures near 1 are elements whose whole error is the last rounding to T next to a tie.  Nothing was found wrong in either
kernel or in the launchers.  conv_gemm's plain epilogue is not reached: these layers' outputs are 16-byte aligned rows of whole 16-byte
chunks, which is what launch_conv sends through the LDS-staged one.  profiles/r19_grouped_conv.md has the CPU tables.)
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import conv_refs as R
from test_gpu_kernels import DT

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 128                      # rows behind the output
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
GCONV32_ON = os.environ.get("OCRVI_GCONV32", "1") != "0"      # (as csrc/gconv32.h reads it; 0 only in the fallback test's child)
WORST = {}
WALKED = set()
GROUPS = lambda C: C // 32


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_plan(dt, x, Co, stride, groups, of, has_res, tiling=None):
    n, C, H, W = x.shape
    plan = R.plan_of(_L().load(), dt, n, C, H, W, Co, stride, groups, of, has_res, _n_cu())
    assert plan == R.expect_plan(dt, n, C, H, W, Co, stride, groups, of, has_res, _n_cu(), GCONV32_ON), (dt, tuple(x.shape), Co, stride, of, has_res, plan)
    if tiling is not None and plan[0] == 1:
        assert plan[3:7] == tiling, (dt, tuple(x.shape), plan)
    return plan


def run_conv(x, w, b, res, stride, groups, act, res_post, dt, of, in_place=False):
    """One launch (x, res: CPU or GPU float32 NCHW): the output as rows [n Ho Wo, Co] float32 on the GPU.  Guards and NaNs are checked here."""
    L = _L()
    n, C, H, W = x.shape
    Co = w.shape[0]
    Ho, Wo = R.out_hw(H, W, stride)
    M = n * Ho * Wo
    esz = 4 if (of or dt in ("f32", "f16x2")) else 2
    raw = torch.full(((M + GUARD) * Co * esz,), 0xFF, dtype=torch.uint8, device="cuda")        # every element a NaN
    guard = raw[M * Co * esz:].view(torch.int32)
    guard.fill_(X_GUARD)
    out = torch.full((n, Co, Ho, Wo), float("nan"), device="cuda")
    xd = x.cuda().contiguous()
    rd = None if res is None else res.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_conv_raw(0, DT[dt], xd.data_ptr(), wh.ctypes.data, bh.ctypes.data, None if rd is None else rd.data_ptr(),
                                         n, C, H, W, Co, 3, stride[0], stride[1], groups, act, int(res_post), int(of), int(in_place),
                                         raw.data_ptr(), out.data_ptr()))
    torch.cuda.synchronize()
    assert bool((guard == X_GUARD).all()), "the guard rows behind the output changed"
    assert bool(torch.isfinite(out).all()), "an element of the output was not written (or is not finite)"
    return R.rows_of(out).contiguous()


def _bits(t):
    return t.view(torch.int32)


def run_twice(*a, **k):
    out = run_conv(*a, **k)
    assert torch.equal(_bits(out), _bits(run_conv(*a, **k))), "two runs differ"
    return out


def _hold(out, ref, bound, family, dt, tag):
    q = R.err_ratio(out.cpu(), ref, bound)
    worst = float(q.max())
    print(f"\n[gconv {family} {dt} {tag}] max err / bound {worst:.3f}")
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), worst)
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (family, dt, tag, worst, bad[:8].tolist())


def _equal(out, ref, tag):
    o = out.cpu()
    bad = (o.double() != ref).nonzero()
    assert bad.numel() == 0, (tag, int(bad.shape[0]), [(r, c, float(o[r, c]), float(ref[r, c])) for r, c in bad[:8].tolist()])


FAMILIES = ("value", "in place", "later", "strided")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[gconv summary] {time.time() - t0:.1f} s; largest err / bound per family and type")
    for fam in FAMILIES:
        print(f"[gconv summary] {fam:8s} " + "   ".join(f"{dt} " + (f"{WORST[(fam, dt)]:.3f}" if (fam, dt) in WORST else "-") for dt in R.DTS))
    print(f"[gconv summary] tiles per workgroup walked in the later-tiles family: {sorted(WALKED)}")


def _routing(dt, i):
    (n, C, H, W), tiling = R.ROUTE_SHAPES[i]
    for (of, rp, act) in R.ROUTE_VARIANTS:
        x, w, b, res = R.routed_case(n, C, H, W, C, (1, 1), GROUPS(C), 11 + i, with_res=rp is not None)
        _assert_plan(dt, x, C, (1, 1), GROUPS(C), of, rp is not None, tiling)
        out = run_twice(x, w, b, res, (1, 1), GROUPS(C), act, rp or 0, dt, of)
        _equal(out, R.conv_ref(x, w, b, res, (1, 1), GROUPS(C), act, rp or 0), (dt, n, C, H, W, of, rp, act))


@pytest.mark.parametrize("i", range(len(R.ROUTE_SHAPES)))
@pytest.mark.parametrize("dt", R.DTS)
def test_gconv_routing(dt, i):
    _routing(dt, i)


@pytest.mark.parametrize("shape", R.VALUE_SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
def test_gconv_value(dt, shape):
    n, C, H, W = shape
    for (of, rp, act) in R.VALUE_VARIANTS:
        x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPS(C), dt, of, 5)
        res = res if rp is not None else None
        _assert_plan(dt, x, C, (1, 1), GROUPS(C), of, rp is not None)
        out = run_twice(x, w, b, res, (1, 1), GROUPS(C), act, rp or 0, dt, of)
        _hold(out, R.conv_ref(x, w, b, res, (1, 1), GROUPS(C), act, rp or 0), R.conv_bound(x, w, b, res, (1, 1), GROUPS(C), act, rp or 0, dt, of),
              "value", dt, f"{n}x{H}x{W} out_f32 {of} res {rp} act {act}")


@pytest.mark.parametrize("dt", R.DTS)
def test_gconv_in_place(dt):
    """rec_model.hip runs LocalMixing's conv2 with the fp32 residual stream as residual AND output: every element's residual is read by the
    lane that writes it, before it writes it."""
    n, C, H, W = R.IN_PLACE_SHAPE
    x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPS(C), dt, 1, 6)
    _assert_plan(dt, x, C, (1, 1), GROUPS(C), 1, True, (3, 5, 2, 1))
    apart = run_twice(x, w, b, res, (1, 1), GROUPS(C), R.ACT_GELU, 1, dt, 1)
    inpl = run_twice(x, w, b, res, (1, 1), GROUPS(C), R.ACT_GELU, 1, dt, 1, in_place=True)
    _hold(apart, R.conv_ref(x, w, b, res, (1, 1), GROUPS(C), R.ACT_GELU, 1), R.conv_bound(x, w, b, res, (1, 1), GROUPS(C), R.ACT_GELU, 1, dt, 1),
          "in place", dt, "separate buffers")
    bad = (_bits(apart) != _bits(inpl)).nonzero()
    assert bad.numel() == 0, (dt, int(bad.shape[0]), bad[:8].tolist())


@pytest.mark.parametrize("t", (2, 4))
@pytest.mark.parametrize("of", (0, 1))
@pytest.mark.parametrize("dt", ("bf16", "f16"))
def test_gconv_later_tiles_equal_the_first(dt, of, t):
    """gconv32's next-tile prefetch: fetch(next) into registers before the MFMAs, stage(next) into LDS after the barrier."""
    n, C, H, W, grid, lo, hi = R.later_shape(_n_cu(), t)
    x1, w, b, r1 = R.value_case(1, C, H, W, C, (1, 1), GROUPS(C), dt, of, 21)
    r1 = r1 if of else None                                    # (a residual only as the fp32 stream beside an fp32 output)
    x = x1.cuda().expand(n, -1, -1, -1)
    res = None if r1 is None else r1.cuda().expand(n, -1, -1, -1)
    plan = _assert_plan(dt, x, C, (1, 1), GROUPS(C), of, bool(of), (3, 1, 3, 1))
    assert plan[0] == 1 and plan[7:10] == (grid, lo, hi) and hi == lo + 1 and grid % 3
    WALKED.update((lo, hi))
    out = run_twice(x, w, b, res, (1, 1), GROUPS(C), R.ACT_GELU, 1, dt, of)
    M1 = H * W
    _hold(out[:M1], R.conv_ref(x1, w, b, r1, (1, 1), GROUPS(C), R.ACT_GELU, 1), R.conv_bound(x1, w, b, r1, (1, 1), GROUPS(C), R.ACT_GELU, 1, dt, of),
          "later", dt, f"out_f32 {of} n {n} tiles {lo}/{hi}")
    o3 = _bits(out).reshape(n, M1, C)
    bad = (o3 != o3[:1]).any(-1).nonzero()
    assert bad.numel() == 0, (dt, of, t, int(bad.shape[0]), bad[:8].tolist())


def test_gconv_later_tiles_walk_one_to_four():
    """Over the family the workgroups walk 1, 2, 3 and 4 tiles (from the plan: no launch)."""
    every = set()
    for t in (2, 4):
        *_, lo, hi = R.later_shape(_n_cu(), t)
        assert hi == lo + 1
        every |= {lo, hi}
    assert every >= {1, 2, 3, 4}, every


@pytest.mark.parametrize("of", (0, 1))
@pytest.mark.parametrize("dt", R.DTS)
def test_gconv_independence(dt, of):
    n, C, H, W = R.INDEP_SHAPE
    groups = GROUPS(C)
    x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), groups, dt, of, 7)
    res = res if of else None
    _assert_plan(dt, x, C, (1, 1), groups, of, bool(of))
    run = lambda x_, w_, b_: run_conv(x_, w_, b_, res, (1, 1), groups, R.ACT_GELU, 1, dt, of)
    out = _bits(run_twice(x, w, b, res, (1, 1), groups, R.ACT_GELU, 1, dt, of)).reshape(n, H, W, C)
    i0, c0, y0, x0 = 1, 40, 2, 37                              # image 1, channel 40 (group 1), row 2, column 37
    x2 = x.clone()
    x2[i0, c0, y0, x0] = R.round_to(x[i0, c0, y0, x0] * 1.5 + 0.25, dt)
    out2 = _bits(run(x2, w, b)).reshape(n, H, W, C)
    reach = torch.zeros(n, H, W, C, dtype=torch.bool, device="cuda")
    reach[i0, y0 - 1:y0 + 2, x0 - 1:x0 + 2, 32:64] = True
    assert torch.equal(out[~reach], out2[~reach]), "an output outside the element's 3x3 reach and group changed"
    assert not torch.equal(out[reach], out2[reach])
    ch = 77
    assert float(w[ch].abs().max()) < float(w.abs().max())     # (f16x2: the layer's weight scale, a function of max |w|, stays)
    w2, b2 = w.clone(), b.clone()
    w2[ch] = R.round_to(w[ch] * 0.5, dt)
    b2[ch] = b[ch] + 1.0
    out3 = _bits(run(x, w2, b2)).reshape(n, H, W, C)
    keep = torch.arange(C, device="cuda") != ch
    assert torch.equal(out[..., keep], out3[..., keep]) and not torch.equal(out[..., ch], out3[..., ch])


@pytest.mark.parametrize("i", range(len(R.STRIDED)))
@pytest.mark.parametrize("dt", R.DTS)
def test_strided_conv_gemm_routing(dt, i):
    n, C, H, W, Co, stride, (of, _) = R.STRIDED[i]
    x, w, b, _ = R.routed_case(n, C, H, W, Co, stride, 1, 31 + i, with_res=False)
    for o in (of, 0):
        assert _assert_plan(dt, x, Co, stride, 1, o, False)[:3] == (0, 128, 128)
        for act in (R.ACT_NONE, R.ACT_RELU):
            out = run_twice(x, w, b, None, stride, 1, act, 0, dt, o)
            _equal(out, R.conv_ref(x, w, b, None, stride, 1, act, 0), (dt, R.STRIDED[i], o, act))


@pytest.mark.parametrize("i", range(len(R.STRIDED)))
@pytest.mark.parametrize("dt", R.DTS)
def test_strided_conv_gemm_value(dt, i):
    n, C, H, W, Co, stride, (of, act) = R.STRIDED[i]
    x, w, b, _ = R.value_case(n, C, H, W, Co, stride, 1, dt, of, 9)
    assert _assert_plan(dt, x, Co, stride, 1, of, False)[:3] == (0, 128, 128)
    out = run_twice(x, w, b, None, stride, 1, act, 0, dt, of)
    _hold(out, R.conv_ref(x, w, b, None, stride, 1, act, 0), R.conv_bound(x, w, b, None, stride, 1, act, 0, dt, of), "strided", dt,
          f"{n}x{H}x{W} {C}->{Co} stride {stride} act {act}")


def fallback_body():
    """Runs in the child of test_gconv32_off_falls_back_to_conv_gemm: OCRVI_GCONV32=0, read once per process by the library."""
    assert not GCONV32_ON
    done = 0
    for dt in ("bf16", "f16"):
        for i, ((n, C, H, W), _) in enumerate(R.ROUTE_SHAPES):
            for (of, rp, act) in R.ROUTE_VARIANTS:
                plan = R.plan_of(_L().load(), dt, n, C, H, W, C, (1, 1), GROUPS(C), of, rp is not None, _n_cu())
                assert plan[:3] == (0, 128, 32) and plan[11] == 5, plan       # conv_gemm, 4.5 K-steps of 64 elements
            _routing(dt, i)
            done += 1
    print(f"fallback ok {done}")


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_grouped_conv as T
T.fallback_body()
"""


def test_gconv32_off_falls_back_to_conv_gemm():
    """conv_gemm's 16-bit 3x3 mode at 32 channels per group: K = 288 is four and a half 64-element K-steps, the last one half padding (the
    tenth tap, masked in the A operand and zero in the packed weights)."""
    env = dict(os.environ, OCRVI_GCONV32="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"fallback ok {2 * len(R.ROUTE_SHAPES)}" in r.stdout, r.stdout[-2000:]
