"""GPU: the detector's stem -- stem_pool_kernel (csrc/stem_pool.hip: conv 7x7 / 2 + bias + ReLU + max-pool 3x3 / 2 in one f16x2 kernel) and
the two-kernel form that every other element type runs (conv_gemm's rows mode, then k_maxpool3x3s2; `fused = 0`, all four types) -- through
ocrvi_test_stem_pool_raw, every pooled element held to the float64 reference of tests/halo_refs.py: equal to it on routed and probe data,
within stem_bound (gemm_refs.gemm_bound of the type per conv pixel, its maximum over the pool window) on value data.
tests/test_halo_refs_cpu.py shows on the CPU that an fp32 emulation does the same on these cases and that wrong kernels do not.  The fused
cases first assert the tiling through ocrvi_test_halo_plan with the device's CU count; every case runs twice into a NaN-filled output with
128 guard rows of a NaN payload behind it: bit-identical runs, every element finite, guards untouched.  No element is excluded; a failure
names (image, y, x, channel, got, want) in pooled coordinates.

  routed        routed_stem_case: integers, 0 / +-1 weights using every (filter row, pixel, channel): output == reference
  probe a       impulses of +-2^e seven pixels apart (no 7x7 window holds two), the channel running over the three, full-width Gaussian
                weights: every conv pixel is one weight times a power of two, every pooled one the largest of nine such
  probe b       one-hot weights at the channel's own (row, pixel, channel) in three launches, value data: a pooled, shifted copy of x
  value         value_stem_case (Gaussian, cancelling, 2^-10 and outlier image rows; the bias sweeps [-12, 12]): err <= bound everywhere
  independence  one input element changed: only the pooled pixels its 7x7 reach maps to change bits; one output channel's weights and bias:
                only that channel (fused form)
  later tiles   routed, DISTINCT 96x84 images (3 x 3 tiles) making the workgroups walk 1 and 2, then 3 tiles, on a grid no multiple of 9
Shapes: halo_refs.STEM_SHAPES, the fused form and the two-kernel form in f32, f16x2, bf16 and f16.

Measured on the MI355X (256 CUs): 124 tests, 3.0 s for the file, the slowest test 0.33 s.  Largest err / bound of the value family:
                fused f16x2   two kernels: f32   f16x2    bf16     f16
  GPU           0.0080                     0.0389  0.0084   0.9940   0.9708
  CPU emulation 0.004                      0.010   0.004    0.994    0.971
(the 16-bit figures near 1 are elements whose whole error is the last rounding to T next to a tie); every other family is an equality
and holds.  The later-tiles launches walked 1, 2 and 3 tiles per workgroup.  Nothing was found wrong in either form.
profiles/r27_halo_elements.md has the CPU tables and the mutant-by-family matrix.
"""
import time

import numpy as np
import pytest
import torch

import gemm_refs as G
import halo_refs as Hh
from test_gpu_conv3_halo_elements import _L, assert_plan, bits, check_written, equal, h, hold, n_cu, raw_buffer, twice

pytestmark = pytest.mark.gpu

WORST = {}
WALKED = set()
FORMS = [("f16x2", 1)] + [(dt, 0) for dt in Hh.STEM_DTS]
FORM_IDS = ["fused"] + [f"two-kernel-{dt}" for dt in Hh.STEM_DTS]
IDS = [f"{n}x{H}x{W}" for (n, H, W) in Hh.STEM_SHAPES]


def run_stem(x, w, b, dt, fused):
    """One launch: pooled rows [n H/4 W/4, 64] float32 on the GPU."""
    L = _L()
    n, _, H, W = x.shape
    raw, guard = raw_buffer(n * (H // 4) * (W // 4), 64, 4 if dt in ("f32", "f16x2") else 2)
    out = torch.full((n, 64, H // 4, W // 4), float("nan"), device="cuda")
    xd = x.cuda().contiguous()
    wh, bh = h(w), h(b)
    L.check(L.load().ocrvi_test_stem_pool_raw(0, G.DT_CODE[dt], xd.data_ptr(), wh.ctypes.data, bh.ctypes.data, n, H, W, fused, raw.data_ptr(), out.data_ptr()))
    check_written(guard, out, f"stem {dt} fused {fused}")
    return Hh.rows_of(out).contiguous()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[stem summary] {time.time() - t0:.1f} s; largest err / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
    print(f"[stem summary] tiles per workgroup walked in the later-tiles family: {sorted(WALKED)}")


def _plan(n, H, W, fused):
    if fused:
        assert_plan(2, n, 3, H, W, 64)


@pytest.mark.parametrize("dt,fused", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(Hh.STEM_SHAPES)), ids=IDS)
def test_stem_routed(i, dt, fused):
    n, H, W = Hh.STEM_SHAPES[i]
    _plan(n, H, W, fused)
    x, w, b = Hh.routed_stem_case(n, H, W, 3 + i)
    equal(twice(run_stem, x, w, b, dt, fused), Hh.stem_ref(x, w, b), n, H // 4, W // 4, ("routed", IDS[i], dt, fused))


@pytest.mark.parametrize("dt,fused", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(Hh.STEM_SHAPES)), ids=IDS)
def test_stem_probe_impulses(i, dt, fused):
    n, H, W = Hh.STEM_SHAPES[i]
    _plan(n, H, W, fused)
    for l in range(Hh.probe_a_launches(n, 3, H, W, 7)):
        x, w, b = Hh.probe_a_stem_case(n, H, W, l, dt, 7 + i)
        equal(twice(run_stem, x, w, b, dt, fused), Hh.stem_ref(x, w, b), n, H // 4, W // 4, ("probe a", IDS[i], dt, fused, l))


@pytest.mark.parametrize("dt,fused", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(Hh.STEM_SHAPES)), ids=IDS)
def test_stem_probe_one_hot_weights(i, dt, fused):
    n, H, W = Hh.STEM_SHAPES[i]
    _plan(n, H, W, fused)
    for l in range(Hh.probe_b_launches(147, 64)):
        x, w, b = Hh.probe_b_stem_case(n, H, W, l, dt, 9 + i)
        equal(twice(run_stem, x, w, b, dt, fused), Hh.stem_ref(x, w, b), n, H // 4, W // 4, ("probe b", IDS[i], dt, fused, l))


@pytest.mark.parametrize("dt,fused", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(Hh.STEM_SHAPES)), ids=IDS)
def test_stem_value(i, dt, fused):
    n, H, W = Hh.STEM_SHAPES[i]
    _plan(n, H, W, fused)
    x, w, b = Hh.value_stem_case(n, H, W, dt, 5 + i)
    hold(twice(run_stem, x, w, b, dt, fused), Hh.stem_ref(x, w, b), Hh.stem_bound(x, w, b, dt), n, H // 4, W // 4,
         f"value {dt} {'fused' if fused else 'two kernels'}", IDS[i], WORST)


def test_stem_independence():
    n, H, W = 3, 36, 52
    _plan(n, H, W, 1)
    x, w, b = Hh.value_stem_case(n, H, W, "f16x2", 23)
    b = b.abs() + 1.0                                                    # (every channel alive behind the ReLU)
    OH, OW = H // 4, W // 4
    out = bits(twice(run_stem, x, w, b, "f16x2", 1)).reshape(n, OH, OW, 64)
    i0, c0, y0, x0 = 2, 1, 31, 28                                       # next to the tile boundaries (pooled row 8, column 7) of the last image
    x2 = x.clone()
    x2[i0, c0, y0, x0] = Hh.round_to(x[i0, c0, y0, x0] * 1.5 + 4.0, "f16x2")
    out2 = bits(run_stem(x2, w, b, "f16x2", 1)).reshape(n, OH, OW, 64)
    # conv pixels cy with |y0 + 3 - 2 cy - 3| <= 3, pooled pixels py with |cy - 2 py| <= 1
    cy = [c for c in range(H // 2) if abs(y0 - 2 * c) <= 3]
    cx = [c for c in range(W // 2) if abs(x0 - 2 * c) <= 3]
    reach = torch.zeros(n, OH, OW, dtype=torch.bool, device="cuda")
    for py in range(OH):
        for px in range(OW):
            if any(abs(c - 2 * py) <= 1 for c in cy) and any(abs(c - 2 * px) <= 1 for c in cx):
                reach[i0, py, px] = True
    assert torch.equal(out[~reach], out2[~reach]), "a pooled pixel outside the element's reach changed"
    assert not torch.equal(out[reach], out2[reach])
    ch = 37
    assert float(w[ch].abs().max()) < float(w.abs().max())
    w2, b2 = w.clone(), b.clone()
    w2[ch] = Hh.round_to(w[ch] * 0.5, "f16x2")
    b2[ch] = b[ch] + 1.0
    out3 = bits(run_stem(x, w2, b2, "f16x2", 1)).reshape(n, OH, OW, 64)
    keep = torch.arange(64, device="cuda") != ch
    assert torch.equal(out[..., keep], out3[..., keep]) and not torch.equal(out[..., ch], out3[..., ch])


@pytest.mark.parametrize("t", (2, 3))
def test_stem_later_tiles(t):
    """A workgroup's second and third tiles: the patch fetched two tiles ahead into registers, put into LDS under the pooling pass of the
    tile before, the staging reused behind barrier B."""
    n, grid, lo, hi = Hh.later_shape(2, n_cu(), t)
    plan = assert_plan(2, n, 3, 96, 84, 64)
    assert plan[3:5] == (3, 3) and plan[5:] == (grid, lo, hi) and hi == t and grid % 9
    WALKED.update((lo, hi))
    x, w, b = Hh.routed_stem_case(n, 96, 84, 60 + t)
    equal(twice(run_stem, x, w, b, "f16x2", 1), Hh.stem_ref(x, w, b), n, 24, 21, ("later", n, lo, hi))


def test_stem_pool_raw_refuses_the_fused_kernel_for_other_types():
    L = _L()
    raw, _ = raw_buffer(64, 64, 2)
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    out = torch.empty(1, 64, 8, 8, device="cuda")
    w, b = np.zeros((64, 3, 7, 7), np.float32), np.zeros(64, np.float32)
    with pytest.raises(ValueError):
        L.check(L.load().ocrvi_test_stem_pool_raw(0, G.DT_CODE["f16"], x.data_ptr(), w.ctypes.data, b.ctypes.data, 1, 32, 32, 1, raw.data_ptr(), out.data_ptr()))
