"""GPU: conv3_halo_kernel (csrc/conv3_halo.h: the f16x2 detector's FPN smoothing convs, head_conv and layer1 conv2) through
ocrvi_test_conv3_halo_raw, every element held to the float64 reference of tests/halo_refs.py: equal to it on routed and probe data, within
conv_bound (gemm_refs.gemm_bound on the im2col matrix) on value data.  tests/test_halo_refs_cpu.py shows on the CPU that an fp32 emulation
of the kernel does the same on these cases and that wrong kernels do not.  Every case first asserts, through ocrvi_test_halo_plan with the
device's CU count, that it takes conv3_halo and the tiling it means, then runs twice into a NaN-filled output with 128 guard rows of a NaN
payload behind it: the two runs must be bit-identical, every element finite, the guard rows untouched.  No element is excluded anywhere; a
failure names (image, y, x, channel, got, want).

  routed        routed_conv_case: integers, 0 / +-1 weights using every (tap, channel) inside every column tile: output == reference
  probe a       impulses of +-2^e, one per 3x3 window, the impulse channel running over all Cin (in as many launches as that takes), full-width
                Gaussian weights: every output is one weight times a power of two -- both halves of every weight at every tap
  probe b       one-hot weights 2^e at the channel's own (tap, channel), value data with fp16-subnormal lo halves: the output is a shifted copy
                of x or 0 in the halo -- both halves of every activation, every (tap, channel) in ceil(9 Cin / Co) launches
  value         conv_refs.value_case (Gaussian, cancelling, 2^-10 and outlier rows; the bias sweeps [-12, 12]): err <= bound everywhere
  independence  one input element changed: only its 3x3 reach changes bits; one output channel's weights and bias: only that channel
  later tiles   routed, DISTINCT 48x48 images, as many as make the workgroups walk 1 and 2, then 3 tiles on a grid that is no multiple of
                the 9 tiles of an image: 32 -> 64 (the patch stage switches at every tile), 64 -> 128, 64 -> 256 (two column tiles)
All families run the eight shapes of halo_refs.CONV_SHAPES with no activation and with ReLU (the probes alternate them by launch).

Measured on the MI355X (256 CUs): 42 tests, 5.0 s for the file, the slowest test 0.56 s (the first, which loads the library).  Largest
err / bound of the value family 0.0059 (the CPU emulation: 0.006; per shape 0.0004 .. 0.0059 -- gemm_bound charges each of the 3 K + 1
partial products a full rounding of the sum of magnitudes); every other family is an equality and holds.  The later-tiles launches walked
1, 2 and 3 tiles per workgroup.  Nothing was found wrong in the kernel, the packer or the launcher.  profiles/r27_halo_elements.md has the
CPU tables and the mutant-by-family matrix.
"""
import os
import time

import numpy as np
import pytest
import torch

import halo_refs as Hh
from halo_refs import ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

GUARD = 128                      # rows behind the output
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
WORST = {}
WALKED = set()


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def h(t):
    return np.ascontiguousarray(t.numpy(), dtype=np.float32)


def bits(t):
    return t.view(torch.int32)


def assert_plan(kind, n, C, H, W, Co):
    """The launch takes the kernel named, on the tiling halo_refs computes for this device."""
    plan = Hh.plan_of(_L().load(), kind, n, C, H, W, Co, n_cu())
    assert plan == Hh.expect_plan(kind, n, C, H, W, Co, n_cu()), (kind, n, C, H, W, Co, plan)
    return plan


def raw_buffer(rows, C, esz=4):
    """(buffer, guard): rows x C elements of 0xFF bytes (every f16x2, fp32, fp16 or bf16 element a NaN), then GUARD rows of X_GUARD."""
    raw = torch.full(((rows + GUARD) * C * esz,), 0xFF, dtype=torch.uint8, device="cuda")
    guard = raw[rows * C * esz:].view(torch.int32)
    guard.fill_(X_GUARD)
    return raw, guard


def check_written(guard, out, what):
    torch.cuda.synchronize()
    assert bool((guard == X_GUARD).all()), f"{what}: the guard rows behind the output changed"
    assert bool(torch.isfinite(out).all()), f"{what}: an element of the output was not written (or is not finite)"


def run_conv(x, w, b, act):
    """One launch (x: CPU or GPU float32 NCHW): the output as rows [n H W, Co] float32 on the GPU."""
    L = _L()
    n, C, H, W = x.shape
    Co = w.shape[0]
    raw, guard = raw_buffer(n * H * W, Co)
    out = torch.full((n, Co, H, W), float("nan"), device="cuda")
    xd = x.cuda().contiguous()
    wh, bh = h(w), h(b)
    L.check(L.load().ocrvi_test_conv3_halo_raw(0, xd.data_ptr(), wh.ctypes.data, bh.ctypes.data, n, C, H, W, Co, act, raw.data_ptr(), out.data_ptr()))
    check_written(guard, out, "conv3_halo")
    return Hh.rows_of(out).contiguous()


def twice(run, *a):
    out = run(*a)
    again = run(*a)
    for o, p in zip(out if isinstance(out, tuple) else (out,), again if isinstance(again, tuple) else (again,)):
        assert o is None or torch.equal(bits(o), bits(p)), "two runs differ"
    return out


def where(bad, n, H, W, got, ref):
    """The first few failing elements as (image, y, x, channel, got, want)."""
    return [(r // (H * W), r // W % H, r % W, c, float(got[r, c]), float(ref[r, c])) for r, c in bad[:6].tolist()]


def equal(out, ref, n, H, W, tag):
    o = out.cpu()
    bad = (o.double() != ref).nonzero()
    assert bad.numel() == 0, (tag, int(bad.shape[0]), where(bad, n, H, W, o, ref))


def hold(out, ref, bound, n, H, W, family, tag, worst=WORST):
    o = out.cpu()
    q = Hh.err_ratio(o, ref, bound)
    top = float(q.max())
    print(f"\n[halo {family} {tag}] max err / bound {top:.4f}")
    worst[family] = max(worst.get(family, 0.0), top)
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (family, tag, top, where(bad, n, H, W, o, ref))


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[conv3_halo summary] {time.time() - t0:.1f} s; largest err / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
    print(f"[conv3_halo summary] tiles per workgroup walked in the later-tiles family: {sorted(WALKED)}")


IDS = [f"{n}x{C}x{H}x{W}-{Co}" for (n, C, H, W, Co) in Hh.CONV_SHAPES]


@pytest.mark.parametrize("i", range(len(Hh.CONV_SHAPES)), ids=IDS)
def test_conv3_halo_routed(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    assert_plan(0, n, C, H, W, Co)
    x, w, b = Hh.routed_conv_case(n, C, H, W, Co, 3 + i)
    for act in (ACT_NONE, ACT_RELU):
        equal(twice(run_conv, x, w, b, act), Hh.conv_ref(x, w, b, act), n, H, W, ("routed", IDS[i], act))


@pytest.mark.parametrize("i", range(len(Hh.CONV_SHAPES)), ids=IDS)
def test_conv3_halo_probe_impulses(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    assert_plan(0, n, C, H, W, Co)
    for l in range(Hh.probe_a_launches(n, C, H, W)):
        x, w, b = Hh.probe_a_conv_case(n, C, H, W, Co, l, 7 + i)
        act = (ACT_NONE, ACT_RELU)[l % 2]
        equal(twice(run_conv, x, w, b, act), Hh.conv_ref(x, w, b, act), n, H, W, ("probe a", IDS[i], l))


@pytest.mark.parametrize("i", range(len(Hh.CONV_SHAPES)), ids=IDS)
def test_conv3_halo_probe_one_hot_weights(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    assert_plan(0, n, C, H, W, Co)
    for l in range(Hh.probe_b_launches(9 * C, Co)):
        x, w, b = Hh.probe_b_conv_case(n, C, H, W, Co, l, 9 + i)
        act = (ACT_NONE, ACT_RELU)[l % 2]
        equal(twice(run_conv, x, w, b, act), Hh.conv_ref(x, w, b, act), n, H, W, ("probe b", IDS[i], l))


@pytest.mark.parametrize("i", range(len(Hh.CONV_SHAPES)), ids=IDS)
def test_conv3_halo_value(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    assert_plan(0, n, C, H, W, Co)
    x, w, b = Hh.value_conv_case(n, C, H, W, Co, 5 + i)
    for act in (ACT_NONE, ACT_RELU):
        hold(twice(run_conv, x, w, b, act), Hh.conv_ref(x, w, b, act), Hh.conv_bound(x, w, b, act), n, H, W, "value", f"{IDS[i]} act {act}")


@pytest.mark.parametrize("i", (4, 6, 7), ids=[IDS[4], IDS[6], IDS[7]])
def test_conv3_halo_independence(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    assert_plan(0, n, C, H, W, Co)
    x, w, b = Hh.value_conv_case(n, C, H, W, Co, 15 + i)
    out = bits(twice(run_conv, x, w, b, ACT_NONE)).reshape(n, H, W, Co)
    i0, c0, y0, x0 = n - 1, C - 5, H - 2, min(16, W - 2)             # the last image, next to the bottom edge, at a tile boundary across
    x2 = x.clone()
    x2[i0, c0, y0, x0] = Hh.round_to(x[i0, c0, y0, x0] * 1.5 + 0.25, Hh.DT)
    out2 = bits(run_conv(x2, w, b, ACT_NONE)).reshape(n, H, W, Co)
    reach = torch.zeros(n, H, W, Co, dtype=torch.bool, device="cuda")
    reach[i0, y0 - 1:y0 + 2, x0 - 1:x0 + 2] = True
    assert torch.equal(out[~reach], out2[~reach]), "an output outside the element's 3x3 reach changed"
    assert not torch.equal(out[reach], out2[reach])
    ch = Co - 3
    assert float(w[ch].abs().max()) < float(w.abs().max())            # (the layer's weight scale, a function of max |w|, stays)
    w2, b2 = w.clone(), b.clone()
    w2[ch] = Hh.round_to(w[ch] * 0.5, Hh.DT)
    b2[ch] = b[ch] + 1.0
    out3 = bits(run_conv(x, w2, b2, ACT_NONE)).reshape(n, H, W, Co)
    keep = torch.arange(Co, device="cuda") != ch
    assert torch.equal(out[..., keep], out3[..., keep]) and not torch.equal(out[..., ch], out3[..., ch])


@pytest.mark.parametrize("t", (2, 3))
@pytest.mark.parametrize("C,Co", Hh.LATER_CONV)
def test_conv3_halo_later_tiles(C, Co, t):
    """A workgroup's second and third tiles: the counted waits across the tile boundary, the look-ahead behind the epilogue's stores, the
    patch stage that switches at every tile (Cin = 32), both column tiles walking the same pixel tiles (256 columns)."""
    n, grid, lo, hi = Hh.later_shape(0, n_cu(), t, Co)
    plan = assert_plan(0, n, C, 48, 48, Co)
    assert plan[3:5] == (3, 3) and plan[5:] == (grid, lo, hi) and hi == t and (grid // plan[2]) % 9
    WALKED.update((lo, hi))
    x, w, b = Hh.routed_conv_case(n, C, 48, 48, Co, 40 + t)
    equal(twice(run_conv, x, w, b, ACT_RELU), Hh.conv_ref(x, w, b, ACT_RELU), n, 48, 48, ("later", C, Co, n, lo, hi))


def test_conv3_halo_raw_refuses_what_the_kernel_does_not_take():
    L = _L()
    raw, _ = raw_buffer(16 * 16, 64)
    out = torch.empty(1, 64, 16, 16, device="cuda")
    for (C, Co) in ((48, 64), (64, 300)):
        x = torch.zeros(1, C, 16, 16, device="cuda")
        w, b = np.zeros((Co, C, 3, 3), np.float32), np.zeros(Co, np.float32)
        with pytest.raises(ValueError):
            L.check(L.load().ocrvi_test_conv3_halo_raw(0, x.data_ptr(), w.ctypes.data, b.ctypes.data, 1, C, 16, 16, Co, 0, raw.data_ptr(), out.data_ptr()))
