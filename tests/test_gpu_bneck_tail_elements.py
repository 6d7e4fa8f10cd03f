"""GPU: bneck_tail_kernel (csrc/bneck_tail.h: the f16x2 detector's fused layer1 chain conv2 3x3 + ReLU -> conv3 1x1 + identity + ReLU = y
-> next conv1 1x1 + ReLU = t1'), full and y-only form, through ocrvi_test_bneck_tail_raw, every element of y and t1' held to the float64
chain of tests/halo_refs.py: equal to it on routed and probe data, within bneck_bound (three chained gemm_refs.gemm_bound, each stage's
bound the next one's a_err) on value data.  tests/test_halo_refs_cpu.py shows on the CPU that an fp32 emulation of the kernel does the same
on these cases and that wrong kernels do not.  Every case first asserts the tiling through ocrvi_test_halo_plan with the device's CU count,
then runs twice into NaN-filled y and t1' buffers with 128 guard rows of a NaN payload behind each: bit-identical runs, every element
finite, guards untouched.  No element is excluded; a failure names (image, y, x, channel, got, want).

  routed        routed_bneck_case: integers all the way (t2 <= 92, y <= 408, t1' <= 2456: exact in fp32 and f16x2), every k of every unit of
                the tail used: y == reference, t1' == reference (and with them t2)
  probes a, b   halo_refs' impulse and one-hot-weight probes on conv2 (bneck_tail's own copy of conv3_halo's unit loop), the tail passing
                t2 through as in probe c; the two forms alternate by launch
  probe c       pass-through: conv2 the centre-tap identity, conv3 copies t2 into y[0..127] and leaves y[128..] to the identity, conv1 selects
                64 channels of y per launch (four launches read all 256): y and t1' equal the selected full-width inputs bit for bit -- the
                accumulator-lane hand-off A -> B -> C and the identity's group schedule
  rounding      t2 = 512.25 + m 2^-14, which the pack must round before conv3 takes differences of it: == the chain with t2 rounded to f16x2
  value         conv_refs.value_case rows for t1, Gaussian weights with equal halves, biases sweeping [-12, 12], identity >= 0: err <= bound
  independence  one t1 element: only its 3x3 reach of y and t1' changes bits; one identity element: only that (pixel, channel) of y and that
                pixel of t1'; one conv3 channel's weights and bias: only that channel of y; one conv1 channel's: only that channel of t1'
  later tiles   routed, DISTINCT 48x48 images making the workgroups walk 1 and 2, then 3 tiles, on a grid no multiple of 9, both forms
Shapes: halo_refs.BNECK_SHAPES, both forms.

Measured on the MI355X (256 CUs): 66 tests, 6.2 s for the file, the slowest test 0.78 s (later tiles, 58 images).  Largest err / bound of
the value family: y 0.0012, t1' 0.0001 (the CPU emulation: 0.001 and 0.000: the chained bound carries the stage before through |W|);
every other family is an equality and holds.  The later-tiles launches walked 1, 2 and 3 tiles per workgroup.  Nothing was found wrong
in the kernel, the packer or the launcher.  profiles/r27_halo_elements.md has the CPU tables and the mutant-by-family matrix.
"""
import time

import pytest
import torch

import halo_refs as Hh
from test_gpu_conv3_halo_elements import X_GUARD, _L, assert_plan, bits, check_written, equal, h, hold, n_cu, raw_buffer, twice

pytestmark = pytest.mark.gpu

WORST = {}
WALKED = set()


def run_bneck(t1, idn, wb, y_only=False):
    """One launch: (y rows [n H W, 256], t1' rows [n H W, 64] or None), float32 on the GPU."""
    L = _L()
    n, _, H, W = t1.shape
    hw = [h(t) for t in wb]
    td, idd = t1.cuda().contiguous(), idn.cuda().contiguous()
    yraw, yg = raw_buffer(n * H * W, 256)
    traw, tg = raw_buffer(n * H * W, 64)
    y = torch.full((n, 256, H, W), float("nan"), device="cuda")
    tn = torch.full((n, 64, H, W), float("nan"), device="cuda")
    L.check(L.load().ocrvi_test_bneck_tail_raw(0, td.data_ptr(), idd.data_ptr(), *[a.ctypes.data for a in hw], n, H, W, 1 if y_only else 0,
                                               yraw.data_ptr(), traw.data_ptr(), y.data_ptr(), tn.data_ptr()))
    check_written(yg, y, "bneck_tail y")
    if y_only:
        torch.cuda.synchronize()
        assert bool((traw[:n * H * W * 256].view(torch.int32) == -1).all()) and bool((tg == X_GUARD).all()), "the y-only form wrote t1'"
        return Hh.rows_of(y).contiguous(), None
    check_written(tg, tn, "bneck_tail t1'")
    return Hh.rows_of(y).contiguous(), Hh.rows_of(tn).contiguous()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[bneck_tail summary] {time.time() - t0:.1f} s; largest err / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
    print(f"[bneck_tail summary] tiles per workgroup walked in the later-tiles family: {sorted(WALKED)}")


IDS = [f"{n}x{H}x{W}" for (n, H, W) in Hh.BNECK_SHAPES]
FORMS = pytest.mark.parametrize("y_only", (False, True), ids=("full", "y-only"))


def _both(out, ref, n, H, W, tag):
    (y, tn), (_, ry, rt) = out, ref
    equal(y, ry, n, H, W, (*tag, "y"))
    if tn is not None:
        equal(tn, rt, n, H, W, (*tag, "t1'"))


@FORMS
@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_routed(i, y_only):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    t1, idn, wb = Hh.routed_bneck_case(n, H, W, 3 + i)
    _both(twice(run_bneck, t1, idn, wb, y_only), Hh.bneck_ref(t1, idn, wb), n, H, W, ("routed", IDS[i], y_only))


@FORMS
@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_pass_through(i, y_only):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    for l in range(1 if y_only else 4):
        t1, idn, wb = Hh.probe_c_bneck_case(n, H, W, l, 7 + i)
        ref = Hh.bneck_ref(t1, idn, wb)
        assert torch.equal(ref[1][:, :64], Hh.rows_of(t1).double()) and torch.equal(ref[1][:, 128:], Hh.rows_of(idn)[:, 128:].double())
        _both(twice(run_bneck, t1, idn, wb, y_only), ref, n, H, W, ("probe c", IDS[i], y_only, l))


@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_probe_impulses(i):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    for l in range(max(4, Hh.probe_a_launches(n, 64, H, W))):
        t1, idn, wb = Hh.probe_a_bneck_case(n, H, W, l, 11 + i)
        _both(twice(run_bneck, t1, idn, wb, l % 2 == 1), Hh.bneck_ref(t1, idn, wb), n, H, W, ("probe a", IDS[i], l))


@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_probe_one_hot_weights(i):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    for l in range(Hh.probe_b_launches(576, 64)):
        t1, idn, wb = Hh.probe_b_bneck_case(n, H, W, l, 13 + i)
        _both(twice(run_bneck, t1, idn, wb, l % 2 == 1), Hh.bneck_ref(t1, idn, wb), n, H, W, ("probe b", IDS[i], l))


@FORMS
@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_rounds_t2(i, y_only):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    t1, idn, wb = Hh.rounding_bneck_case(n, H, W)
    _both(twice(run_bneck, t1, idn, wb, y_only), Hh.bneck_ref(t1, idn, wb, round_t2=True), n, H, W, ("rounding", IDS[i], y_only))


@FORMS
@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)), ids=IDS)
def test_bneck_tail_value(i, y_only):
    n, H, W = Hh.BNECK_SHAPES[i]
    assert_plan(1, n, 64, H, W, 256)
    t1, idn, wb = Hh.value_bneck_case(n, H, W, 5 + i)
    (_, ry, rt), (_, by, bt) = Hh.bneck_ref(t1, idn, wb), Hh.bneck_bound(t1, idn, wb)
    y, tn = twice(run_bneck, t1, idn, wb, y_only)
    hold(y, ry, by, n, H, W, "value y", f"{IDS[i]} y_only {y_only}", WORST)
    if tn is not None:
        hold(tn, rt, bt, n, H, W, "value t1'", IDS[i], WORST)


@FORMS
def test_bneck_tail_independence(y_only):
    n, H, W = 3, 17, 23
    assert_plan(1, n, 64, H, W, 256)
    t1, idn, wb = Hh.value_bneck_case(n, H, W, 21)
    w2, b2, w3, b3, w1, b1 = wb
    shape = lambda o, c: None if o is None else bits(o).reshape(n, H, W, c)
    run = lambda *a: tuple(shape(o, c) for o, c in zip(run_bneck(*a, y_only), (256, 64)))
    y, tn = (shape(o, c) for o, c in zip(twice(run_bneck, t1, idn, wb, y_only), (256, 64)))
    i0, c0, y0, x0 = 2, 41, 15, 16                                      # across both tile boundaries of the last image
    # ---- one element of t1
    t1b = t1.clone()
    t1b[i0, c0, y0, x0] = Hh.round_to(t1[i0, c0, y0, x0] * 1.5 + 0.25, Hh.DT)
    yb, tb = run(t1b, idn, wb)
    reach = torch.zeros(n, H, W, dtype=torch.bool, device="cuda")
    reach[i0, y0 - 1:y0 + 2, x0 - 1:x0 + 2] = True
    assert torch.equal(y[~reach], yb[~reach]) and not torch.equal(y[reach], yb[reach]), "y outside the t1 element's 3x3 reach changed"
    assert y_only or (torch.equal(tn[~reach], tb[~reach]) and not torch.equal(tn[reach], tb[reach]))
    # ---- one element of the identity (channel 200: group 6)
    idb = idn.clone()
    idb[i0, 200, y0, x0] = Hh.round_to(idn[i0, 200, y0, x0] * 1.5 + 30.0, Hh.DT)
    yb, tb = run(t1, idb, wb)
    one = torch.zeros(n, H, W, 256, dtype=torch.bool, device="cuda")
    one[i0, y0, x0, 200] = True
    assert torch.equal(y[~one], yb[~one]) and not torch.equal(y[one], yb[one]), "y beside the identity's element changed"
    pix = one.any(-1)
    assert y_only or (torch.equal(tn[~pix], tb[~pix]) and not torch.equal(tn[pix], tb[pix]))
    # ---- one channel of conv3, one of the next conv1 (not the layers' largest weights: the scales stay)
    ch3, ch1 = 77, 13
    assert float(w3[ch3].abs().max()) < float(w3.abs().max()) and float(w1[ch1].abs().max()) < float(w1.abs().max())
    w3b, b3b = w3.clone(), b3.clone()
    w3b[ch3] = Hh.round_to(w3[ch3] * 0.5, Hh.DT)
    b3b[ch3] = 3.0
    yb, tb = run(t1, idn, (w2, b2, w3b, b3b, w1, b1))
    keep = torch.arange(256, device="cuda") != ch3
    assert torch.equal(y[..., keep], yb[..., keep]) and not torch.equal(y[..., ch3], yb[..., ch3])
    if not y_only:
        w1b, b1b = w1.clone(), b1.clone()
        w1b[ch1] = Hh.round_to(w1[ch1] * 0.5, Hh.DT)
        b1b[ch1] = 3.0
        yb, tb = run(t1, idn, (w2, b2, w3, b3, w1b, b1b))
        keep = torch.arange(64, device="cuda") != ch1
        assert torch.equal(y, yb) and torch.equal(tn[..., keep], tb[..., keep]) and not torch.equal(tn[..., ch1], tb[..., ch1])


@FORMS
@pytest.mark.parametrize("t", (2, 3))
def test_bneck_tail_later_tiles(t, y_only):
    """A workgroup's second and third tiles: 34 (26) units per tile through the ring of eight, xoff rebuilt behind the tail, the identity
    prefetch and the t1' stores counted into the next tile's first waits."""
    n, grid, lo, hi = Hh.later_shape(1, n_cu(), t)
    plan = assert_plan(1, n, 64, 48, 48, 256)
    assert plan[3:5] == (3, 3) and plan[5:] == (grid, lo, hi) and hi == t and grid % 9
    WALKED.update((lo, hi))
    t1, idn, wb = Hh.routed_bneck_case(n, 48, 48, 50 + t)
    _both(twice(run_bneck, t1, idn, wb, y_only), Hh.bneck_ref(t1, idn, wb), n, 48, 48, ("later", n, lo, hi, y_only))
