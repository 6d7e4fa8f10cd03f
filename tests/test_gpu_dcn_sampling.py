"""GPU: the modulated deformable 3x3 convolution in all four element types on the default dispatch -- dcn_pipe_kernel (csrc/dcn_pipe.h) for
bf16, f16 and f16x2, conv_gemm.h's AM_DCN mode for fp32 (both of its row tiles where the layer has 256-column tiles) -- through
ocrvi_test_deform_conv_raw, every element held to the float64 reference of tests/dcn_refs.py: EQUAL to it on probe data, within dcn_bound
(derivation there) on value data.  tests/test_dcn_refs_cpu.py shows on the CPU that an fp32 emulation of the kernels equals the reference
and stays inside the bound on exactly these cases and that sixteen wrong kernels are each caught by one of them.  Every case first asserts
its plan (kernel, row and column tile, patch shape, tiles, grid, K-steps) through ocrvi_test_dcn_plan with the device's CU count, then
runs twice into a NaN-filled NHWC output of the element type with 128 guard rows of a NaN payload behind it: the two runs must be
bit-identical, every element written, the guard rows untouched.  No element is excluded from any comparison.

  probe         one weight of 1 per output channel, every (tap, channel block) probed; x encodes row, column, image and channel; offsets
                constructed so that in every tap both axes reach -1, -3/4, -1/4, 0, an interior integer, that + 3/4, L - 1, L - 3/4,
                L - 1/4, L and L + 5, in all pairs; masks 1 and 1/2: output == reference
  value         Gaussian x and w, offsets N(0, 3) on the 2^-10 grid, masks on the 2^-8 grid; every third map sends all samples into the
                one-pixel bands around the four border lines: err <= bound on every element
  maps          33x3, 9x17, 10x13, 3x65, 2x130, 1x129 (patches of 4, 8, 16, 32, 64 and 128 columns, all ragged) and 13x19 at stride 2; 2 or 3
                images; C_in with an odd and an even number of K-steps; C_out 72, 128, 320 (128-column build: N tail, exact, three tiles)
                and 200, 256, 512 (256-column build: N tail, exact, two tiles); the 10x13 map goes through the residual build
  wild, mask 0  +-1e9, +-3e38, +-inf and NaN offsets on every seventh (pixel, tap) contribute exactly 0; mask 0 on taps 1, 4, 8 gives the bias
  persistent    31x127, C_in 64, C_out 640: 310 tiles, more than the device has CUs, so workgroups walk two tiles (dcn_pipe)
  independence  x changed at one pixel of image 1: images 0 and 2 keep their bits; the offsets of one output pixel changed: every other
                pixel does

Largest err / bound per family and type, measured on the MI355X (256 CUs)
(71 tests, 7 s for the file; the slowest test 1.2 s, the persistent map, whose float64 reference has 7874 rows):
                f32      f16x2    bf16     f16
  value         0.013    0.015    1.000    0.996
  persistent    -        0.009    0.999    0.995
(probe, wild, mask 0 and independence are equalities.  The CPU emulation gives the same figures to three digits: 0.013 / 0.015 / 1.000 /
0.996 with the persistent map included.  The 16-bit figures near 1 are elements whose whole error is the last rounding to T next to a tie;
the fp32 and f16x2 figures are small because gemm_bound charges a 4-byte sum of K = 576 .. 864 products its worst case, K u S.  Found:
nothing wrong in either kernel or in the launchers.  The paths that ran here for the first time -- an odd number of K-steps (the single
step() of the last pair in waves 0-3, the drain of waves 4-7), patches of 4, 32, 64 and 128 columns, C_out != C_in in both column builds
with their clamped bias and residual reads, the persistent loop's second tile -- give bit-identical results on repeated runs and equal
the reference on the probe data.  The patch / grid choice of launch_dcn_pipe and the row-tile choice of launch_mode<AM_DCN> moved into
dcn_pipe_plan and dcn_gemm_tile_m for the plan hook: ocrvi_test_deform_conv gives the same bits before and after on all 62 probe and
value launches of this file.  profiles/r18_dcn_sampling.md has the CPU tables.)
"""
import os
import time

import numpy as np
import pytest
import torch

import dcn_refs as D
from test_gpu_kernels import DT

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

GUARD = 128                      # rows behind the output
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
WORST = {}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_plan(dt, case):
    name, N, C, H, W, Co, stride, _ = case
    plan = D.plan_of(_L().load(), dt, N, C, H, W, Co, stride, _n_cu())
    assert plan == D.expect_plan(dt, N, C, H, W, Co, stride, _n_cu()), (dt, case, plan)
    assert plan[0] == (1 if dt in D.PIPE else 0), (dt, plan)
    if name in D.MAP_LW and dt in D.PIPE:
        assert plan[3] == D.MAP_LW[name], (name, plan)
    return plan


def run_dcn(x, off, mask, w, b, res, stride, dt):
    """One launch: out [N Ho Wo, Co] float32 on the CPU.  Guards and unwritten elements are checked here."""
    L = _L()
    N, C, H, W = x.shape
    Co = w.shape[0]
    Ho, Wo = off.shape[-2:]
    M = N * Ho * Wo
    esz = 4 if dt in ("f32", "f16x2") else 2
    raw = torch.full(((M + GUARD) * Co * esz,), 0xFF, dtype=torch.uint8, device="cuda")        # every element a NaN
    guard = raw[M * Co * esz:].view(torch.int32)
    guard.fill_(X_GUARD)
    out = torch.full((N, Co, Ho, Wo), float("nan"), device="cuda")
    xd, od, md = x.cuda().contiguous(), off.cuda().contiguous(), mask.cuda().contiguous()
    rd = None if res is None else res.cuda().contiguous()
    wh, bh = np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32)
    L.check(L.load().ocrvi_test_deform_conv_raw(0, DT[dt], xd.data_ptr(), od.data_ptr(), md.data_ptr(), wh.ctypes.data, bh.ctypes.data,
                                                None if rd is None else rd.data_ptr(), N, C, H, W, Co, stride, 1, raw.data_ptr(), out.data_ptr()))
    torch.cuda.synchronize()
    assert bool((guard == X_GUARD).all()), "the guard rows behind the output changed"
    bad = (~torch.isfinite(out)).nonzero()
    assert bad.numel() == 0, ("elements of the output were not written (or are not finite)", int(bad.shape[0]), bad[:8].tolist())
    return out.permute(0, 2, 3, 1).reshape(M, Co).cpu()


def run_twice(x, off, mask, w, b, res, stride, dt):
    out = run_dcn(x, off, mask, w, b, res, stride, dt)
    assert torch.equal(out, run_dcn(x, off, mask, w, b, res, stride, dt)), "two runs differ"
    return out


def run_case(dt, case, inp):
    """The launches of one case on the default dispatch: one, or -- fp32 with 256-column tiles -- conv_gemm's 32- and 64-row tiles through the
    launcher's per-launch OCRVI_DCN_TILE_M, which only regroup pixels: same sums in the same order."""
    plan = _assert_plan(dt, case)
    if dt in D.PIPE or plan[2] != 256:
        return [run_twice(*inp, case[6], dt)]
    outs = []
    for tm in ("32", "64"):
        os.environ["OCRVI_DCN_TILE_M"] = tm
        try:
            outs.append(run_twice(*inp, case[6], dt))
        finally:
            os.environ.pop("OCRVI_DCN_TILE_M", None)
    assert torch.equal(outs[0], outs[1]), "the 32- and the 64-row tile differ"
    return outs


def _hold(out, ref, bound, family, dt, tag):
    q = D.err_ratio(out, ref, bound)
    worst = float(q.max())
    print(f"\n[dcn {family} {dt} {tag}] max err / bound {worst:.3f}")
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), worst)
    bad = (q > 1.0).nonzero()
    assert bad.numel() == 0, (family, dt, tag, worst, bad[:8].tolist())


def _equal(out, ref, dt, case, Wo):
    bad = (out.double() != ref).nonzero()
    if bad.numel():
        C = case[2]
        where = []
        for m, n in bad[:8].tolist():
            tap, ch = D.probe_where(n, C, dt)
            where.append(f"pixel {m} (image {m // (Wo * (ref.shape[0] // case[1] // Wo))}, ow {m % Wo}) channel {n} = tap {tap} of input channel {ch}: "
                         f"{float(out[m, n])} for {float(ref[m, n])}")
        raise AssertionError((dt, case, int(bad.shape[0]), where))


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[dcn summary] {time.time() - t0:.0f} s; largest err / bound per family and type")
    for fam in ("value", "persistent"):
        print(f"[dcn summary] {fam:10s} " + "   ".join(f"{dt} {WORST.get((fam, dt), float('nan')):.3f}" for dt in D.DTS))


PARAMS = [(dt, i) for dt in D.DTS for i in range(len(D.MAPS))]
IDS = [f"{dt}-{D.MAPS[i][0]}" for dt, i in PARAMS]


@pytest.mark.parametrize("dt,i", PARAMS, ids=IDS)
def test_dcn_probe(dt, i):
    case = D.cases(dt)[i]
    ref, _ = D.ref_and_bound("probe", dt, case)
    for out in run_case(dt, case, D.inputs("probe", dt, case)):
        _equal(out, ref, dt, case, D.out_hw(case[3], case[4], case[6])[1])


@pytest.mark.parametrize("dt,i", PARAMS, ids=IDS)
def test_dcn_value(dt, i):
    case = D.cases(dt)[i]
    ref, bound = D.ref_and_bound("value", dt, case)
    for out in run_case(dt, case, D.inputs("value", dt, case)):
        _hold(out, ref, bound, "value", dt, f"{case[0]} C {case[2]} Co {case[5]}")


@pytest.mark.parametrize("kind", ("wild", "mask0"))
@pytest.mark.parametrize("dt", D.DTS)
def test_dcn_probe_degenerate(dt, kind):
    """Documented behaviour (dcn_pipe.h and conv_gemm.h clamp a position before the float-to-int conversion and the corner indices into the
    image after it, so no address outside x is formed): a wild or non-finite offset contributes exactly 0, and so does mask 0."""
    case = D.small_case(dt)
    ref, _ = D.ref_and_bound("probe", dt, case, kind)
    for out in run_case(dt, case, D.inputs("probe", dt, case, kind)):
        _equal(out, ref, dt, case, case[4])


@pytest.mark.parametrize("dt", D.PIPE)
def test_dcn_persistent_loop(dt):
    case = D.persist_case(dt)
    plan = _assert_plan(dt, case)
    assert plan[4] > _n_cu() and plan[6] >= 2, plan               # workgroups walk more than one tile
    ref, _ = D.ref_and_bound("probe", dt, case)
    _equal(run_twice(*D.inputs("probe", dt, case), case[6], dt), ref, dt, case, case[4])
    ref, bound = D.ref_and_bound("value", dt, case)
    _hold(run_twice(*D.inputs("value", dt, case), case[6], dt), ref, bound, "persistent", dt, f"{case[0]} tiles {plan[4]} grid {plan[5]}")


@pytest.mark.parametrize("dt", D.DTS)
def test_dcn_independence(dt):
    case = D.small_case(dt)
    name, N, C, H, W, Co, stride, _ = case
    x, off, mask, w, b, res = D.inputs("value", dt, case)
    out = run_twice(x, off, mask, w, b, res, stride, dt).reshape(N, H * W, Co)
    x2 = x.clone()
    x2[1, :, 4, 8] = D.round_to(x[1, :, 4, 8] * 1.5 + 0.25, dt)
    out2 = run_dcn(x2, off, mask, w, b, res, stride, dt).reshape(N, H * W, Co)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[2], out2[2]) and not torch.equal(out[1], out2[1])
    off2 = off.clone()
    off2[1, :, 4, 8] = -off[1, :, 4, 8]
    out3 = run_dcn(x, off2, mask, w, b, res, stride, dt).reshape(N * H * W, Co)
    keep = torch.arange(N * H * W) != (1 * H + 4) * W + 8
    flat = out.reshape(N * H * W, Co)
    assert torch.equal(flat[keep], out3[keep]) and not torch.equal(flat[~keep], out3[~keep])
