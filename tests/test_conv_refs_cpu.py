"""CPU: tests/conv_refs.py separates right from wrong.  (1) conv_ref is torch's own conv2d / relu / gelu in float64, grouped and strided.
(2) An fp32 + T emulation of gconv32 and of conv_gemm's 3x3 mode stays within conv_bound on every case tests/test_gpu_grouped_conv.py
runs and equals the reference on the routed integer cases: the inputs are admissible.  (3) Eleven wrong kernels, applied to that
emulation, break the routed equality or leave the bound on a named case of the family meant for them; the (kernel, type) pairs that cannot
be told apart are asserted to stay inside, by name.  (4) routed_case meets its own conditions.  (5) Through ocrvi_test_gconv_plan (host
only) every launch takes the kernel and the tiling the GPU file names on devices of 256, 304 and 64 compute units.  (6) The halo-index
multiplication of gconv32 is exact where the kernel uses it, and not up to 2^11.  Ratios are printed (pytest -s);
profiles/r19_grouped_conv.md has the tables."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_refs as R

N_CU = 256                       # the device the bound test builds the later-tiles shapes for
WORST = {}
GROUPED = lambda C: C // 32


def _q(got, ref, bound):
    return float(R.err_ratio(got, ref, bound).max())


def _note(family, dt, q):
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), q)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for fam in ("value", "in place", "later", "strided", "indep"):
        print(f"\n[conv emulation] {fam:8s} " + "   ".join(f"{dt} {WORST.get((fam, dt), float('nan')):.3f}" for dt in R.DTS))


def test_reference_is_torch_in_float64():
    g = torch.Generator().manual_seed(1)
    for (n, C, H, W, Co, stride, groups) in ((2, 8, 5, 7, 12, (1, 1), 4), (1, 6, 9, 4, 6, (2, 1), 1), (3, 4, 6, 11, 8, (2, 2), 2), (1, 64, 1, 5, 64, (1, 1), 2)):
        Ho, Wo = R.out_hw(H, W, stride)
        x, w, b, res = (torch.randn(s, generator=g) for s in ((n, C, H, W), (Co, C // groups, 3, 3), (Co,), (n, Co, Ho, Wo)))
        conv = F.conv2d(x.double(), w.double(), b.double(), stride, 1, 1, groups)
        assert conv.shape == (n, Co, Ho, Wo)
        rows = R.rows_of
        close = lambda got, want: float((got - rows(want)).abs().max()) < 1e-12
        assert close(R.conv_ref(x, w, b, None, stride, groups, R.ACT_NONE, 0), conv)
        assert close(R.conv_ref(x, w, b, res, stride, groups, R.ACT_RELU, 0), F.relu(conv + res.double()))
        assert close(R.conv_ref(x, w, b, res, stride, groups, R.ACT_RELU, 1), F.relu(conv) + res.double())
        assert close(R.conv_ref(x, w, b, res, stride, groups, R.ACT_GELU, 1), F.gelu(conv) + res.double())
        assert close(R.conv_ref(x, w, b, res, stride, groups, R.ACT_GELU, 0), F.gelu(conv + res.double()))


def test_routed_case_meets_its_conditions():
    shapes = [(n, C, H, W, C, (1, 1), GROUPED(C)) for (n, C, H, W), _ in R.ROUTE_SHAPES] + [(*s[:6], 1) for s in R.STRIDED]
    for (n, C, H, W, Co, stride, groups) in shapes:
        x, w, b, res = R.routed_case(n, C, H, W, Co, stride, groups, 13)
        Cg, Ng = C // groups, Co // groups
        assert float(x.abs().max()) <= 7 and float(b.abs().max()) <= 8 and float(res.abs().max()) <= 32
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        wk = w.permute(0, 2, 3, 1).reshape(Co, 9 * Cg)
        cnt = (wk != 0).sum(1)
        assert int(cnt.min()) >= 9 and int(cnt.max()) <= 12
        assert bool((w != 0).sum(1).ge(1).all()), "a channel without a weight at some tap"
        for g in range(groups):                                         # inside every group every (tap, channel) position is used
            assert bool((wk[g * Ng:(g + 1) * Ng] != 0).any(0).all()), g
        assert len({tuple(r) for r in wk.int().tolist()}) == Co        # no two channels of the layer share a weight row
        for act in (R.ACT_NONE, R.ACT_RELU):
            for rp in (0, 1):
                y = R.conv_ref(x, w, b, res, stride, groups, act, rp)
                assert float(y.abs().max()) <= 124 and torch.equal(y, y.round())
        S = torch.cat([a.abs() @ wg.abs().t() for a, wg in R.group_gemms(x, w, groups, stride)], 1)
        assert float((S + b.abs() + R.rows_of(res).abs()).max()) <= 124


def _routing(dt):
    """(tag, args of routed_case, out_f32, res_post or None, act, gconv32_on) of every routed launch of the GPU file."""
    out = []
    for i, ((n, C, H, W), _) in enumerate(R.ROUTE_SHAPES):
        for (of, rp, act) in R.ROUTE_VARIANTS:
            out.append((f"{n}x{H}x{W} C{C} {(of, rp, act)}", (n, C, H, W, C, (1, 1), GROUPED(C), 11 + i), of, rp, act, True))
            if dt in ("bf16", "f16"):
                out.append((f"fallback {n}x{H}x{W} C{C} {(of, rp, act)}", (n, C, H, W, C, (1, 1), GROUPED(C), 11 + i), of, rp, act, False))
    for i, (n, C, H, W, Co, stride, (of, _)) in enumerate(R.STRIDED):
        for o in (of, 0):
            for act in (R.ACT_NONE, R.ACT_RELU):
                out.append((f"strided {n}x{H}x{W} {C}->{Co} {(o, act)}", (n, C, H, W, Co, stride, 1, 31 + i), o, None, act, True))
    return out


@pytest.mark.parametrize("dt", R.DTS)
def test_emulation_equals_the_reference_on_routed_cases(dt):
    for tag, args, of, rp, act, on in _routing(dt):
        x, w, b, res = R.routed_case(*args, with_res=rp is not None)
        stride, groups = args[5], args[6]
        ref = R.conv_ref(x, w, b, res, stride, groups, act, rp or 0)
        assert torch.equal(R.emulate(x, w, b, res, stride, groups, act, rp or 0, dt, of, gconv32_on=on).double(), ref), (dt, tag)


def _held(fam, dt, tag, x, w, b, res, stride, groups, act, rp, of):
    ref = R.conv_ref(x, w, b, res, stride, groups, act, rp or 0)
    bound = R.conv_bound(x, w, b, res, stride, groups, act, rp or 0, dt, of)
    q = _q(R.emulate(x, w, b, res, stride, groups, act, rp or 0, dt, of), ref, bound)
    print(f"\n[conv emulation {fam} {dt} {tag}] max err / bound {q:.3f}")
    _note(fam, dt, q)
    assert q <= 1.0, (fam, dt, tag, q)


@pytest.mark.parametrize("dt", R.DTS)
def test_emulation_stays_within_the_bound(dt):
    """The admissibility condition: err / bound <= 1 for the fp32 emulation on the value, in-place, later-tiles, independence and strided cases."""
    for (n, C, H, W) in R.VALUE_SHAPES:
        for (of, rp, act) in R.VALUE_VARIANTS:
            x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPED(C), dt, of, 5)
            _held("value", dt, f"{n}x{H}x{W} {(of, rp, act)}", x, w, b, res if rp is not None else None, (1, 1), GROUPED(C), act, rp, of)
    n, C, H, W = R.IN_PLACE_SHAPE
    x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPED(C), dt, 1, 6)
    _held("in place", dt, "", x, w, b, res, (1, 1), GROUPED(C), R.ACT_GELU, 1, 1)
    n, C, H, W = R.INDEP_SHAPE
    for of in (0, 1):
        x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPED(C), dt, of, 7)
        _held("indep", dt, f"out_f32 {of}", x, w, b, res if of else None, (1, 1), GROUPED(C), R.ACT_GELU, 1, of)
    _, C, H, W, *_ = R.later_shape(N_CU, 4)
    for of in (0, 1):
        x, w, b, res = R.value_case(1, C, H, W, C, (1, 1), GROUPED(C), dt, of, 21)
        _held("later", dt, f"out_f32 {of}", x, w, b, res if of else None, (1, 1), GROUPED(C), R.ACT_GELU, 1, of)
    for (n, C, H, W, Co, stride, (of, act)) in R.STRIDED:
        x, w, b, _ = R.value_case(n, C, H, W, Co, stride, 1, dt, of, 9)
        _held("strided", dt, f"{n}x{H}x{W} {C}->{Co}", x, w, b, None, stride, 1, act, None, of)


# Which case of which family catches which wrong kernel: (family, shape n C H W, (out_f32, res_post, act), gconv32 on).
R6, R7, R5 = (2, 128, 6, 80), (1, 128, 7, 100), (1, 128, 5, 81)
CATCH = {
    "taps (r, s) exchanged": ("routing", R7, (0, None, R.ACT_NONE), True),
    "last tap dropped": ("routing", R7, (0, None, R.ACT_NONE), True),
    "x of the next group": ("routing", R7, (1, None, R.ACT_RELU), True),
    "output-channel permutation left out": ("routing", R7, (0, None, R.ACT_NONE), True),
    "bias of the next 4-channel block": ("routing", R7, (1, None, R.ACT_RELU), True),
    "res_post flipped": ("routing", R7, (1, 1, R.ACT_RELU), True),
    "halo clamped, not zeroed": ("routing", R6, (0, None, R.ACT_NONE), True),
    "halo row of the neighbouring image": ("routing", R6, (1, 1, R.ACT_RELU), True),
    "ragged band written from the wrong pixel": ("routing", R5, (0, None, R.ACT_NONE), True),
    "tenth tap not masked": ("routing", R7, (0, None, R.ACT_NONE), False),
    "next tile's halo not staged": ("later", None, (1, 1, R.ACT_GELU), True),
}
# (kernel, type) pairs that no output can tell from a right kernel; the test asserts that they stay INSIDE, so each exemption is a checked
# statement:
#   the channel permutation, the ragged bands and the staged next tile are gconv32's: in the 4-byte types these calls run on conv_gemm, which
#   has none of them;
#   the tenth tap exists only in conv_gemm's 64-element K-step (the 16-bit types with OCRVI_GCONV32=0: 288 = 4.5 steps).  There the packer
#   fills weight columns 288..319 with zeros, so whatever finite values an unmasked tap reads -- all its addresses are inside the image,
#   the row and column tests stay -- are multiplied by zero: the mask saves the loads, no output depends on it.
NOT_SEPARABLE = {(m, dt) for m in ("output-channel permutation left out", "ragged band written from the wrong pixel", "next tile's halo not staged")
                 for dt in ("f32", "f16x2")}
NOT_SEPARABLE |= {("tenth tap not masked", dt) for dt in R.DTS}


@pytest.mark.parametrize("dt", R.DTS)
def test_wrong_kernels_are_caught(dt):
    assert set(CATCH) == set(R.MUTANTS)
    for name in R.MUTANTS:
        fam, shape, (of, rp, act), on = CATCH[name]
        if fam == "routing":
            n, C, H, W = shape
            idx = [s for s, _ in R.ROUTE_SHAPES].index(shape)
            x, w, b, res = R.routed_case(n, C, H, W, C, (1, 1), GROUPED(C), 11 + idx, with_res=rp is not None)
            n_cu = N_CU
        else:                                         # identical images on a launch whose workgroups walk three and four tiles
            n, C, H, W, _, lo, hi = R.later_shape(N_CU, 4)
            assert (lo, hi) == (3, 4)
            x1, w, b, r1 = R.value_case(1, C, H, W, C, (1, 1), GROUPED(C), dt, of, 21)
            x, res = x1.expand(n, -1, -1, -1), r1.expand(n, -1, -1, -1)
            n_cu = N_CU
        groups = GROUPED(C)
        ref = R.conv_ref(x, w, b, res, (1, 1), groups, act, rp or 0)
        good = R.emulate(x, w, b, res, (1, 1), groups, act, rp or 0, dt, of, None, n_cu, on)
        bad = R.emulate(x, w, b, res, (1, 1), groups, act, rp or 0, dt, of, name, n_cu, on)
        if fam == "routing":
            assert torch.equal(good.double(), ref)
            wrong = int((bad.double() != ref).sum())
            print(f"\n[conv mutant {dt}] {name:42s} routing {shape} {(of, rp, act)}: {wrong} elements differ")
            caught = wrong > 0
        else:
            bound = R.conv_bound(x, w, b, res, (1, 1), groups, act, rp or 0, dt, of)
            assert _q(good, ref, bound) <= 1.0
            q = _q(bad, ref, bound)
            M1 = H * W
            moved = not torch.equal(bad.reshape(n, M1, C), bad[:M1].expand(n, -1, -1))
            print(f"\n[conv mutant {dt}] {name:42s} later {n} x {H}x{W}: max err / bound {q:.3g}, later images differ from image 0: {moved}")
            caught = q > 1.0 and moved
        assert caught != ((name, dt) in NOT_SEPARABLE), (name, dt)


def test_res_post_is_seen_under_the_gelu():
    """The residual-after-GELU order of LocalMixing's second convolution: flipping it leaves the bound of the value family."""
    n, C, H, W = R.VALUE_SHAPES[0]
    for dt in R.DTS:
        x, w, b, res = R.value_case(n, C, H, W, C, (1, 1), GROUPED(C), dt, 1, 5)
        ref = R.conv_ref(x, w, b, res, (1, 1), GROUPED(C), R.ACT_GELU, 1)
        bound = R.conv_bound(x, w, b, res, (1, 1), GROUPED(C), R.ACT_GELU, 1, dt, 1)
        assert _q(R.emulate(x, w, b, res, (1, 1), GROUPED(C), R.ACT_GELU, 1, dt, 1, "res_post flipped"), ref, bound) > 1.0


def _lib():
    from ocr_vi_invoice_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("n_cu", (256, 304, 64))
def test_every_launch_takes_the_kernel_it_names(n_cu):
    lib = _lib()
    for dt in R.DTS:
        for (n, C, H, W, Co, stride, groups, of, has_res) in R.launches(dt):
            plan = R.plan_of(lib, dt, n, C, H, W, Co, stride, groups, of, has_res, n_cu)
            assert plan == R.expect_plan(dt, n, C, H, W, Co, stride, groups, of, has_res, n_cu), (dt, n, C, H, W, Co, stride, of, has_res, plan)
        for (n, C, H, W), tiling in R.ROUTE_SHAPES:                       # the tilings the table names, whatever the device
            for (of, rp, act) in R.ROUTE_VARIANTS:
                plan = R.plan_of(lib, dt, n, C, H, W, C, (1, 1), GROUPED(C), of, rp is not None, n_cu)
                gc = dt in ("bf16", "f16") and (rp is None or of)
                assert plan[0] == (1 if gc else 0)
                assert plan[1:7] == ((0, 0, *tiling) if gc else (128, 32, 0, 0, 0, 0)), (dt, n, C, H, W, plan)
                assert plan[10:] == (GROUPED(C), 5 if dt in ("bf16", "f16") else 9)
        for (n, C, H, W, Co, stride, _) in R.STRIDED:
            assert R.plan_of(lib, dt, n, C, H, W, Co, stride, 1, 1, False, n_cu)[:3] == (0, 128, 128)
        if dt in ("bf16", "f16"):
            walked = set()
            for t in (2, 4):
                n, C, H, W, grid, lo, hi = R.later_shape(n_cu, t)
                for of in (0, 1):
                    plan = R.plan_of(lib, dt, n, C, H, W, C, (1, 1), GROUPED(C), of, bool(of), n_cu)
                    assert plan[:10] == (1, 0, 0, 3, 1, 3, 1, grid, lo, hi) and hi == lo + 1 and grid % 3, (dt, t, plan)
                walked |= {lo, hi}
            assert walked == {1, 2, 3, 4}, walked


def test_halo_index_multiplication():
    """gconv32 splits a halo pixel index by pix / HW == (pix * (65536 // HW + 1)) >> 16.  It needs that for pix < (GC_TH + 2) * HW at the
    halo widths HW = 16 nbx + 2, nbx = 1..GC_NBX; it does not hold up to 2^11 (the header's static_assert states the requirement)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ocr_vi_invoice_amd", "csrc", "gconv32.h")).read()
    assert (int(re.search(r"constexpr int GC_TH = (\d+);", src).group(1)), int(re.search(r"constexpr int GC_NBX = (\d+);", src).group(1))) == (R.GC_TH, R.GC_NBX)
    assert "static_assert(gc_hw_magic_exact()" in src
    for nbx in range(1, R.GC_NBX + 1):
        hw = 16 * nbx + 2
        first = R.magic_first_failure(hw)
        assert first is None or first >= (R.GC_TH + 2) * hw, (hw, first)
    assert [16 * nbx + 2 for nbx in range(1, R.GC_NBX + 1)] == [18, 34, 50, 66, 82]
    assert R.magic_first_failure(82) == 1065 and (R.GC_TH + 2) * 82 == 492
