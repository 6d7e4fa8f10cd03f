"""CPU: tests/gemm_refs.py separates right from wrong.  (1) gemm_ref is torch's own linear / relu / gelu in float64.  (2) An fp32 + T emulation
of the ring GEMM's order of operations stays within gemm_bound on every case tests/test_gpu_ring_gemm.py runs (and equals the reference on
the routed integer cases): the inputs are admissible.  (3) Fourteen wrong kernels, applied to that emulation, land outside the bound in the
family meant for them; the (kernel, type) pairs that cannot be told apart are asserted to stay inside, by name.  (4) routed_int_case meets
its own conditions.  (5) Through ocrvi_test_ring_plan (host only) every shape reaches the build and the tiles per workgroup it names on
devices of 256, 304 and 64 compute units.  Ratios are printed (pytest -s); profiles/r16_ring_gemm.md has the tables."""
import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R

N_CU = 256                       # the device the bound test builds its shapes for
WORST = {}


def _q(got, ref, bound):
    return float(R.err_ratio(got, ref, bound).max())


def _note(family, dt, q):
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), q)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for fam in ("value", "tail", "later"):
        print(f"\n[gemm emulation] {fam:6s} " + "   ".join(f"{dt} {WORST.get((fam, dt), float('nan')):.3f}" for dt in R.DTS))


def test_reference_is_torch_in_float64():
    g = torch.Generator().manual_seed(1)
    for M, K, N in ((5, 7, 3), (33, 96, 20), (130, 64, 129)):
        a, w, b, res = (torch.randn(s, generator=g) for s in ((M, K), (N, K), (N,), (M, N)))
        lin = F.linear(a.double(), w.double(), b.double())
        assert torch.equal(R.gemm_ref(a, w, b, None, R.ACT_NONE, 0), lin)
        assert torch.equal(R.gemm_ref(a, w, b, res, R.ACT_RELU, 0), F.relu(lin + res.double()))
        assert torch.equal(R.gemm_ref(a, w, b, res, R.ACT_RELU, 1), F.relu(lin) + res.double())
        # (F.gelu is x (1 + erf) / 2: it loses the tail's relative accuracy, not its absolute one)
        assert float((R.gemm_ref(a, w, b, res, R.ACT_GELU, 1) - (F.gelu(lin) + res.double())).abs().max()) < 1e-14
        assert float((R.gemm_ref(a, w, b, res, R.ACT_GELU, 0) - F.gelu(lin + res.double())).abs().max()) < 1e-14


@pytest.mark.parametrize("dt", R.DTS)
def test_emulation_equals_the_reference_on_routed_cases(dt):
    """The routed integers are exact in every type and in fp32 sums of any order: the routing cases, and one case per build."""
    cases = [(M, K, N, of, rp, act) for (M, K, N, of, rp, act) in R.routing_cases(dt)]
    for build, of in R.build_variants(dt):
        for nk in R.build_nks(build):
            cases.append((*R.build_shape(build, nk, dt), of, 0, R.ACT_RELU))
    seen = set()
    for i, (M, K, N, of, rp, act) in enumerate(cases):
        if (M, K, N, of, rp, act) in seen:
            continue
        seen.add((M, K, N, of, rp, act))
        a, w, b, res = R.routed_int_case(M, K, N, 11 + i % 7, rp is not None)
        ref = R.gemm_ref(a, w, b, res, act, rp or 0)
        assert float(ref.abs().max()) <= 256
        assert torch.equal(R.emulate(a, w, b, res, act, rp or 0, dt, of).double(), ref), (M, K, N, of, rp, act)


@pytest.mark.parametrize("dt", R.DTS)
def test_emulation_stays_within_the_bound(dt):
    """The admissibility condition: err / bound <= 1 for the fp32 emulation on the value, tail and later-tiles cases of the GPU file."""
    for (M, K, N, of, rp, act) in R.value_cases(dt):
        a, w, b, res = R.value_case(M, K, N, dt, of, 5)
        res = res if rp is not None else None
        q = _q(R.emulate(a, w, b, res, act, rp or 0, dt, of), R.gemm_ref(a, w, b, res, act, rp or 0), R.gemm_bound(a, w, b, res, act, rp or 0, dt, of))
        print(f"\n[gemm emulation value {dt} act {act} res {rp} out_f32 {of}] max err / bound {q:.3f}")
        _note("value", dt, q)
        assert q <= 1.0, (act, rp, of, q)
    for (nk, K, N, of, rp, act) in R.tail_cases(dt):
        a, w, b, res = R.tail_case(dt, nk, N, of)
        res = res if rp is not None else None
        q = _q(R.emulate(a, w, b, res, act, rp or 0, dt, of), R.gemm_ref(a, w, b, res, act, rp or 0), R.gemm_bound(a, w, b, res, act, rp or 0, dt, of))
        print(f"\n[gemm emulation tail {dt} nk {nk} N {N}] max err / bound {q:.3f}")
        _note("tail", dt, q)
        assert q <= 1.0, (nk, N, q)           # (every M of tail_M is a prefix of these 383 rows)
    for build, of in R.build_variants(dt):
        _, K, N, *_ = R.later_shape(build, dt, N_CU, 4)
        a, w, b, res = R.periodic_case(K, N, dt, of, 21)
        q = _q(R.emulate(a, w, b, res, R.ACT_GELU, 1, dt, of), R.gemm_ref(a, w, b, res, R.ACT_GELU, 1), R.gemm_bound(a, w, b, res, R.ACT_GELU, 1, dt, of))
        print(f"\n[gemm emulation later {dt} {build} out_f32 {of}] max err / bound {q:.3f}")
        _note("later", dt, q)
        assert q <= 1.0, (build, of, q)


# (kernel, type) pairs this bound cannot tell from a right kernel; the test asserts that they stay INSIDE, so each exemption is a checked statement:
#   the bias of the N-tail columns reaches only columns that are never stored -- the kernel zeroes it so that nothing depends on memory past
#   the bias vector, which no output can show;
#   wscale is 1 in every type but f16x2;
#   the two f16x2 mutants are the identity in the other types.
NOT_SEPARABLE = {("bias kept in the N tail", dt) for dt in R.DTS}
NOT_SEPARABLE |= {(m, dt) for m in ("bias times wscale", "f16x2 without lo hi", "f16x2 output without lo") for dt in ("f32", "bf16", "f16")}
LATER = ("residual of the previous tile", "accumulator not reset")
VALUE = ("f16x2 without lo hi", "f16x2 output without lo")


@pytest.mark.parametrize("dt", R.DTS)
def test_wrong_kernels_land_outside_the_bound(dt):
    of = 0
    routed = R.routed_int_case(300, 256, 232, 3)
    value = R.value_case(200, 128, 232, dt, of, 5)
    # later tiles in small: two row-tile lanes of four and three 128-row tiles, rows of period 97
    bm, gm, M = 128, 2, 128 * 7 - 41
    blk = R.periodic_case(R.bke(dt), 128, dt, of, 21)
    idx = torch.arange(M) % R.PERIOD
    later = (blk[0][idx], blk[1], blk[2], blk[3][idx])
    for name in R.MUTANTS:
        (a, w, b, res), act, rp = (later, R.ACT_GELU, 1) if name in LATER else ((value, R.ACT_GELU, 1) if name in VALUE else (routed, R.ACT_RELU, 0))
        ref, bound = R.gemm_ref(a, w, b, res, act, rp), R.gemm_bound(a, w, b, res, act, rp, dt, of)
        assert _q(R.emulate(a, w, b, res, act, rp, dt, of, None, bm, gm), ref, bound) <= 1.0
        q = _q(R.emulate(a, w, b, res, act, rp, dt, of, name, bm, gm), ref, bound)
        print(f"\n[gemm mutant {dt}] {name:32s} max err / bound {q:.3g}")
        if (name, dt) in NOT_SEPARABLE:
            assert q <= 1.0, (name, q)
        else:
            assert q > 1.0, (name, q)


def test_routed_case_meets_its_conditions():
    for (M, K, N) in ((300, 256, 128), (300, 256, 232), (600, 256, 64), (1499, 384, R.WIDE_N), (1499, 128, R.WIDE_N)):
        a, w, b, res = R.routed_int_case(M, K, N, 13)
        assert float(a.abs().max()) <= 7 and float(b.abs().max()) <= 8 and float(res.abs().max()) <= 32
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        cnt = (w != 0).sum(1)
        assert int(cnt.min()) >= 8 and int(cnt.max()) <= 12
        for n0 in range(0, N, 128):                                     # within every column tile every k is used by some column
            assert bool((w[n0:n0 + 128] != 0).any(0).all()), n0
        assert len({tuple(r) for r in a.int().tolist()}) == M and len({tuple(r) for r in w.int().tolist()}) == N
        for act in (R.ACT_NONE, R.ACT_RELU):
            for rp in (0, 1):
                y = R.gemm_ref(a, w, b, res, act, rp)
                assert float(y.abs().max()) <= 256 and torch.equal(y, y.round())
        pre = a.double() @ w.double().t()
        assert float((pre.abs() + b.double().abs() + res.double().abs()).max()) <= 256
    x, w4, b = R.routed_conv_case(2, 64, 9, 9, 128, 3, 5)
    assert w4.shape == (128, 64, 3, 3) and int((w4 != 0).sum((1, 2, 3)).min()) >= 8 and float(R.conv_ref(x, w4, b, 1, R.ACT_NONE).abs().max()) <= 256


def _lib():
    from ocr_vi_invoice_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("n_cu", (256, 304, 64))
def test_every_shape_reaches_the_build_it_names(n_cu):
    lib = _lib()
    for dt in R.DTS:
        small = lambda N: "256x64" if N == 64 else "128x128"
        for (M, K, N, of, rp, act) in R.routing_cases(dt) + R.value_cases(dt):
            assert R.plan_of(lib, dt, 0, M, K, N, of, rp is not None, n_cu)[:5] == (1, *R.expect(small(N), dt, of)), (dt, M, K, N, of)
        for (nk, K, N, of, rp, act) in R.tail_cases(dt):
            for M in R.tail_M:
                plan = R.plan_of(lib, dt, 0, M, K, N, of, rp is not None, n_cu)
                assert plan[:5] == (1, *R.expect("128x128", dt, of)), (dt, M, K, N)
                tiles = -(-M // 128)
                assert plan[5:] == (tiles * -(-N // 128), 1, 1), (dt, M, K, N, plan)     # one tile per workgroup: M <= 128 at nk = 1 is one step
        for build, of in R.build_variants(dt):
            for nk in R.build_nks(build):
                M, K, N = R.build_shape(build, nk, dt)
                assert R.plan_of(lib, dt, 0, M, K, N, of, True, n_cu)[:5] == (1, *R.expect(build, dt, of)), (dt, build, nk, of)
            counts = set()
            for t in (2, 4):
                M, K, N, gm, lo, hi = R.later_shape(build, dt, n_cu, t)
                plan = R.plan_of(lib, dt, 0, M, K, N, of, True, n_cu)
                assert plan[:5] == (1, *R.expect(build, dt, of)), (dt, build, t, plan)
                assert plan[5:] == (gm * (N // R.BUILDS[build][1]), lo, hi) and hi == lo + 1, (dt, build, t, plan)
                counts |= {lo, hi}
            assert any(c % 2 for c in counts) and any(c % 2 == 0 for c in counts)
            if n_cu >= 192:                       # (a big_m launch has 192 tiles or more: three or more per workgroup on a smaller device)
                assert counts == {1, 2, 3, 4}, (dt, build, counts)
        for (n, C, H, W, Co, ks, stride, build) in R.CONV_ROUTED:
            if ks == 3 and dt not in ("bf16", "f16"):
                continue
            M = n * ((H - 1) // stride[0] + 1) * ((W - 1) // stride[1] + 1)
            assert R.plan_of(lib, dt, 1 if ks == 3 else 0, M, ks * ks * C, Co, 0, False, n_cu)[:5] == (1, *R.expect(build, dt, 0)), (dt, M, C, Co)
    # and the hook's own edges: a K that is no multiple of the K-step and 64 columns in a 4-byte type are not ring GEMMs
    assert R.plan_of(lib, "bf16", 0, 300, 96, 128, 0, False, n_cu)[0] == 0
    assert R.plan_of(lib, "f32", 0, 300, 64, 64, 0, False, n_cu)[0] == 0
