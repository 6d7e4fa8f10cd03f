"""CPU: tests/halo_refs.py against itself, before the GPU files use it on conv3_halo, bneck_tail and stem_pool.  On the cases
tests/test_gpu_conv3_halo_elements.py, test_gpu_bneck_tail_elements.py and test_gpu_stem_pool_elements.py launch (the later-tiles
launches at 64 CUs, where they are small) the fp32 emulation of each kernel is inside the per-element bound on value data and EQUAL to the
float64 reference on routed and probe data; every deliberately wrong kernel of halo_refs.MUTANTS leaves the bound or breaks an equality in
at least one family (the matrix is printed; the one mutant that cannot change a result is shown to be the identity); the routed and probe
builders have the properties the equalities rest on; and through ocrvi_test_halo_plan, which touches no device, every shape takes the
kernel and tiling named for 256, 304 and 64 CUs.  No GPU."""
import functools
import os

import pytest
import torch

import halo_refs as Hh
from aux_refs import round_to
from halo_refs import ACT_NONE, ACT_RELU, DT

torch.set_num_threads(min(16, os.cpu_count() or 1))
WORST = {}
CUS = (256, 304, 64)


def _lib():
    from ocr_vi_invoice_amd import _lib as L
    return L.load()


def _eq(got, ref, tag):
    bad = (got.double() != ref).nonzero()
    assert bad.numel() == 0, (tag, int(bad.shape[0]), [(r, c, float(got[r, c]), float(ref[r, c])) for r, c in bad[:6].tolist()])
    assert torch.equal(round_to(ref.float(), DT).double(), ref), (tag, "the reference is not exact in f16x2")


def _hold(got, ref, bound, fam, tag):
    q = float(Hh.err_ratio(got, ref, bound).max())
    WORST[fam] = max(WORST.get(fam, 0.0), q)
    assert q <= 1.0, (fam, tag, q)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[halo refs] largest err / bound of the fp32 emulations per family:")
    for fam in sorted(WORST):
        print(f"[halo refs]   {fam:24s} {WORST[fam]:.3f}")


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("n_cu", CUS)
def test_every_shape_takes_the_kernel_and_tiling_named(n_cu):
    lib = _lib()
    for (n, C, H, W, Co) in Hh.CONV_SHAPES:
        assert Hh.plan_of(lib, 0, n, C, H, W, Co, n_cu) == Hh.expect_plan(0, n, C, H, W, Co, n_cu), (n, C, H, W, Co)
    for (n, H, W) in Hh.BNECK_SHAPES:
        assert Hh.plan_of(lib, 1, n, 64, H, W, 256, n_cu) == Hh.expect_plan(1, n, 64, H, W, 256, n_cu)
    for (n, H, W) in Hh.STEM_SHAPES:
        assert Hh.plan_of(lib, 2, n, 3, H, W, 64, n_cu) == Hh.expect_plan(2, n, 3, H, W, 64, n_cu)
    # the tilings the shapes stand for, whatever the device: (NC, column tiles, tiles_x, tiles_y)
    tilings = [Hh.plan_of(lib, 0, *s, n_cu)[1:5] for s in Hh.CONV_SHAPES]
    assert tilings == [(64, 1, 1, 1), (64, 1, 1, 1), (128, 1, 1, 2), (128, 1, 2, 1), (128, 1, 2, 2), (64, 1, 2, 2), (128, 2, 5, 1), (128, 2, 3, 2)]
    assert [Hh.plan_of(lib, 2, n, 3, H, W, 64, n_cu)[3:5] for (n, H, W) in Hh.STEM_SHAPES] == [(1, 1), (1, 1), (1, 2), (2, 1), (2, 2), (4, 5)]
    # later tiles: 2 and 3 tiles per workgroup on a grid that is no multiple of an image's 9 tiles
    walked = set()
    for kind, Co in [(0, 64), (0, 128), (0, 256), (1, 64), (2, 64)]:
        for t in (2, 3):
            n, grid, lo, hi = Hh.later_shape(kind, n_cu, t, Co)
            H, W = (96, 84) if kind == 2 else (48, 48)
            plan = Hh.plan_of(lib, kind, n, 64, H, W, Co, n_cu)
            assert plan[0] == 1 and plan[3:5] == (3, 3) and plan[5:] == (grid, lo, hi) and hi == t and (grid // plan[2]) % 9, (kind, Co, t, plan)
            walked |= {lo, hi}
    assert walked >= {2, 3}


def test_plan_refuses_what_conv3_halo_does_not_take():
    lib = _lib()
    assert Hh.plan_of(lib, 0, 1, 48, 16, 16, 64, 256)[0] == 0          # half a channel block
    assert Hh.plan_of(lib, 0, 1, 64, 16, 16, 300, 256)[0] == 0         # more than 256 columns
    assert Hh.plan_of(lib, 0, 1, 64, 16, 16, 30, 256)[0] == 0          # 30: no whole 4-channel chunks (and a 32-column pack)


# ------------------------------------------------------------------------------------------------ builders
def test_routed_builders_cover_every_k_in_every_column_tile():
    for (n, C, H, W, Co) in Hh.CONV_SHAPES:
        x, w, b = Hh.routed_conv_case(n, C, H, W, Co, 3)
        wk = Hh.wk_of(w)
        nc = Hh.halo_plan(n, H, W, Co, 256)[0]
        for c0 in range(0, Co, nc):
            assert bool((wk[c0:c0 + nc] != 0).any(0).all()), (Co, c0)
        assert torch.unique(wk, dim=0).shape[0] == Co
        nnz = int((wk != 0).sum(1).max())
        assert nnz * 7 + 8 < 2 ** 11, (Co, nnz)
        assert float(Hh.conv_ref(x, w, b, ACT_NONE).abs().max()) < 2 ** 11
    t1, idn, (w2, b2, w3, b3, w1, b1) = Hh.routed_bneck_case(3, 17, 23, 5)
    assert bool((Hh.wk_of(w2) != 0).any(0).all()) and bool((w1 != 0).any(0).all())
    for q in range(8):
        assert bool((w3[32 * q:32 * q + 32] != 0).any(0).all()), q
    for m in (Hh.wk_of(w2), w3, w1):
        assert torch.unique(m, dim=0).shape[0] == m.shape[0]
    t2, y, tn = Hh.bneck_ref(t1, idn, (w2, b2, w3, b3, w1, b1))
    assert float(idn.min()) >= 0 and max(float(t2.max()), float(y.max()), float(tn.max())) < 65520
    for t in (t2, y, tn):
        assert torch.equal(t, t.round()) and torch.equal(round_to(t.float(), DT).double(), t)
    x, w, b = Hh.routed_stem_case(1, 36, 28, 7)
    wk = w.permute(0, 2, 3, 1).reshape(64, 147)
    assert bool((wk != 0).any(0).all()) and torch.unique(wk, dim=0).shape[0] == 64 and int((wk != 0).sum(1).max()) * 7 + 8 < 2 ** 11


def test_probe_builders_pin_every_position():
    for (n, C, H, W, Co) in Hh.CONV_SHAPES:
        seen = torch.zeros(C, dtype=torch.bool)
        for l in range(Hh.probe_a_launches(n, C, H, W)):
            x = Hh.probe_a_x(n, C, H, W, l)
            seen |= (x != 0).any(0).any(-1).any(-1)
            assert int(F_max_window(x, 3)) <= 1
        assert bool(seen.all()), (n, C, H, W)
        hit = torch.zeros(9 * C, dtype=torch.bool)
        for l in range(Hh.probe_b_launches(9 * C, Co)):
            wk = Hh.probe_b_weights(Co, 9 * C, l)
            assert bool(((wk != 0).sum(1) == 1).all())
            hit |= (wk != 0).any(0)
        assert bool(hit.all())
    for (n, H, W) in Hh.STEM_SHAPES:
        seen = torch.zeros(3, dtype=torch.bool)
        for l in range(Hh.probe_a_launches(n, 3, H, W, 7)):
            x = Hh.probe_a_x(n, 3, H, W, l, 7)
            seen |= (x != 0).any(0).any(-1).any(-1)
            assert int(F_max_window(x, 7)) <= 1
        assert bool(seen.all())
    hit = torch.zeros(147, dtype=torch.bool)
    for l in range(Hh.probe_b_launches(147, 64)):
        hit |= (Hh.probe_b_weights(64, 147, l) != 0).any(0)
    assert bool(hit.all())
    read = torch.zeros(256, dtype=torch.bool)
    for l in range(4):
        read |= (Hh.probe_c_bneck_case(1, 4, 4, l, 3)[2][4] != 0).any(0)
    assert bool(read.all())


def F_max_window(x, k):
    """The most non-zero entries any k x k window of x (all channels together) holds."""
    nz = (x != 0).float().sum(1, keepdim=True)
    return torch.nn.functional.avg_pool2d(nz, k, 1, k // 2, divisor_override=1).max()


def test_chain3_is_the_mfma_chain():
    g = torch.Generator().manual_seed(1)
    a, w = round_to(torch.randn(37, 96, generator=g), DT), round_to(torch.randn(20, 96, generator=g), DT)
    assert torch.equal(Hh._chain3(a, w), Hh._mfma_chain(a, w, DT))


# ------------------------------------------------------------------------------------------------ the emulations on the GPU files' cases
@pytest.mark.parametrize("i", range(len(Hh.CONV_SHAPES)))
def test_conv3_halo_emulation(i):
    n, C, H, W, Co = Hh.CONV_SHAPES[i]
    for act in (ACT_NONE, ACT_RELU):
        x, w, b = Hh.routed_conv_case(n, C, H, W, Co, 3 + i)
        _eq(Hh.emulate_conv(x, w, b, act), Hh.conv_ref(x, w, b, act), ("routed", i, act))
        x, w, b = Hh.value_conv_case(n, C, H, W, Co, 5 + i)
        _hold(Hh.emulate_conv(x, w, b, act), Hh.conv_ref(x, w, b, act), Hh.conv_bound(x, w, b, act), "conv3_halo value", (i, act))
    na, nb = Hh.probe_a_launches(n, C, H, W), Hh.probe_b_launches(9 * C, Co)
    for l in sorted({0, na // 2, na - 1}):
        x, w, b = Hh.probe_a_conv_case(n, C, H, W, Co, l, 7 + i)
        _eq(Hh.emulate_conv(x, w, b, ACT_NONE), Hh.conv_ref(x, w, b, ACT_NONE), ("probe a", i, l))
    for l in sorted({0, nb // 2, nb - 1}):
        x, w, b = Hh.probe_b_conv_case(n, C, H, W, Co, l, 9 + i)
        _eq(Hh.emulate_conv(x, w, b, ACT_NONE), Hh.conv_ref(x, w, b, ACT_NONE), ("probe b", i, l))


@pytest.mark.parametrize("i", range(len(Hh.BNECK_SHAPES)))
def test_bneck_tail_emulation(i):
    n, H, W = Hh.BNECK_SHAPES[i]
    for y_only in (False, True):
        t1, idn, wb = Hh.routed_bneck_case(n, H, W, 3 + i)
        _, y, tn = Hh.bneck_ref(t1, idn, wb)
        ey, et = Hh.emulate_bneck(t1, idn, wb, y_only)
        _eq(ey, y, ("routed y", i, y_only))
        if not y_only:
            _eq(et, tn, ("routed t1'", i))
    t1, idn, wb = Hh.value_bneck_case(n, H, W, 5 + i)
    (_, y, tn), (_, by, bt) = Hh.bneck_ref(t1, idn, wb), Hh.bneck_bound(t1, idn, wb)
    ey, et = Hh.emulate_bneck(t1, idn, wb)
    _hold(ey, y, by, "bneck_tail value y", i)
    _hold(et, tn, bt, "bneck_tail value t1'", i)
    for l in range(4):
        t1, idn, wb = Hh.probe_c_bneck_case(n, H, W, l, 7 + i)
        _, y, tn = Hh.bneck_ref(t1, idn, wb)
        ey, et = Hh.emulate_bneck(t1, idn, wb)
        _eq(ey, y, ("probe c y", i, l))
        _eq(et, tn, ("probe c t1'", i, l))
        assert torch.equal(y[:, :64], Hh.rows_of(t1).double()) and torch.equal(y[:, 128:], Hh.rows_of(idn)[:, 128:].double())
    na = Hh.probe_a_launches(n, 64, H, W)
    for name, case, ls in (("probe a", Hh.probe_a_bneck_case, sorted({0, na // 2, na - 1})), ("probe b", Hh.probe_b_bneck_case, (0, 4, 8))):
        for l in ls:
            t1, idn, wb = case(n, H, W, l, 11 + i)
            _, y, tn = Hh.bneck_ref(t1, idn, wb)
            ey, et = Hh.emulate_bneck(t1, idn, wb)
            _eq(ey, y, (name, "y", i, l))
            _eq(et, tn, (name, "t1'", i, l))
    t1, idn, wb = Hh.rounding_bneck_case(n, H, W)
    _, y, tn = Hh.bneck_ref(t1, idn, wb, round_t2=True)
    ey, et = Hh.emulate_bneck(t1, idn, wb)
    _eq(ey, y, ("rounding y", i))
    _eq(et, tn, ("rounding t1'", i))
    assert not torch.equal(y, Hh.bneck_ref(t1, idn, wb)[1])            # (the rounding of t2 is visible in y)


@pytest.mark.parametrize("i", range(len(Hh.STEM_SHAPES)))
def test_stem_emulation(i):
    n, H, W = Hh.STEM_SHAPES[i]
    for dt, fused in [(DT, True)] + [(d, False) for d in Hh.STEM_DTS]:
        x, w, b = Hh.routed_stem_case(n, H, W, 3 + i)
        _eq(Hh.emulate_stem(x, w, b, dt, fused), Hh.stem_ref(x, w, b), ("routed", i, dt, fused))
        for l in range(Hh.probe_a_launches(n, 3, H, W, 7)):
            x, w, b = Hh.probe_a_stem_case(n, H, W, l, dt, 7 + i)
            ref = Hh.stem_ref(x, w, b)
            got = Hh.emulate_stem(x, w, b, dt, fused)
            assert torch.equal(got.double(), ref) and torch.equal(round_to(ref.float(), dt).double(), ref), ("probe a", i, dt, l)
        for l in range(Hh.probe_b_launches(147, 64)):
            x, w, b = Hh.probe_b_stem_case(n, H, W, l, dt, 9 + i)
            ref = Hh.stem_ref(x, w, b)
            assert torch.equal(Hh.emulate_stem(x, w, b, dt, fused).double(), ref) and torch.equal(round_to(ref.float(), dt).double(), ref), ("probe b", i, dt, l)
        x, w, b = Hh.value_stem_case(n, H, W, dt, 5 + i)
        _hold(Hh.emulate_stem(x, w, b, dt, fused), Hh.stem_ref(x, w, b), Hh.stem_bound(x, w, b, dt), f"stem value {dt} {'fused' if fused else 'two kernels'}", i)


@pytest.mark.parametrize("t", (2, 3))
def test_later_tiles_emulation_at_64_cus(t):
    for (C, Co) in Hh.LATER_CONV:
        n = Hh.later_shape(0, 64, t, Co)[0]
        x, w, b = Hh.routed_conv_case(n, C, 48, 48, Co, 40 + t)
        _eq(Hh.emulate_conv(x, w, b, ACT_RELU, n_cu=64), Hh.conv_ref(x, w, b, ACT_RELU), ("later conv", C, Co, t))
    n = Hh.later_shape(1, 64, t)[0]
    t1, idn, wb = Hh.routed_bneck_case(n, 48, 48, 50 + t)
    _, y, tn = Hh.bneck_ref(t1, idn, wb)
    ey, et = Hh.emulate_bneck(t1, idn, wb, n_cu=64)
    _eq(ey, y, ("later y", t))
    _eq(et, tn, ("later t1'", t))
    n = Hh.later_shape(2, 64, t)[0]
    x, w, b = Hh.routed_stem_case(n, 96, 84, 60 + t)
    _eq(Hh.emulate_stem(x, w, b, n_cu=64), Hh.stem_ref(x, w, b), ("later stem", t))


# ------------------------------------------------------------------------------------------------ the wrong kernels
N_CU_M = 64       # the mutants about a workgroup's later tiles need launches in which there are some: the later-tiles launches at 64 CUs


@functools.lru_cache(None)
def _conv_families():
    """family -> [(x, w, b, act, reference, bound or None)]: a few of the GPU files' launches per family."""
    fam = {"routed": [], "probe a": [], "probe b": [], "value": [], "later tiles": []}
    for i in (4, 5, 6, 7):
        n, C, H, W, Co = Hh.CONV_SHAPES[i]
        x, w, b = Hh.routed_conv_case(n, C, H, W, Co, 3 + i)
        fam["routed"].append((x, w, b, ACT_NONE, Hh.conv_ref(x, w, b, ACT_NONE), None))
        x, w, b = Hh.probe_a_conv_case(n, C, H, W, Co, 0, 7 + i)
        fam["probe a"].append((x, w, b, ACT_NONE, Hh.conv_ref(x, w, b, ACT_NONE), None))
        nb = Hh.probe_b_launches(9 * C, Co)
        for l in (nb // 2, nb - 1):
            x, w, b = Hh.probe_b_conv_case(n, C, H, W, Co, l, 9 + i)
            fam["probe b"].append((x, w, b, ACT_NONE, Hh.conv_ref(x, w, b, ACT_NONE), None))
        x, w, b = Hh.value_conv_case(n, C, H, W, Co, 5 + i)
        fam["value"].append((x, w, b, ACT_NONE, Hh.conv_ref(x, w, b, ACT_NONE), Hh.conv_bound(x, w, b, ACT_NONE)))
    for (C, Co) in Hh.LATER_CONV[:2]:
        n = Hh.later_shape(0, N_CU_M, 2, Co)[0]
        x, w, b = Hh.routed_conv_case(n, C, 48, 48, Co, 42)
        fam["later tiles"].append((x, w, b, ACT_RELU, Hh.conv_ref(x, w, b, ACT_RELU), None))
    return fam


def _caught(got, ref, bound):
    if bound is None:
        return not torch.equal(got.double(), ref)
    return float(Hh.err_ratio(got, ref, bound).max()) > 1.0


@functools.lru_cache(None)
def _bneck_families():
    fam = {"routed": [], "probe a": [], "probe b": [], "probe c": [], "rounding": [], "value": []}
    n, H, W = 3, 17, 23
    for l in (0, 1):
        t1, idn, wb = Hh.probe_a_bneck_case(n, H, W, l, 11)
        fam["probe a"].append((t1, idn, wb, False, Hh.bneck_ref(t1, idn, wb), None))
    for l in (4, 8):
        t1, idn, wb = Hh.probe_b_bneck_case(n, H, W, l, 12)
        fam["probe b"].append((t1, idn, wb, False, Hh.bneck_ref(t1, idn, wb), None))
    for y_only in (False, True):
        t1, idn, wb = Hh.routed_bneck_case(n, H, W, 6)
        fam["routed"].append((t1, idn, wb, y_only, Hh.bneck_ref(t1, idn, wb), None))
    for l in (0, 3):
        t1, idn, wb = Hh.probe_c_bneck_case(n, H, W, l, 9)
        fam["probe c"].append((t1, idn, wb, False, Hh.bneck_ref(t1, idn, wb), None))
    t1, idn, wb = Hh.rounding_bneck_case(n, H, W)
    fam["rounding"].append((t1, idn, wb, False, Hh.bneck_ref(t1, idn, wb, round_t2=True), None))
    t1, idn, wb = Hh.value_bneck_case(n, H, W, 8)
    fam["value"].append((t1, idn, wb, False, Hh.bneck_ref(t1, idn, wb), Hh.bneck_bound(t1, idn, wb)))
    return fam


@functools.lru_cache(None)
def _stem_families():
    fam = {"routed": [], "probe a": [], "probe b": [], "value": [], "later tiles": []}
    for (n, H, W) in ((3, 36, 52), (1, 132, 88)):
        x, w, b = Hh.routed_stem_case(n, H, W, 6)
        fam["routed"].append((x, w, b, Hh.stem_ref(x, w, b), None))
        x, w, b = Hh.probe_a_stem_case(n, H, W, 0, DT, 10)
        fam["probe a"].append((x, w, b, Hh.stem_ref(x, w, b), None))
        for l in range(3):
            x, w, b = Hh.probe_b_stem_case(n, H, W, l, DT, 12)
            fam["probe b"].append((x, w, b, Hh.stem_ref(x, w, b), None))
        x, w, b = Hh.value_stem_case(n, H, W, DT, 8)
        fam["value"].append((x, w, b, Hh.stem_ref(x, w, b), Hh.stem_bound(x, w, b)))
    n = Hh.later_shape(2, N_CU_M, 2)[0]
    x, w, b = Hh.routed_stem_case(n, 96, 84, 62)
    fam["later tiles"].append((x, w, b, Hh.stem_ref(x, w, b), None))
    return fam


def _matrix():
    rows = {}
    for mut in Hh.MUTANTS:
        hits = []
        if not mut.startswith(("bneck:", "stem:")):
            for fam, cases in _conv_families().items():
                if any(_caught(Hh.emulate_conv(x, w, b, act, mut, N_CU_M), ref, bd) for (x, w, b, act, ref, bd) in cases):
                    hits.append("conv3_halo " + fam)
        if not mut.startswith("stem:"):
            for fam, cases in _bneck_families().items():
                for (t1, idn, wb, y_only, (_, y, tn), bd) in cases:
                    ey, et = Hh.emulate_bneck(t1, idn, wb, y_only, mut, N_CU_M)
                    if _caught(ey, y, None if bd is None else bd[1]) or (et is not None and _caught(et, tn, None if bd is None else bd[2])):
                        hits.append("bneck_tail " + fam)
                        break
        if mut.startswith("stem:"):
            for fam, cases in _stem_families().items():
                if any(_caught(Hh.emulate_stem(x, w, b, DT, True, mut, N_CU_M), ref, bd) for (x, w, b, ref, bd) in cases):
                    hits.append("stem " + fam)
        rows[mut] = hits
    return rows


def test_every_wrong_kernel_is_caught_by_some_family():
    rows = _matrix()
    print("\n[halo refs] which family catches which wrong kernel:")
    for mut, hits in rows.items():
        print(f"[halo refs]   {mut:48s} {', '.join(hits) if hits else ('- (cannot change a result)' if mut in Hh.EQUIVALENT else 'NOTHING')}")
    missed = [m for m, hits in rows.items() if not hits and m not in Hh.EQUIVALENT]
    assert not missed, missed
    for mut in Hh.EQUIVALENT:           # the pool runs behind a ReLU: padding it with 0 or with -inf is one function
        for cases in _stem_families().values():
            for (x, w, b, ref, bd) in cases:
                assert torch.equal(Hh.emulate_stem(x, w, b, DT, True, mut), Hh.emulate_stem(x, w, b, DT, True))
    # the kernel-specific mutants are caught in their own kernel's families, the unit-loop ones in conv3_halo's and in bneck_tail's phase A
    assert any(h.startswith("bneck_tail") for h in rows["taps (r, s) exchanged"]) and any(h.startswith("conv3_halo") for h in rows["taps (r, s) exchanged"])
