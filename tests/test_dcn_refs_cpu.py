"""CPU: tests/dcn_refs.py separates right from wrong.  (1) dcn_ref is the oracle's deform_conv2d_gather in float64, and its grid_sample
formulation.  (2) An fp32 + T emulation of the two kernels' order of operations EQUALS the reference on every probe case of
tests/test_gpu_dcn_sampling.py in all four types and stays within dcn_bound on every value case: the inputs are admissible.  (3) Sixteen
wrong kernels, applied to that emulation, are each caught by at least one case of the GPU list (a table of kernel against family is
printed); the (kernel, type) pairs that cannot be told apart are asserted to stay inside, by name.  (4) Through ocrvi_test_dcn_plan (host
only) on devices of 256, 304 and 64 compute units the case list reaches every patch shape on a ragged map, both column tiles with and
without an N tail, odd and even K-step counts in every type, both row tiles of fp32, and a launch whose workgroups walk more than one tile.
Ratios are printed (pytest -s); profiles/r18_dcn_sampling.md has the tables."""
import pytest
import torch

import dcn_refs as D

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\n[dcn emulation] value  " + "   ".join(f"{dt} {WORST.get(dt, float('nan')):.3f}" for dt in D.DTS))


def _rows_of_nchw(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def test_reference_is_the_oracle_in_float64():
    """Against deform_conv2d_gather: the same sums in another order (the oracle adds corner by corner into K = 9 C columns in (channel, tap)
    order and multiplies weight x columns; dcn_ref multiplies columns x weight^T in (tap, channel) order).  Two float64 sums of K products
    in any two orders differ by at most 2 K 2^-53 S, S = sum |column| |w|, and the columns themselves -- four products and three additions
    each way -- by 8 x 2^-53 Sabs, carried through |W|: that, per element, is the tolerance; nothing is added to it.  Measured: the largest
    difference is 0.005 of it.  Against deform_conv2d_gridsample (maps of two or more rows and columns): its round trip through normalised
    coordinates moves a position by a few ulps of float64 at magnitude <= 256, below 2^-42, and with it every bilinear weight: 2^-40
    max |x| sum |w| per output covers the four corners."""
    from oracle import dbnet_cpu
    worst = 0.0
    for (name, N, C, H, W, Co, stride, wr) in D.cases("f32"):
        x, off, mask, w, b, _ = D.inputs("value", "f32", (name, N, C, H, W, Co, stride, wr))
        ref = D.dcn_ref(x, off, mask, w, torch.zeros(Co), None, stride, relu=False)
        got = _rows_of_nchw(dbnet_cpu.deform_conv2d_gather(x.double(), off.double(), mask.double(), w.double(), stride))
        cols, sabs = D.sample_columns(x, off, mask, stride)
        wabs = D.weight_rows(w).double().abs()
        tol = (2 * 9 * C * 2.0 ** -53) * (cols.abs() @ wabs.t()) + 8 * 2.0 ** -53 * (sabs @ wabs.t())
        q = float(D.err_ratio(got, ref, tol).max())
        worst = max(worst, q)
        assert q <= 1.0, (name, q)
        if H > 1 and W > 1:
            gs = _rows_of_nchw(dbnet_cpu.deform_conv2d_gridsample(x.double(), off.double(), mask.double(), w.double(), stride))
            lim = 2.0 ** -40 * float(x.abs().max()) * wabs.sum(1)
            assert bool(((gs - ref).abs() <= lim).all()), (name, float((gs - ref).abs().max()))
    print(f"\n[dcn reference] largest |gather - dcn_ref| / tolerance {worst:.3f}")


@pytest.mark.parametrize("dt", D.DTS)
def test_emulation_equals_the_reference_on_probe_cases(dt):
    for fam, case, kind in D.gpu_list(dt):
        if fam != "probe":
            continue
        x, off, mask, w, b, res = D.inputs(fam, dt, case, kind)
        ref, _ = D.ref_and_bound(fam, dt, case, kind)
        out = D.emulate(x, off, mask, w, b, res, case[6], dt)
        bad = (out.double() != ref).nonzero()
        assert bad.numel() == 0, (dt, case, kind, bad[:4].tolist())


def test_probe_cases_answer_for_themselves():
    """The wild entries sample nothing and mask 0 gives the bias: from the reference alone."""
    for dt in ("bf16", "f32"):
        case = D.small_case(dt)
        name, N, C, H, W, Co, stride, wr = case
        x, off, mask, w, b, _ = D.inputs("probe", dt, case, "mask0")
        ref, _ = D.ref_and_bound("probe", dt, case, "mask0")
        dead = torch.tensor([D.probe_where(j, C, dt)[0] in (1, 4, 8) for j in range(Co)])
        assert bool((ref[:, dead] == torch.clamp(b.double(), min=0.0)[dead]).all()) and int(dead.sum()) > 0
        x, off, mask, w, b, _ = D.inputs("probe", dt, case, "wild")
        cols, _ = D.sample_columns(x, off, mask, stride)
        o = off.permute(0, 2, 3, 1).reshape(-1, 9, 2)
        gone = ~(o.abs() <= D.OFF_MAX).all(-1)                                   # (NaN compares false)
        assert int(gone.sum()) > 50 and {v for v in torch.tensor(D.WILD).tolist() if v == v} <= set(o[gone].flatten().tolist())
        assert bool(torch.isnan(o[gone]).any()) and bool((cols.reshape(-1, 9, C)[gone] == 0).all())


@pytest.mark.parametrize("dt", D.DTS)
def test_emulation_stays_within_the_bound(dt):
    for fam, case, kind in D.gpu_list(dt):
        if fam != "value":
            continue
        x, off, mask, w, b, res = D.inputs(fam, dt, case, kind)
        ref, bound = D.ref_and_bound(fam, dt, case, kind)
        q = float(D.err_ratio(D.emulate(x, off, mask, w, b, res, case[6], dt), ref, bound).max())
        print(f"\n[dcn emulation value {dt} {case[0]} C {case[2]} Co {case[5]}] max err / bound {q:.3f}")
        WORST[dt] = max(WORST.get(dt, 0.0), q)
        assert q <= 1.0, (dt, case, q)


# (kernel, type) pairs that cannot be told from a right kernel: the f16x2 pack in the other types, and pixel_of, which conv_gemm (fp32) has not.
NOT_SEPARABLE = {("f16x2 pack without lo", dt) for dt in ("f32", "bf16", "f16")} | {("patch row and column exchanged", "f32")}


@pytest.mark.parametrize("dt", D.DTS)
def test_every_wrong_kernel_is_caught_by_a_case_of_the_gpu_list(dt):
    """Per family, the first case that catches the kernel (probe: an element differs or is never stored; value: an element outside the
    bound), or "-" when no case of that family does.  Every kernel needs one family at least."""
    runs = [r for r in D.gpu_list(dt) if r[1][0] != D.PERSIST[0]]
    for name in D.MUTANTS:
        caught = {}
        for fam, case, kind in runs:
            if fam in caught:
                continue
            x, off, mask, w, b, res = D.inputs(fam, dt, case, kind)
            ref, bound = D.ref_and_bound(fam, dt, case, kind)
            out = D.emulate(x, off, mask, w, b, res, case[6], dt, mut=name)
            hit = bool((out.double() != ref).any()) if fam == "probe" else float(D.err_ratio(out, ref, bound).max()) > 1.0
            if hit:
                caught[fam] = f"{case[0]}{'' if kind == 'plain' else ' ' + kind}"
        print(f"\n[dcn mutant {dt}] {name:52s} probe {caught.get('probe', '-'):14s} value {caught.get('value', '-')}")
        if (name, dt) in NOT_SEPARABLE:
            assert not caught, (name, dt, caught)
        else:
            assert caught, (name, dt)


def _lib():
    from ocr_vi_invoice_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("n_cu", (256, 304, 64))
def test_the_case_list_reaches_what_it_names(n_cu):
    lib = _lib()
    lws, cols, rows32 = {}, set(), set()
    for dt in D.DTS:
        nks = set()
        for (name, N, C, H, W, Co, stride, wr) in D.cases(dt) + [D.small_case(dt)]:
            plan = D.plan_of(lib, dt, N, C, H, W, Co, stride, n_cu)
            assert plan == D.expect_plan(dt, N, C, H, W, Co, stride, n_cu), (dt, name, plan)
            assert plan[0] == (1 if dt in D.PIPE else 0)
            nks.add(plan[7] % 2)
            cols.add((dt in D.PIPE, plan[2], Co % plan[2] != 0, -(-Co // plan[2])))
            if dt in D.PIPE:
                lw = plan[3]
                Ho, Wo = D.out_hw(H, W, stride)
                assert lw == D.patch_lw(Ho, Wo) and (name not in D.MAP_LW or D.MAP_LW[name] == lw), (name, lw)
                if Ho % (128 >> lw) or Wo % (1 << lw):
                    lws.setdefault(dt, set()).add(lw)
            else:
                rows32.add(plan[1])
        assert nks == {0, 1}, (dt, nks)                      # odd and even K-step counts in every type
        if dt in D.PIPE:
            name, N, C, H, W, Co, stride, _ = D.persist_case(dt)
            plan = D.plan_of(lib, dt, N, C, H, W, Co, stride, n_cu)
            assert plan == D.expect_plan(dt, N, C, H, W, Co, stride, n_cu) and plan[4] > n_cu and plan[6] >= 2, (dt, plan)
            assert lws[dt] == {2, 3, 4, 5, 6, 7}, (dt, lws[dt])      # every patch shape, each on a ragged map
    for pipe in (True, False):                                # both column tiles: with an N tail (72, 200), exact (128, 256), several tiles (320, 512)
        assert {c[1:] for c in cols if c[0] == pipe} == {(128, True, 1), (128, False, 1), (128, True, 3), (256, True, 1), (256, False, 1), (256, False, 2)}, cols
    assert rows32 == {32, 64}, rows32                          # fp32: both row tiles of conv_gemm's deformable mode
    print(f"\n[dcn plan {n_cu} CUs] patch_lw on ragged maps {sorted(lws['bf16'])}; fp32 row tiles {sorted(rows32)}; column tiles (pipe, BN, N tail, tiles) {sorted(cols)}")
