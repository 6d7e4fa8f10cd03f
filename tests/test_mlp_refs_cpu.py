"""CPU: tests/mlp_refs.py separates right from wrong.  (1) mlp_ref is torch's own layer_norm / gelu / linear in float64.  (2) An fp32 + T
emulation of the kernels' order of operations stays within mlp_bound on every family, type, width and mode that
tests/test_gpu_mlp_fused.py runs: the inputs are admissible.  (3) Sixteen wrong kernels, applied to that emulation, land at
least 10x outside the bound on the family meant to expose them, and the five mutations of the float64 reference that the dense randn
test lets through in bf16 are rejected in every type.  (4) The routing tables scatter the four hidden units of an output as claimed and
the token-tail table reaches the lanes it claims.  Ratios are printed (pytest -s); profiles/r14_mlp_kernels.md has the tables."""
import pytest
import torch
import torch.nn.functional as F

import mlp_refs as R

DTS = ("bf16", "f16", "f16x2")
DS = (128, 256, 384)
PERMS = R.PERMS
M_ROUTE, M_EDGE = 129, 160          # what the GPU file uses


def _ratio(got, ref, bound):
    """max err / bound over x_new and xn; NaN or inf in `got` counts as infinite."""
    worst = 0.0
    for g, r, b in zip(got, ref, bound):
        if r is None:
            continue
        q = (g.double() - r).abs() / b
        q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
        worst = max(worst, float(q.max()))
    return worst


def _case(family, D, dt, perm="random", M=M_EDGE):
    return R.make_case(family, M, D, perm, dt)


_CACHE = {}


def _ref_and_bound(family, D, dt, mode, perm="random", M=M_EDGE):
    key = (family, D, dt, mode, perm, M)
    if key not in _CACHE:
        x, params, info = _case(family, D, dt, perm, M)
        tr = R.mlp_trace(x, *params, mode)
        _CACHE[key] = (x, params, info, (tr["y"], tr["xn"]), R.mlp_bound(x, *params, mode, dt, tr))
    return _CACHE[key]


def test_reference_is_torch_in_float64():
    x, params, _ = _case("rows", 128, "f16")
    lg, lb, w1, b1, w2, b2, ng, nb = [p.double() for p in params]
    xd = x.double()
    y = xd + F.linear(F.gelu(F.linear(F.layer_norm(xd, (128,), lg, lb, 1e-5), w1, b1)), w2, b2)
    got_y, got_n = R.mlp_ref(x, *params, "ln")
    # (F.gelu is x (1 + erf) / 2: it loses the tail's relative accuracy, not its absolute one)
    assert float((got_y - y).abs().max()) < 1e-12 * float(y.abs().max())
    assert float((got_n - F.layer_norm(y, (128,), ng, nb, 1e-5)).abs().max()) < 1e-9
    assert torch.equal(R.mlp_ref(x, *params, "cast")[1], got_y) and R.mlp_ref(x, *params, "none")[1] is None


def test_gelu_family_reaches_the_bands_it_claims():
    for D in DS:
        x, params, info = _case("gelu", D, "f16")
        pre = R.mlp_trace(x, *params, "none")["pre"][0]
        tgt = torch.empty(4 * D, dtype=torch.float64)
        tgt[info["H"].reshape(-1)] = R.gelu_targets(D).reshape(-1)
        assert float((pre - tgt).abs().max()) <= 2.0 ** -24 * 32         # fp32(b1), |b1| < 32
        assert int((pre == 0).sum()) >= 4 and float(pre.min()) < -12 and float(pre.max()) > 12
        assert int(((pre.abs() > 5e-5) & (pre.abs() < 2e-4)).sum()) >= 8
        assert int(((pre > -6) & (pre < -3)).sum()) >= D // 4 and int((pre > 6).sum()) >= D // 2
        h16 = R.gelu64(pre).abs()
        assert int(((h16 > 0) & (h16 < 2.0 ** -14)).sum()) >= D // 8       # fp16 subnormals and below


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", DS)
def test_emulation_stays_within_the_bound(D, dt):
    """The admissibility condition: max err / bound <= 1 for the fp32 emulation on every case of the GPU file."""
    cases = [("rows", perm, M_ROUTE, R.MODES[i]) for i, perm in enumerate(PERMS)]
    cases += [(fam, "random", M_EDGE, mode) for fam in ("rows", "gelu", "epilogue") for mode in R.MODES]
    for fam, perm, M, mode in cases:
        x, params, _, ref, bound = _ref_and_bound(fam, D, dt, mode, perm, M)
        q = _ratio(R.mlp_emulate(x, *params, mode, dt), ref, bound)
        print(f"\n[mlp emulation {fam} {perm} M={M} D={D} {mode} {dt}] max err / bound {q:.3f}")
        assert q <= 1.0, (fam, perm, mode, q)


def _swap(v, i, j):
    v = v.clone()
    v[[i, j]] = v[[j, i]]
    return v


def _mutants(dt, D):
    """name -> (family, index of the parameter to replace or None, function of (params) -> new parameter, emulation flags)."""
    ch = R.CHUNK[dt]
    h0 = 3 * ch + 16 + 8                      # chunk 3, hidden block 1, lane group 2: the first of a lane's k-slot group

    def chunk_zero(p):
        v = p[3].clone()
        v[2 * ch:3 * ch] = 0
        return v

    def group_shift(p):
        v = p[5].clone()
        v[16 + 4:16 + 8] = p[5][16 + 8:16 + 12]
        return v

    def kslot_swap(p):
        w = p[4].clone()
        w[:, [h0, h0 + 1]] = w[:, [h0 + 1, h0]]
        return w

    def slot_early(p):                         # chunk 1's h meets chunk 2's fc2 slice: chunk 1's slice is skipped, chunk 2's used twice
        w = p[4].clone()
        w[:, ch:2 * ch] = p[4][:, 2 * ch:3 * ch]
        return w

    return {
        "b1 pair swapped": ("rows", 3, lambda p: _swap(p[3], h0, h0 + 1), ()),
        "b1 of one chunk zero": ("rows", 3, chunk_zero, ()),
        "b2 pair swapped": ("epilogue", 5, lambda p: _swap(p[5], 5, 6), ()),
        "b2 lane group shifted": ("epilogue", 5, group_shift, ()),
        "ln_g pair swapped": ("rows", 0, lambda p: _swap(p[0], 9, 10), ()),
        "ln_b pair swapped": ("rows", 1, lambda p: _swap(p[1], 9, 10), ()),
        "next_g pair swapped": ("epilogue", 6, lambda p: _swap(p[6], 9, 10), ()),
        "next_b pair swapped": ("epilogue", 7, lambda p: _swap(p[7], 9, 10), ()),
        "fc2 k-slots swapped": ("rows", 4, kslot_swap, ()),
        "ring slot read early": ("rows", 4, slot_early, ()),
        "row 0 statistics": ("rows", None, None, ("row0_stats",)),
        "one-pass variance": ("rows", None, None, ("one_pass_var",)),
        "eps outside sqrt": ("rows", None, None, ("eps_outside",)),
        "norm2 without residual": ("rows", None, None, ("norm2_branch",)),
        "tanh gelu": ("gelu", None, None, ("gelu_tanh",)),
        "h rounded before bias": ("gelu", None, None, ("round_h_first",)),
    }


# f16x2 computes fc1 + b1 in fp32 and has no 16-bit value to round early: rounding fc1's accumulator to f16x2 costs 2^-23 of it, 6 x 2^-23 x
# gelu'(0) = 3.6e-7 at the most here, against u |x_new| = 1.2e-7 for the residual addition alone and 48 u |pre| for the gelu evaluation.
# This bound does not separate it; the test asserts that it stays INSIDE (ratio <= 1), so the exemption is a checked statement.
NOT_SEPARABLE = {("h rounded before bias", "f16x2")}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", DS)
def test_wrong_kernels_land_ten_times_outside(D, dt):
    for name, (fam, idx, make, flags) in _mutants(dt, D).items():
        x, params, _, ref, bound = _ref_and_bound(fam, D, dt, "ln")
        p = list(params)
        if idx is not None:
            p[idx] = make(params)
            assert not torch.equal(p[idx], params[idx]), name
        q = _ratio(R.mlp_emulate(x, *p, "ln", dt, flags), ref, bound)
        print(f"\n[mlp mutant D={D} {dt}] {name:24s} max err / bound {q:.3g}")
        if (name, dt) in NOT_SEPARABLE:
            assert q <= 1.0, (name, q)           # the complementary fact: such a kernel is admissible in f16x2
        else:
            assert q >= 10.0, (name, q)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", (256, 384))
def test_mutations_the_dense_test_lets_through_are_rejected(D, dt):
    """The five mutations of the float64 reference that test_mlp_fused_kernel's metric passes in bf16 (swapped b1 / b2 / ln_b pairs, a chunk's
    b1 zero, b1 dropped): each moves some element of x_new by more than its bound -- 10 x more -- in every type."""
    x, params, _, ref, bound = _ref_and_bound("rows", D, dt, "none")
    muts = {"b1 pair swapped": (3, _swap(params[3], 200, 201)), "b1 of a 64-chunk zero": (3, None), "b2 pair swapped": (5, _swap(params[5], 5, 6)),
            "ln_b pair swapped": (1, _swap(params[1], 9, 10)), "b1 dropped": (3, torch.zeros_like(params[3]))}
    z = params[3].clone()
    z[128:192] = 0
    muts["b1 of a 64-chunk zero"] = (3, z)
    for name, (idx, v) in muts.items():
        p = list(params)
        p[idx] = v
        q = _ratio(R.mlp_ref(x, *p, "none"), ref, bound)
        print(f"\n[mlp reference mutation D={D} {dt}] {name:24s} max err / bound {q:.3g}")
        assert q >= 10.0, (name, q)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("perm", PERMS)
def test_routing_tables_scatter_as_claimed(D, perm):
    pi1, H = R.routing_tables(D, perm, 5)
    assert torch.equal(torch.sort(H.reshape(-1)).values, torch.arange(4 * D))            # every hidden unit feeds exactly one output
    assert torch.equal(torch.bincount(pi1, minlength=D), torch.full((D,), 4))            # every input channel is read four times
    for ch in (64, 32):
        assert all(len(set((H[n] // ch).tolist())) == 4 for n in range(D)), ch           # four different chunks
    assert all(len(set(((H[n] >> 2) & 3).tolist())) == 4 for n in range(D))              # four different lane groups
    assert all(len(set((H[n] & 3).tolist())) == 4 for n in range(D))                     # four different k-slots
    for ch in (64, 32):                                                                   # every (chunk, lane group, k-slot) is somebody's
        assert len({(int(h) // ch, (int(h) >> 2) & 3, int(h) & 3) for h in H.reshape(-1)}) == 4 * D // ch * 16
    w1, w2, info = R.routed_weights(D, perm, 5, "bf16")
    assert int((w1 != 0).sum()) == 4 * D and int((w2 != 0).sum()) == 4 * D and int((w2 != 0).sum(-1).min()) == 4
    assert {abs(v) for v in w1[w1 != 0].tolist()} <= set(R.COEF)


def test_parameter_vectors_are_distinct_and_apart():
    for n in (128, 256, 384, 512, 1024, 1536):
        v = R.param_vector(n, 3)
        assert len(set(v.tolist())) == n and 0.25 <= float(v.abs().min()) and float(v.abs().max()) <= 2.0
        assert float((v[1:].abs() - v[:-1].abs()).abs().min()) > 0.5                       # neighbours in index differ by more than 0.5


def test_tail_table_reaches_the_lanes_it_claims():
    """M = 1: one lane of wave 0.  15 / 16 / 17: the last row of a block missing, a full block, one row into the next wave (the next block
    of the same wave in the 32-token build).  33: wave 2 (wave 1 there).  127 / 128 / 129: the last lane of the tile missing, the full tile,
    one token in a second tile.  257: a third tile, on a third workgroup."""
    want16 = {1: (0, 0, 0, 0), 15: (0, 0, 0, 14), 16: (0, 0, 0, 15), 17: (0, 1, 0, 0), 33: (0, 2, 0, 0), 127: (0, 7, 0, 14), 128: (0, 7, 0, 15),
              129: (1, 0, 0, 0), 257: (2, 0, 0, 0)}
    want32 = {1: (0, 0, 0, 0), 15: (0, 0, 0, 14), 16: (0, 0, 0, 15), 17: (0, 0, 1, 0), 33: (0, 1, 0, 0), 127: (0, 3, 1, 14), 128: (0, 3, 1, 15),
              129: (1, 0, 0, 0), 257: (2, 0, 0, 0)}
    assert set(R.TAIL_M) == set(want16)
    for M in R.TAIL_M:
        assert R.last_token_place(M, "bf16", 384) == want16[M] and R.last_token_place(M, "f16x2", 256) == want16[M]
        assert R.last_token_place(M, "f16x2", 384) == want32[M]
    for n_cu in (4, 64, 256, 304):
        tiles = (R.later_tiles_M(n_cu) + 127) // 128
        grid = min(tiles, n_cu)
        grid = -(-tiles // -(-tiles // grid))
        per = [(tiles - b + grid - 1) // grid for b in range(grid)]
        assert min(per) >= 2 and max(per) <= 3, (n_cu, per[:3])
