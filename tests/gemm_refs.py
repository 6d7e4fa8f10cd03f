"""The ring GEMM (csrc/gemm_ring.h, dispatched by csrc/conv_launch.h: ring_plan) in plain float64, a per-element error bound derived from the
reference's own intermediates, an fp32 emulation of the kernel's order of operations with fourteen deliberate errors, and the input
families and shapes of tests/test_gpu_ring_gemm.py.  tests/test_gemm_refs_cpu.py shows on the CPU that the emulation stays inside the bound
on every case the GPU file runs, that the wrong kernels land outside it, and -- through ocrvi_test_ring_plan, which touches no device --
that every shape reaches the build it names for 256, 304 and 64 compute units.  No GPU, no library: torch and numpy only.

    out = act(a W^T + b (+ res))        res_post = 0 (ResNet: relu(bn(conv) + identity))
    out = act(a W^T + b) + res          res_post = 1 (x + mixer(x))
"""
import torch
import torch.nn.functional as F

from aux_refs import U32, half_ulp, round_to
from mlp_refs import _gelu_err, _mfma_chain, _x2_scale, gelu64, gelu_erf32

DTS = ("f32", "f16x2", "bf16", "f16")
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
tail_M = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 383)
PERIOD = 97


def bke(dt):
    """Elements of one 128-byte K-step."""
    return 32 if dt in ("f32", "f16x2") else 64


def out_type(dt, out_f32):
    """The element type the output (and a residual) is stored in: raw fp32, or T."""
    return "f32" if (out_f32 or dt == "f32") else dt


def _act64(y, act):
    return y if act == ACT_NONE else (torch.clamp(y, min=0.0) if act == ACT_RELU else gelu64(y))


def gemm_ref(a, w, b, res, act, res_post):
    """act(a W^T + b (+ res)) or act(a W^T + b) + res in float64."""
    y = a.double() @ w.double().t() + b.double()
    if res is not None and not res_post:
        y = y + res.double()
    y = _act64(y, act)
    if res is not None and res_post:
        y = y + res.double()
    return y


def gemm_bound(a, w, b, res, act, res_post, dt, out_f32, a_err=None):
    """Bound on |kernel - gemm_ref| per element for element type `dt` and output type out_type(dt, out_f32).  a, w must be exact in `dt`
    and res in the output type (the case builders pre-round them), so the hook's casts are exact.  With u = 2^-24, step by step:
      products  16-bit and f16x2: exact in fp32 (at most 11 x 11 significant bits per partial product).  f16x2 has three partial products
                per weight (lo hi, hi lo, hi hi) and drops lo lo <= 2^-11 |w| 2^-11 |a| = 4 u |w| |a| (`ll`).  fp32: one rounding each;
      sum       16-bit and f16x2: n - 1 additions of non-zero terms, n = the most non-zero (partial) products of any output, 2 u each relative
                to S = sum |a| |w| -- the order and the rounding of the additions inside an MFMA are not documented, 1 ulp covers a truncating
                adder -- so (2 (n - 1) u + ll) S.  fp32: the classical bound of a length-K inner product in any order, K u S.  The fp32 and
                f16x2 builds start the accumulator at the bias (divided by the power-of-two weight scale: exact), so every partial sum carries
                it: S includes |b| there, and fp32 counts K + 1 terms;
      bias      one rounding, u |pre| (the 16-bit builds add it in the epilogue; charged to all);
      residual  one fp32 addition, u |pre + res|;
      act       ReLU is 1-Lipschitz; GELU: mlp_refs._gelu_err (the image of the error interval plus the error of common.h's gelu_erf);
      output    half an ulp of the output type at |y| + e (aux_refs.half_ulp), nothing for raw fp32.
    a_err (tests/dcn_refs.py): the kernel builds its A operand itself and a is that operand in float64, known only to within a_err >= 0 per
    element.  What the kernel multiplies is some a' with |a' - a| <= a_err, exact in `dt`: S is taken over |a| + a_err, and
    a_err |W|^T -- the error of a itself, carried through the weights -- is added."""
    for t, name in ((a, "a"), (w, "w")) if a_err is None else ((w, "w"),):
        assert torch.equal(round_to(t.float(), dt), t.float()), f"{name} must be exact in {dt}"
    ot = out_type(dt, out_f32)
    if res is not None:
        assert torch.equal(round_to(res.float(), ot), res.float()), "res must be exact in the output type"
    A, W = a.double(), w.double()
    bd = b.double()
    S = (A.abs() if a_err is None else A.abs() + a_err.double()) @ W.abs().t()
    K = a.shape[1]
    if dt in ("f32", "f16x2"):
        S = S + bd.abs()
    if dt == "f32":
        e = (K + 1) * U32 * S
    else:
        terms = 3 if dt == "f16x2" else 1
        n = int(((A != 0).double() @ (W != 0).double().t()).max()) * terms + (1 if dt == "f16x2" else 0)
        e = (2 * max(n - 1, 0) * U32 + (4 * U32 if dt == "f16x2" else 0.0)) * S
    if a_err is not None:
        e = e + a_err.double() @ W.abs().t()
    pre = A @ W.t() + bd
    e = e + U32 * (pre.abs() + e)
    if res is not None and not res_post:
        pre = pre + res.double()
        e = e + U32 * (pre.abs() + e)
    if act == ACT_GELU:
        e = _gelu_err(pre, e)
    y = _act64(pre, act)
    if res is not None and res_post:
        y = y + res.double()
        e = e + U32 * (y.abs() + e)
    if ot != "f32":
        e = e + half_ulp(y.abs() + e, ot)
    return e


def err_ratio(got, ref, bound):
    """err / bound per element (float64), 0 where both are 0 (GELU's far negative tail is exactly 0 in the reference and in the bound) and
    inf where the bound is 0 and the error is not, or where `got` is not finite."""
    err = (got.double() - ref).abs()
    q = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return torch.where(torch.isfinite(got.double()), q, torch.full_like(q, float("inf")))


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernel
MUTANTS = ("last k-step dropped", "one k-group dropped", "A k-groups against B's", "bias of the next column tile", "bias kept in the N tail",
           "bias times wscale", "residual of row m + 1", "residual of the previous tile", "accumulator not reset", "res_post flipped",
           "f16x2 without lo hi", "f16x2 output without lo", "row M-1 for row M-2", "channels c and c + 4 exchanged")


def emulate(a, w, b, res, act, res_post, dt, out_f32, mut=None, bm=128, gm=1):
    """The kernel in float32: mlp_refs._mfma_chain over K (one MFMA per 32 k, the accumulator rounded to fp32 after each; f16x2's three
    partial products on scaled, split weights), the accumulators of the fp32 and f16x2 builds starting at bias / wscale and the 16-bit
    builds adding the bias in the epilogue, the residual before or after the activation, the output rounded to its type (f16x2: packed
    as hi + lo).  Not followed: the order inside an MFMA (and that a 16-bit K-step feeds its two MFMAs from interleaved 8-element
    groups), fp32's individual product roundings, fmas.  bm, gm: the row tile and the row-tile lanes of the launch, which the two mutants
    about a workgroup's earlier tiles need (row tile t belongs to lane t % gm; its predecessor there is tile t - gm).
    `mut`: one of MUTANTS, a deliberately wrong kernel."""
    assert mut is None or mut in MUTANTS, mut
    a, w, b = a.float().clone(), w.float().clone(), b.float().clone()
    res = None if res is None else res.float()
    M, K = a.shape
    N = w.shape[0]
    step, ot, split = bke(dt), out_type(dt, out_f32), dt == "f16x2"
    bias_first = dt in ("f32", "f16x2")
    wscale = 1.0 / _x2_scale(w) if split else 1.0
    if mut == "last k-step dropped":
        a[:, K - step:] = 0
    elif mut == "one k-group dropped":                       # group 5 of the middle step (8 elements: one lane group's 16 or 32 bytes)
        k0 = (K // step // 2) * step + 5 * (step // 8)
        a[:, k0:k0 + step // 8] = 0
    elif mut == "A k-groups against B's":                    # A's fragment offsets foa0 / foa1 exchanged, B's not
        g = step // 8
        a = a.reshape(M, K // (2 * g), 2, g).flip(2).reshape(M, K)
    elif mut == "row M-1 for row M-2" and M >= 2:            # the clamp of rows past M applied one row early
        a[M - 2] = a[M - 1]
    elif mut == "f16x2 without lo hi" and split:             # the w_lo a_hi product: the weights lose their lo halves
        s = _x2_scale(w)
        w = ((w.double() * s).float().half().double() / s).float()
    Np = -(-N // 128) * 128 if N > 64 else 64
    bp = torch.zeros(Np + 128)
    bp[:N] = b
    if mut == "bias kept in the N tail":                     # columns N .. Np - 1 see a bias; they are never stored
        bp[N:Np] = 3.0
    if mut == "bias of the next column tile":
        bp = torch.cat([bp[128:], torch.zeros(128)])
    wp = torch.zeros(Np, K)
    wp[:N] = w
    bv = bp[:Np]
    if mut == "bias times wscale":
        bv = bv * (wscale * wscale if bias_first else wscale)
    if split:
        wp[N:] = 0.0                                          # (the scale comes from w: the padding rows are zero)
    chain = lambda acc0: _mfma_chain(a, wp, dt, acc0) if not split else _chain_x2(a, wp, w, acc0)
    acc = chain(bv if bias_first else None)
    if mut == "accumulator not reset" and M > 2 * gm * bm:   # a lane's tile i + 2 starts from the finished tile i of the same set
        raw = chain(None)
        acc = acc.clone()
        acc[2 * gm * bm:] = acc[2 * gm * bm:] + raw[:M - 2 * gm * bm]
    v = acc if bias_first else acc + bv
    v = v[:, :N]
    if res is not None:
        if mut == "residual of row m + 1":
            res = torch.roll(res, -1, 0)
        elif mut == "residual of the previous tile" and M > gm * bm:
            res = torch.cat([res[:gm * bm], res[:M - gm * bm]])
    post = bool(res_post) != (mut == "res_post flipped")
    fact = {ACT_NONE: lambda t: t, ACT_RELU: lambda t: torch.clamp(t, min=0.0), ACT_GELU: gelu_erf32}[act]
    if res is not None and not post:
        v = v + res
    v = fact(v)
    if res is not None and post:
        v = v + res
    if mut == "f16x2 output without lo" and ot == "f16x2":
        v = v.half().float()
    out = round_to(v, ot)
    if mut == "channels c and c + 4 exchanged":
        n8 = N // 8 * 8
        out = torch.cat([out[:, :n8].reshape(M, n8 // 8, 2, 4).flip(2).reshape(M, n8), out[:, n8:]], 1)
    return out


def _chain_x2(a, wp, w, acc0):
    """_mfma_chain for f16x2 on the padded weights, with the scale of the unpadded ones (the same number: padding rows are zero)."""
    assert _x2_scale(wp) == _x2_scale(w)
    return _mfma_chain(a, wp, "f16x2", acc0)


# ------------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def routed_weights(N, K, seed):
    """w [N, K]: 8 to 12 entries of +-1 per row, all else zero.  Column n of a tile of nc columns (128, or what is left of N) uses
    k = c, c + nc, c + 2 nc, ... with c its index in the tile, so within every column tile every k is used by some column; the rest of
    its entries are seeded."""
    g = _gen(seed)
    n = torch.arange(N)
    tile0 = n // 128 * 128
    nc = torch.clamp(N - tile0, max=128)
    c = n - tile0
    k = torch.arange(K)
    cover = (k[None, :] % nc[:, None]) == c[:, None]
    ncover = cover.sum(1)
    assert int(ncover.max()) <= 8, "K too deep for this tile width: more than 8 covering entries in a row"
    want = 8 + (n * 7 + seed) % 5
    score = torch.rand(N, K, generator=g)
    score[cover] = -1.0
    rank = score.argsort(1, descending=True).argsort(1)
    mask = cover | (rank < (want - ncover)[:, None])
    sign = torch.randint(0, 2, (N, K), generator=g) * 2.0 - 1.0
    return torch.where(mask, sign, torch.zeros(()))


def routed_int_case(M, K, N, seed, with_res=True):
    """(a, w, b, res): integer a in [-7, 7], routed_weights, integer bias in [-8, 8] and residual in [-32, 32] (or None).  Every value,
    intermediate and output is an integer of magnitude at most 12 x 7 + 8 + 32 = 124 <= 256: bf16, fp16, f16x2 and fp32 all hold them
    exactly and fp32 sums them exactly in any order, so a kernel's output must EQUAL gemm_ref.  (tests/test_gemm_refs_cpu.py checks the
    magnitudes, the coverage of k and that no two rows of a and no two rows of w are equal.)"""
    g = _gen(seed + 1)
    a = torch.randint(-7, 8, (M, K), generator=g).float()
    w = routed_weights(N, K, seed)
    b = torch.randint(-8, 9, (N,), generator=g).float()
    res = torch.randint(-32, 33, (M, N), generator=g).float() if with_res else None
    return a, w, b, res


def routed_conv_case(n_img, C, H, W, Co, ks, seed):
    """(x [n, C, H, W], w [Co, C, ks, ks], b) for the convolution hooks: the same integers, the weights routed in the kernels' K order
    (tap, channel).  No residual (neither the strided 1x1 mode nor the 3x3 mode of the ring takes one)."""
    g = _gen(seed + 1)
    x = torch.randint(-7, 8, (n_img, C, H, W), generator=g).float()
    wg = routed_weights(Co, ks * ks * C, seed)
    w = wg.reshape(Co, ks, ks, C).permute(0, 3, 1, 2).contiguous()
    b = torch.randint(-8, 9, (Co,), generator=g).float()
    return x, w, b


def conv_ref(x, w, b, stride, act):
    ks = w.shape[-1]
    return _act64(F.conv2d(x.double(), w.double(), b.double(), stride, ks // 2), act)


ROW_KINDS = ("randn", "cancel", "small", "outlier")


def value_rows(M, K, dt, seed):
    """[M, K] rows rounded to `dt`, row m of kind ROW_KINDS[m % 4]: Gaussian; cancelling -- second half = -(first half) + 2^-6 Gaussian,
    scaled by 8, against weights whose two halves are equal (value_case): sum a w is of order 0.1 while sum |a| |w| is of order 50 --;
    Gaussian times 2^-10 (the lo halves of f16x2 are fp16 subnormals); Gaussian with one entry of 100."""
    g = _gen(seed)
    a = torch.randn(M, K, generator=g)
    noise = torch.randn(M, K // 2, generator=g) * 2.0 ** -6
    for m in range(M):
        kind = ROW_KINDS[m % 4]
        if kind == "cancel":
            a[m, K // 2:] = -a[m, :K // 2] + noise[m]
            a[m] *= 8.0
        elif kind == "small":
            a[m] *= 2.0 ** -10
        elif kind == "outlier":
            a[m, (7 * m) % K] = 100.0
    return round_to(a, dt)


def value_case(M, K, N, dt, out_f32, seed):
    """(a, w, b, res): value_rows; w = [w1 | w1] with w1 Gaussian / sqrt(K), rounded to `dt`; b an even sweep of [-12, 12] over the columns
    (the pre-activations of the Gaussian rows are the sweep plus N(0, 1): GELU's negative tail, its minimum, zero and its identity band);
    a Gaussian residual rounded to the output type."""
    g = _gen(seed + 9)
    w1 = torch.randn(N, K // 2, generator=g) / K ** 0.5
    w = round_to(torch.cat([w1, w1], 1), dt)
    b = torch.linspace(-12.0, 12.0, N)
    res = round_to(torch.randn(M, N, generator=g), out_type(dt, out_f32))
    return value_rows(M, K, dt, seed), w, b, res


def periodic_case(K, N, dt, out_f32, seed):
    """One period (PERIOD = 97 rows) of value_case: the GPU file repeats a and res down M, so that row m of any tile must be bit-equal to row
    m % 97 of the first."""
    return value_case(PERIOD, K, N, dt, out_f32, seed)


# ------------------------------------------------------------------------------------------------ builds and shapes
BUILDS = {          # name -> (BM, BN, SPS)
    "128x128": (128, 128, 2), "256x128": (256, 128, 1), "mid256": (256, 128, 2), "256x64": (256, 64, 2),
}
WIDE_N = 4096       # 32 column tiles: big_m (cdiv(M, 256) N / 128 >= 192) from M = 1281 rows up, on any device of 32 CUs or more


def build_variants(dt):
    """(build, out_f32) pairs that exist for `dt`: fp32 has the 128-row build alone; f16x2 also the 256-row one, both with fp32-layout
    stores (F32O) whether the output is raw fp32 or packed; the 16-bit types have all four, the 128- and 256 x 128-row ones with 16-bit and
    with fp32 output, mid256 and 256x64 with 16-bit output only."""
    if dt == "f32":
        return [("128x128", 1)]
    if dt == "f16x2":
        return [("128x128", 0), ("128x128", 1), ("256x128", 0), ("256x128", 1)]
    return [("128x128", 0), ("128x128", 1), ("256x128", 0), ("256x128", 1), ("mid256", 0), ("256x64", 0)]


def build_nks(build):
    return {"128x128": (1,), "256x128": (4, 5, 6), "mid256": (2, 3), "256x64": (1, 4)}[build]


def expect(build, dt, out_f32):
    """(BM, BN, SPS, F32O) of ocrvi_test_ring_plan."""
    bm, bn, sps = BUILDS[build]
    return bm, bn, sps, 1 if (out_f32 or dt in ("f32", "f16x2")) else 0


def build_shape(build, nk, dt):
    """(M, K, N) of the smallest launch on `build`: ragged M, three 128-row tiles or six 256-row tiles of WIDE_N columns (big_m), or three
    tiles of the 64-column build."""
    K = nk * bke(dt)
    if build == "128x128":
        return 300, K, 128
    if build == "256x64":
        return 600, K, 64
    return 1499, K, WIDE_N


def walk(mtiles, lanes):
    """(row-tile lanes, fewest, most row tiles per workgroup) of the launcher's grid rule: gm = cdiv(mtiles, cdiv(mtiles, min(mtiles, lanes)))."""
    gm = min(mtiles, max(1, lanes))
    gm = -(-mtiles // -(-mtiles // gm))
    return gm, mtiles // gm, -(-mtiles // gm)


def later_shape(build, dt, n_cu, t):
    """(M, K, N, gm, tiles_min, tiles_max) of a launch on `build` whose workgroups walk t - 1 and t row tiles (an odd and an even count in one
    launch), M ragged.  The 128-row build runs at one K-step (with more, a 16-bit or f16x2 GEMM of this many tiles moves to 256 rows).
    A big_m build needs at least 192 tiles, i.e. 192 / n_cu per workgroup: where t - 1 and t cannot be had (a small device), the smallest
    launch with two different counts is taken and named."""
    bm, bn, _ = BUILDS[build]
    nk = {"128x128": 1, "256x128": 4, "mid256": 2, "256x64": 1}[build]     # (256x64 has n_cu row-tile lanes: a long, thin launch)
    N = 64 if build == "256x64" else WIDE_N
    lanes = max(1, n_cu // (N // bn))
    need = 6 if build in ("256x128", "mid256") else 1                 # mtiles for big_m at WIDE_N
    first = None
    for mt in range(need, max(need, lanes * t) + 2 * lanes + 2):
        gm, lo, hi = walk(mt, lanes)
        if lo != hi and first is None:
            first = mt
        if (lo, hi) == (t - 1, t):
            first = mt
            break
    gm, lo, hi = walk(first, lanes)
    return bm * first - 41, nk * bke(dt), N, gm, lo, hi


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_ring_gemm.py
DT_CODE = {"f32": 0, "bf16": 1, "f16": 2, "f16x2": 3}
CONV_ROUTED = (           # n_img, C, H, W, Co, ks, stride, build: the ring's strided 1x1 mode (all types) and its 3x3 mode (16-bit types)
    (3, 128, 37, 45, 256, 1, (2, 2), "128x128"),
    (2, 64, 50, 64, 128, 1, (2, 1), "128x128"),
    (2, 64, 91, 91, 128, 3, (1, 1), "256x128"),       # 16562 rows: just above the 16384 the test session dispatches the 3x3 mode from
)


def routing_cases(dt):
    """(M, K, N, out_f32, res_post or None for no residual, act): N = 128, N = 232 (N tail, fp32 output and residual), N = 64 (the 256x64
    build, 16-bit types), each plain / residual before / residual after the activation, ACT none and ReLU; fp32 output at N = 128."""
    shapes = [(300, 256, 128, 0), (300, 256, 232, 1)] + ([(600, 256, 64, 0)] if dt in ("bf16", "f16") else [])
    cases = [(M, K, N, of, rp, act) for (M, K, N, of) in shapes for rp in (None, 0, 1) for act in (ACT_NONE, ACT_RELU)]
    return cases + [(300, 256, 128, 1, rp, ACT_RELU) for rp in (0, 1)]


def value_cases(dt):
    """(M, K, N, out_f32, res_post or None, act): all three activations, without a residual and with one in both orders."""
    combos = [(rp, act) for act in (ACT_NONE, ACT_RELU, ACT_GELU) for rp in (None, 0, 1)]
    return [(200, 128, 232, i % 2, rp, act) for i, (rp, act) in enumerate(combos)]


def tail_cases(dt):
    """(nk, K, N, out_f32, res_post or None, act) for every M of tail_M: one to four K-steps; N = 128 with a 16-bit (T) output and a residual
    under a ReLU, N = 232 with fp32 output.  M <= 128 at nk = 1 is a launch of one step."""
    return [(nk, nk * bke(dt), N, *((0, 0, ACT_RELU) if N == 128 else (1, None, ACT_NONE))) for nk in (1, 2, 3, 4) for N in (128, 232)]


def tail_case(dt, nk, N, out_f32):
    return value_case(max(tail_M), nk * bke(dt), N, dt, out_f32, 40 + nk)


def plan_of(lib, dt, amode, M, K, N, out_f32, has_res, n_cu):
    """ocrvi_test_ring_plan through the loaded library `lib`: (ring?, BM, BN, SPS, F32O, grid, fewest, most tiles per workgroup)."""
    import ctypes
    plan = (ctypes.c_int32 * 8)()
    rc = lib.ocrvi_test_ring_plan(DT_CODE[dt], amode, M, K, N, int(out_f32), int(has_res), n_cu, plan)
    assert rc == 0, rc
    return tuple(plan)
