"""The recogniser's 3x3 convolutions that do not run on the ring GEMM or on conv3_halo -- LocalMixing's grouped pair (32 channels per
group: csrc/gconv32.h in the 16-bit types, conv_gemm_kernel<T, AM_CONV3, 128, 32, 4, 1> otherwise), PatchMerging at stride (2, 1) and
stem2 at stride 2 (conv_gemm's 128 x 128 tile) -- in plain float64, with the per-element bound of tests/gemm_refs.py applied group by group
to the im2col matrix, an fp32 emulation of either kernel's order of operations with deliberate errors, and the inputs and shapes of
tests/test_gpu_grouped_conv.py.  tests/test_conv_refs_cpu.py shows on the CPU that the emulation stays inside the bound on every case the
GPU file runs, that the wrong kernels leave it, and -- through ocrvi_test_gconv_plan, which touches no device -- that every shape takes the
kernel and the tiling the GPU file names for 256, 304 and 64 compute units.  No GPU: torch and numpy only.

Layouts: x [n, C, H, W], w [Co, C / groups, 3, 3], b [Co], res [n, Co, Ho, Wo] (what the hooks take); references, bounds and emulations
are "rows": [n Ho Wo, Co], NHWC order.

    out = act(conv(x) + b (+ res))        res_post = 0
    out = act(conv(x) + b) + res          res_post = 1 (LocalMixing: x + gelu(bn(conv(..))), svtrv2.py:57-63,98)
"""
import torch
import torch.nn.functional as F

import gemm_refs as G
from aux_refs import round_to
from gemm_refs import ACT_GELU, ACT_NONE, ACT_RELU, DTS, err_ratio, out_type       # (the test files use them through this module)
from mlp_refs import _mfma_chain, gelu_erf32

GC_TH, GC_NBX = 4, 5             # csrc/gconv32.h


def out_hw(H, W, stride):
    return (H - 1) // stride[0] + 1, (W - 1) // stride[1] + 1


def rows_of(t):
    """[n, Co, Ho, Wo] -> [n Ho Wo, Co]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def im2col(x, stride, pad_mode="zeros"):
    """[n Ho Wo, 9, C]: the 3x3 (pad 1) patches of x in the kernels' K order (tap = 3 r + s, channel).  pad_mode "replicate" and "images"
    are two of the wrong kernels (emulate)."""
    n, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, stride)
    if pad_mode == "replicate":
        xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    else:
        xp = F.pad(x, (1, 1, 1, 1))
        if pad_mode == "images":                # the row above image i is the last row of image i - 1, the row below it the first of i + 1
            xp[1:, :, 0, 1:-1] = x[:-1, :, H - 1, :]
            xp[:-1, :, H + 1, 1:-1] = x[1:, :, 0, :]
    taps = [xp[:, :, r:r + (Ho - 1) * stride[0] + 1:stride[0], s:s + (Wo - 1) * stride[1] + 1:stride[1]] for r in range(3) for s in range(3)]
    return torch.stack([rows_of(t) for t in taps], 1)


def group_gemms(x, w, groups, stride, pad_mode="zeros"):
    """[(A_g [M, 9 Cg], W_g [Ng, 9 Cg])] per group, K in (tap, channel) order."""
    cols = im2col(x, stride, pad_mode)
    Co, Cg = w.shape[0], w.shape[1]
    Ng = Co // groups
    return [(cols[:, :, g * Cg:(g + 1) * Cg].reshape(cols.shape[0], 9 * Cg), w[g * Ng:(g + 1) * Ng].permute(0, 2, 3, 1).reshape(Ng, 9 * Cg))
            for g in range(groups)]


def _per_group(fn, x, w, b, res, groups, stride):
    Ng = w.shape[0] // groups
    rr = None if res is None else rows_of(res)
    return torch.cat([fn(a, wg, b[g * Ng:(g + 1) * Ng], None if rr is None else rr[:, g * Ng:(g + 1) * Ng])
                      for g, (a, wg) in enumerate(group_gemms(x, w, groups, stride))], 1)


def conv_ref(x, w, b, res, stride, groups, act, res_post):
    """The convolution in float64, rows."""
    return _per_group(lambda a, wg, bg, rg: G.gemm_ref(a, wg, bg, rg, act, res_post), x.double(), w.double(), b.double(), res, groups, stride)


def conv_bound(x, w, b, res, stride, groups, act, res_post, dt, out_f32):
    """gemm_refs.gemm_bound on every group's im2col matrix: its derivation holds for a chain of MFMAs in any order (nine of 32 channels in
    gconv32, five 64-element K-steps or nine 32-element ones in conv_gemm) and charges the bias, the residual, the activation and the
    output rounding once each, as both kernels' epilogues apply them.  x, w must be exact in `dt`, res in the output type."""
    return _per_group(lambda a, wg, bg, rg: G.gemm_bound(a, wg, bg, rg, act, res_post, dt, out_f32), x, w, b, res, groups, stride)


# ------------------------------------------------------------------------------------------------ launch plans (csrc/gconv32.h, conv_launch.h)
def cdiv(a, b):
    return -(-a // b)


def gconv32_plan(n, H, W, groups, n_cu):
    """(th, nbx, bands_y, bands_x, grid.x, fewest, most tiles per workgroup) of gconv32_plan in csrc/gconv32.h."""
    nbx = min(GC_NBX, cdiv(W, 16))
    th = 4 if H % 4 == 0 else (3 if H % 3 == 0 else (H if H < 4 else 4))
    bands_x, bands_y = cdiv(W, 16 * nbx), cdiv(H, th)
    ntile = n * bands_y * bands_x
    grid = cdiv(ntile, cdiv(ntile, max(1, 2 * n_cu // groups)))
    return th, nbx, bands_y, bands_x, grid, ntile // grid, cdiv(ntile, grid)


def takes_gconv32(dt, C, Co, stride, groups, out_f32, has_res, gconv32_on=True):
    """gconv32_eligible for the hook's calls: a 16-bit type, 32 channels per group in and out, stride 1, and a residual only as the fp32
    stream beside an fp32 output."""
    return (gconv32_on and dt in ("bf16", "f16") and groups >= 2 and C // groups == 32 and Co // groups == 32 and tuple(stride) == (1, 1)
            and (not has_res or bool(out_f32)))


def expect_plan(dt, n, C, H, W, Co, stride, groups, out_f32, has_res, n_cu, gconv32_on=True):
    """What ocrvi_test_gconv_plan must report (12 integers; include/ocrvi.h)."""
    bke = G.bke(dt)
    nk = cdiv(9 * (C // groups), bke)
    if takes_gconv32(dt, C, Co, stride, groups, out_f32, has_res, gconv32_on):
        return (1, 0, 0, *gconv32_plan(n, H, W, groups, n_cu), groups, nk)
    Ng = Co // groups
    bn = 128 if Ng > 64 else (64 if Ng > 32 else 32)
    Ho, Wo = out_hw(H, W, stride)
    return (0, 128, bn, 0, 0, 0, 0, cdiv(n * Ho * Wo, 128) * (cdiv(Ng, bn)), 1, 1, groups, nk)


def plan_of(lib, dt, n, C, H, W, Co, stride, groups, out_f32, has_res, n_cu):
    """ocrvi_test_gconv_plan through the loaded library `lib`."""
    import ctypes
    plan = (ctypes.c_int32 * 12)()
    rc = lib.ocrvi_test_gconv_plan(G.DT_CODE[dt], n, C, H, W, Co, stride[0], stride[1], groups, int(out_f32), int(has_res), n_cu, plan)
    assert rc == 0, rc
    return tuple(plan)


def magic_first_failure(hw, limit=1 << 16):
    """The first pix at which (pix * (65536 // hw + 1)) >> 16 != pix // hw (gconv32's halo-index multiplication), or None below `limit`."""
    m = 65536 // hw + 1
    for pix in range(limit):
        if (pix * m) >> 16 != pix // hw:
            return pix
    return None


# ------------------------------------------------------------------------------------------------ fp32 emulation of the two kernels
MUTANTS = ("taps (r, s) exchanged", "last tap dropped", "x of the next group", "output-channel permutation left out",
           "bias of the next 4-channel block", "res_post flipped", "halo clamped, not zeroed", "halo row of the neighbouring image",
           "ragged band written from the wrong pixel", "tenth tap not masked", "next tile's halo not staged")


def _conv_gemm_k_order(K, dt):
    """The order in which conv_gemm feeds k to its MFMAs: a 16-bit K-step of 64 elements is two MFMAs over the even and over the odd
    8-element chunks (lane group g holds chunks 2 g and 2 g + 1); a 4-byte K-step is 32 consecutive elements."""
    k = torch.arange(K)
    if dt in ("f32", "f16x2"):
        return k
    return k.reshape(K // 64, 4, 2, 8).permute(0, 2, 1, 3).reshape(K)


def emulate(x, w, b, res, stride, groups, act, res_post, dt, out_f32, mut=None, n_cu=256, gconv32_on=True):
    """The kernel that (dt, shape) takes, in float32, rows.  Both: mlp_refs._mfma_chain over K in (tap, channel) order -- gconv32: one MFMA
    per tap (K = 32); conv_gemm: K padded with zeros to whole 128-byte K-steps, the 16-bit K-step's two MFMAs over interleaved chunks
    (_conv_gemm_k_order), f16x2's three partial products on scaled, split weights -- then the bias, the residual before or after the
    activation and the rounding to the output type, in fp32.  Not followed: the order inside an MFMA, fp32's individual product
    roundings, fmas, and that conv_gemm's 32-column f16x2 build also adds the lo lo product.
    `mut`: one of MUTANTS, a deliberately wrong kernel; a mutant that names a feature the kernel taken does not have is the identity."""
    assert mut is None or mut in MUTANTS, mut
    x, w, b = x.float(), w.float().clone(), b.float().clone()
    n, C, H, W = x.shape
    Co, Cg = w.shape[0], w.shape[1]
    Ng = Co // groups
    Ho, Wo = out_hw(H, W, stride)
    ot = out_type(dt, out_f32)
    gc = takes_gconv32(dt, C, Co, stride, groups, out_f32, res is not None, gconv32_on)
    if mut == "x of the next group":
        x = torch.roll(x, -Cg, 1)
    pad_mode = {"halo clamped, not zeroed": "replicate", "halo row of the neighbouring image": "images"}.get(mut, "zeros")
    outs = []
    for g, (a, wg) in enumerate(group_gemms(x, w, groups, stride, pad_mode)):
        M = a.shape[0]
        a = a.reshape(M, 9, Cg).clone()
        if mut == "taps (r, s) exchanged":
            a = a[:, [3 * (t % 3) + t // 3 for t in range(9)]]
        elif mut == "last tap dropped":
            a[:, 8] = 0
        a = a.reshape(M, 9 * Cg)
        if not gc:                                 # conv_gemm: whole K-steps
            Kp = cdiv(9 * Cg, G.bke(dt)) * G.bke(dt)
            tail = torch.zeros(M, Kp - 9 * Cg)
            if mut == "tenth tap not masked" and Kp > 9 * Cg:     # "tap 9" = (r, s) = (3, 0): the pixel two rows below the window's first
                xg = F.pad(x[:, g * Cg:(g + 1) * Cg], (1, 1, 1, 3))
                t9 = xg[:, :, 3:3 + (Ho - 1) * stride[0] + 1:stride[0], 0:(Wo - 1) * stride[1] + 1:stride[1]]
                tail = rows_of(t9)[:, :Kp - 9 * Cg].contiguous()
            a = torch.cat([a, tail], 1)
            wg = torch.cat([wg, torch.zeros(Ng, Kp - 9 * Cg)], 1)
            order = _conv_gemm_k_order(Kp, dt)
            a, wg = a[:, order], wg[:, order]
        outs.append(_mfma_chain(a, wg, dt))
    acc = torch.cat(outs, 1)
    bv = b
    if mut == "bias of the next 4-channel block":
        bv = torch.roll(b, -4)
    if mut == "output-channel permutation left out" and gc and not out_f32:
        # MFMA row lr = 4 g4 + e of N-block nb holds channel 16 nb + lr of the group; the epilogue stores it (and adds the bias) as channel
        # 8 g4 + 4 nb + e
        pos = torch.arange(32)
        g4, nb, e = pos // 8, (pos // 4) % 2, pos % 4
        src = 16 * nb + 4 * g4 + e
        acc = acc.reshape(-1, groups, 32)[:, :, src].reshape(-1, Co)
    v = acc + bv
    rr = None if res is None else rows_of(res.float())
    post = bool(res_post) != (mut == "res_post flipped")
    fact = {ACT_NONE: lambda t: t, ACT_RELU: lambda t: torch.clamp(t, min=0.0), ACT_GELU: gelu_erf32}[act]
    if rr is not None and not post:
        v = v + rr
    v = fact(v)
    if rr is not None and post:
        v = v + rr
    out = round_to(v, ot)
    if gc and mut in ("ragged band written from the wrong pixel", "next tile's halo not staged"):
        th, nbx, by, bx, grid, _, _ = gconv32_plan(n, H, W, groups, n_cu)
        o4 = out.reshape(n, H, W, Co).clone()
        if mut == "ragged band written from the wrong pixel":
            if H % th:
                o4[:, H - 1] = o4[:, H - 2].clone()
            if W % (16 * nbx):
                o4[:, :, W - 1] = o4[:, :, W - 2].clone()
        else:        # a workgroup's second and later tiles are computed from the halo of its tile before: they repeat that tile's output
            good = out.reshape(n, H, W, Co)
            box = lambda t: (t // (by * bx), (t // bx) % by * th, t % bx * 16 * nbx)
            for t in range(grid, n * by * bx):
                (i1, y1, x1), (i0, y0, x0) = box(t), box(t - grid)
                hh, ww = min(th, H - y1, H - y0), min(16 * nbx, W - x1, W - x0)
                o4[i1, y1:y1 + hh, x1:x1 + ww] = good[i0, y0:y0 + hh, x0:x0 + ww]
        out = o4.reshape(-1, Co)
    return out


# ------------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def routed_conv_weights(Co, Cg, groups, seed):
    """w [Co, Cg, 3, 3]: 9 to 12 entries of +-1 per output channel, all else zero.  Channel i of a group uses, at tap j, input channel
    (i + m j) mod Cg -- one weight at each of the nine taps, and, a group having at least Cg output channels, every (tap, channel)
    position of the group is used by some channel --, with an odd step m of its own for every group (and for every Cg channels of a wider
    group), so that no two channels of the layer have the same nine positions; the rest of its entries and all signs are seeded."""
    g = _gen(seed)
    Ng = Co // groups
    assert Ng >= Cg and Ng % Cg == 0 and 2 * (Co // Cg) + 5 < Cg
    i = torch.arange(Co) % Ng
    m = 5 + 2 * (torch.arange(Co) // Cg)
    K = 9 * Cg
    k = torch.arange(K)
    cover = (k[None, :] % Cg) == (i[:, None] + m[:, None] * (k[None, :] // Cg)) % Cg
    want = 9 + (torch.arange(Co) * 7 + seed) % 4
    score = torch.rand(Co, K, generator=g)
    score[cover] = -1.0
    rank = score.argsort(1, descending=True).argsort(1)
    mask = cover | (rank < (want - 9)[:, None])
    sign = torch.randint(0, 2, (Co, K), generator=g) * 2.0 - 1.0
    wk = torch.where(mask, sign, torch.zeros(()))
    return wk.reshape(Co, 3, 3, Cg).permute(0, 3, 1, 2).contiguous()


def routed_case(n, C, H, W, Co, stride, groups, seed, with_res=True):
    """(x, w, b, res): integer x in [-7, 7], routed_conv_weights, integer bias in [-8, 8] and residual in [-32, 32] (or None).  Every value,
    intermediate and output is an integer of magnitude at most 12 x 7 + 8 + 32 = 124: bf16, fp16, f16x2 and fp32 all hold them exactly
    and fp32 sums them exactly in any order, so a kernel's output must EQUAL conv_ref (with no activation or ReLU)."""
    g = _gen(seed + 1)
    Ho, Wo = out_hw(H, W, stride)
    x = torch.randint(-7, 8, (n, C, H, W), generator=g).float()
    w = routed_conv_weights(Co, C // groups, groups, seed)
    b = torch.randint(-8, 9, (Co,), generator=g).float()
    res = torch.randint(-32, 33, (n, Co, Ho, Wo), generator=g).float() if with_res else None
    return x, w, b, res


ROW_KINDS = G.ROW_KINDS


def value_case(n, C, H, W, Co, stride, groups, dt, out_f32, seed):
    """(x, w, b, res) rounded so that the hook's casts are exact.  Image row y is of kind ROW_KINDS[y % 4], as gemm_refs.value_rows:
    Gaussian; cancelling -- in every group the second half of the channels = -(the first half) + 2^-6 Gaussian, times 8, against weights
    whose two halves are equal: at every tap the products cancel to order 0.1 under a sum of magnitudes of order 10 --; Gaussian times
    2^-10; Gaussian with, per group, one entry of 100 in the row.  A 3x3 window sees three kinds at once.  w is Gaussian / sqrt(9 Cg); the
    bias sweeps [-12, 12] evenly over the output channels (GELU's negative tail, its minimum, zero and its identity band); the residual
    is Gaussian, rounded to the output type."""
    g = _gen(seed)
    Cg, h2 = C // groups, C // groups // 2
    Ho, Wo = out_hw(H, W, stride)
    x = torch.randn(n, C, H, W, generator=g)
    noise = torch.randn(n, C, H, W, generator=g) * 2.0 ** -6
    xg = x.reshape(n, groups, Cg, H, W)
    ng = noise.reshape(n, groups, Cg, H, W)
    for y in range(H):
        kind = ROW_KINDS[y % 4]
        if kind == "cancel":
            xg[:, :, h2:, y] = -xg[:, :, :h2, y] + ng[:, :, h2:, y]
            xg[:, :, :, y] *= 8.0
        elif kind == "small":
            xg[:, :, :, y] *= 2.0 ** -10
        elif kind == "outlier":
            for gi in range(groups):
                xg[:, gi, (5 * y) % Cg, y, (7 * y + 3 * gi) % W] = 100.0
    w1 = torch.randn(Co, h2, 3, 3, generator=g) / (9 * Cg) ** 0.5
    w = round_to(torch.cat([w1, w1], 1), dt)
    b = torch.linspace(-12.0, 12.0, Co)
    res = round_to(torch.randn(n, Co, Ho, Wo, generator=g), out_type(dt, out_f32))
    return round_to(x, dt), w, b, res


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_grouped_conv.py
# n, C, H, W -> (th, nbx, bands_y, bands_x) of gconv32, whatever the device
ROUTE_SHAPES = (
    ((1, 128, 4, 16), (4, 1, 1, 1)),      # one tile
    ((1, 128, 1, 5), (1, 1, 1, 1)),       # th = 1, W < 16: one fragment, waves 1..3 idle
    ((1, 128, 2, 33), (2, 3, 1, 1)),      # th = 2, nbx = 3, the last block 1 pixel wide
    ((2, 128, 6, 80), (3, 5, 2, 1)),      # th = 3, two full-width bands, image border
    ((1, 128, 5, 81), (4, 5, 2, 2)),      # th = 4, the last band 1 row, the second column band 1 pixel wide
    ((1, 128, 7, 100), (4, 5, 2, 2)),     # ragged in both directions
    ((2, 128, 8, 160), (4, 5, 2, 2)),     # 2 x 2 full bands
    ((1, 256, 4, 16), (4, 1, 1, 1)),      # 8 groups
    ((1, 384, 4, 16), (4, 1, 1, 1)),      # 12 groups
)
# out_f32, res_post (None: no residual), act.  In the 16-bit types: the 16-bit-output build, the fp32-output build without a residual, with
# it after and before the ReLU, conv_gemm with a 16-bit residual (gconv32 takes none), and a residual with no activation.  In the 4-byte
# types all are conv_gemm; the last is its residual-in-the-store-phase path.
ROUTE_VARIANTS = ((0, None, ACT_NONE), (1, None, ACT_RELU), (1, 1, ACT_RELU), (1, 0, ACT_RELU), (0, 0, ACT_RELU), (1, 1, ACT_NONE))
VALUE_SHAPES = ((2, 128, 6, 80), (1, 128, 7, 100))
VALUE_VARIANTS = tuple((i % 2, None, act) for i, act in enumerate((ACT_NONE, ACT_RELU, ACT_GELU))) + \
    tuple((1, rp, act) for act in (ACT_NONE, ACT_RELU, ACT_GELU) for rp in (0, 1)) + ((0, 0, ACT_RELU), (0, 1, ACT_GELU), (0, None, ACT_GELU))
IN_PLACE_SHAPE = (2, 128, 6, 80)
# n, C, H, W, Co, stride, (out_f32, act) for the value family; routing runs them with no activation and ReLU (GELU of an integer is none)
STRIDED = (
    (2, 128, 8, 20, 256, (2, 1), (1, ACT_NONE)),        # PatchMerging: fp32 output from a 16-bit input, no activation
    (1, 128, 6, 37, 256, (2, 1), (1, ACT_NONE)),
    (1, 64, 9, 13, 128, (2, 2), (1, ACT_GELU)),         # stem2: GELU, fp32 output
    (2, 64, 12, 20, 128, (2, 2), (1, ACT_GELU)),
)
INDEP_SHAPE = (2, 128, 6, 80)


def launches(dt):
    """Every (n, C, H, W, Co, stride, groups, out_f32, has_res) the GPU file launches in type `dt` apart from the later-tiles family (whose
    n depends on the device: later_shape)."""
    out = []
    for (n, C, H, W), _ in ROUTE_SHAPES:
        out += [(n, C, H, W, C, (1, 1), C // 32, of, rp is not None) for (of, rp, act) in ROUTE_VARIANTS]
    for (n, C, H, W) in VALUE_SHAPES:
        out += [(n, C, H, W, C, (1, 1), C // 32, of, rp is not None) for (of, rp, act) in VALUE_VARIANTS]
    for (n, C, H, W) in (IN_PLACE_SHAPE, INDEP_SHAPE):
        out += [(n, C, H, W, C, (1, 1), C // 32, 1, True), (n, C, H, W, C, (1, 1), C // 32, 0, False)]
    for (n, C, H, W, Co, stride, (of, act)) in STRIDED:
        out += [(n, C, H, W, Co, stride, 1, of, False), (n, C, H, W, Co, stride, 1, 0, False)]
    return out


LATER_HW = (9, 16)            # th = 3: three tiles per image, each with other contents
LATER_C = 384                 # 12 groups


def later_shape(n_cu, t):
    """(n, C, H, W, grid.x, fewest, most) of a gconv32 launch on identical 9 x 16 images of 384 channels whose workgroups walk t - 1 and t
    tiles, with grid.x no multiple of 3, so that a workgroup's consecutive tiles lie at different heights of the image.  Where no n gives
    (t - 1, t) the first launch with two different counts is taken."""
    H, W = LATER_HW
    groups = LATER_C // 32
    first = None
    for n in range(1, 4 * t * max(1, 2 * n_cu // groups)):
        _, _, _, _, grid, lo, hi = gconv32_plan(n, H, W, groups, n_cu)
        if grid % 3 == 0 or lo == hi:
            continue
        if first is None:
            first = n
        if (lo, hi) == (t - 1, t):
            first = n
            break
    _, _, _, _, grid, lo, hi = gconv32_plan(first, H, W, groups, n_cu)
    return first, LATER_C, H, W, grid, lo, hi
