"""The three halo-tile kernels that carry the f16x2 detector -- conv3_halo_kernel (csrc/conv3_halo.h), bneck_tail_kernel (csrc/bneck_tail.h)
and stem_pool_kernel (csrc/stem_pool.hip; with it the two-kernel stem of the other element types) -- in plain float64, with per-element bounds
that are gemm_refs.gemm_bound and nothing else, an fp32 emulation of each kernel's order of operations with deliberate errors (MUTANTS), and
the input families and shapes of tests/test_gpu_conv3_halo_elements.py, test_gpu_bneck_tail_elements.py and test_gpu_stem_pool_elements.py.
tests/test_halo_refs_cpu.py shows on the CPU that the emulations stay inside the bounds (value data) or equal the references (routed and
probe data) on the cases the GPU files launch, that every wrong kernel is caught by some family, and -- through ocrvi_test_halo_plan, which
touches no device -- that every shape takes the kernel and tiling named for 256, 304 and 64 compute units.  No GPU: torch and numpy only.

Layouts: x [n, C, H, W], w [Co, C, 3, 3] (stem: [64, 3, 7, 7]), b [Co]: what the hooks take.  References, bounds and emulations are "rows":
[pixels, channels] in NHWC order.

    conv3_halo   out = act(conv3x3(x) + b)                       act none / ReLU
    bneck_tail   t2 = relu(conv3x3(t1; w2) + b2); y = relu(t2 w3^T + b3 + identity); t1' = relu(y w1^T + b1)
    stem         out = maxpool3x3s2p1(relu(conv7x7s2p3(x) + b))   pool padding -inf

Families (the GPU files' docstrings say which shapes run which):
  routed   integers: x in [-7, 7], weights 0 / +-1 from routed_dense (every k position used inside every column tile, no two output channels
           alike), integer bias, integer identity >= 0.  Every intermediate is an integer fp32 and f16x2 hold exactly: output == reference.
  probe a  impulses of +- a power of two, at most one per window, the impulse channel running over all input channels (in as many launches
           as that takes); full-width Gaussian weights, no bias: every output is one weight times a power of two, exactly.
  probe b  one-hot weights (a power of two at the channel's own (tap, channel)), full-width value data: the output is a shifted copy of x.
  probe c  bneck_tail pass-through: conv2 the centre-tap identity, conv3 copies t2 into y's first 128 channels and leaves the identity alone
           in the others, conv1 selects 64 channels of y per launch.
  rounding bneck_tail: t2 = 512.25 + m 2^-14 (24 bits: exact in fp32; its lo half would need 13) and y = t2[2 i] - t2[2 i + 1]: the reference is the chain with t2
           ROUNDED to f16x2 as the kernel's contract says (the unfused path stores it); everything else is exact.  This is the one family
           whose reference is not the plain float64 chain: no comparison with that chain can see whether t2 was rounded.
  value    conv_refs.value_case: Gaussian, cancelling, 2^-10 and outlier image rows; Gaussian weights with two equal halves; bias sweeping
           [-12, 12]: every element within its bound.
(independence and later tiles are built in the GPU files from these.)

Shapes that were replaced: none.  bneck_tail runs probes a and b on its conv2 (its own copy of conv3_halo's unit loop) with the tail
passing through as in probe c.
"""
import torch
import torch.nn.functional as F

import conv_refs as R
import gemm_refs as G
from aux_refs import round_to
from conv_refs import im2col, out_hw, rows_of
from gemm_refs import ACT_NONE, ACT_RELU, ROW_KINDS, err_ratio, gemm_bound, gemm_ref
from mlp_refs import _mfma_chain, _x2_scale

DT = "f16x2"
TILE = 16                                  # conv3_halo / bneck_tail: 16 x 16 output pixels
SP_PH, SP_PW = 8, 7                        # stem_pool: 8 x 7 pooled pixels


def cdiv(a, b):
    return -(-a // b)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def persistent_grid(ntile, slots):
    """common.h"""
    s = max(slots, 1)
    return cdiv(ntile, cdiv(ntile, min(ntile, s)))


# ------------------------------------------------------------------------------------------------ launch plans
def np_of(Co):
    """pack_conv's padded column count."""
    bn = 128 if Co > 64 else (64 if Co > 32 else 32)
    return cdiv(Co, bn) * bn


def halo_plan(n, H, W, Co, n_cu):
    """(NC, column tiles, tiles_x, tiles_y, grid, fewest, most tiles per workgroup) of conv3_halo_plan in csrc/conv3_halo.h."""
    Np = np_of(Co)
    nc = 64 if Np == 64 else 128
    nct = Np // nc
    tx, ty = cdiv(W, TILE), cdiv(H, TILE)
    ntile = n * tx * ty
    gm = persistent_grid(ntile, n_cu // nct)
    return nc, nct, tx, ty, gm * nct, ntile // gm, cdiv(ntile, gm)


def stem_plan(n, H, W, n_cu):
    tx, ty = cdiv(W // 4, SP_PW), cdiv(H // 4, SP_PH)
    total = n * tx * ty
    grid = persistent_grid(total, n_cu)
    return 64, 1, tx, ty, grid, total // grid, cdiv(total, grid)


def expect_plan(kind, n, C, H, W, Co, n_cu):
    """What ocrvi_test_halo_plan must report for a shape of these files (8 integers; include/ocrvi.h)."""
    if kind == 2:
        return (1, *stem_plan(n, H, W, n_cu))
    return (1, *halo_plan(n, H, W, Co if kind == 0 else 64, n_cu))


def plan_of(lib, kind, n, C, H, W, Co, n_cu):
    import ctypes
    plan = (ctypes.c_int32 * 8)()
    rc = lib.ocrvi_test_halo_plan(kind, n, C, H, W, Co, n_cu, plan)
    assert rc == 0, rc
    return tuple(plan)


def later_shape(kind, n_cu, t, Co=64, hw=None):
    """(n, grid, fewest, most) of a launch on n images of 48 x 48 (3 x 3 tiles; the stem: 96 x 84 images, 3 x 3 tiles of pooled pixels) whose
    workgroups walk t - 1 and t tiles -- or, where the equalising grid leaves no such launch (9 n tiles on a grid of cdiv(9 n, 3) workgroups
    is always 3 each), t tiles each -- on a grid that is no multiple of the 9 tiles of an image, so that a workgroup's consecutive tiles lie
    at different places of different images."""
    H, W = hw or ((96, 84) if kind == 2 else (48, 48))
    plan = (lambda n: stem_plan(n, H, W, n_cu)) if kind == 2 else (lambda n: halo_plan(n, H, W, Co, n_cu))
    tpi = plan(1)[2] * plan(1)[3]
    best = None
    for n in range(1, 8 * t * max(1, n_cu // tpi) + 8):
        nct, grid, lo, hi = plan(n)[1], *plan(n)[4:]
        if (grid // nct) % tpi == 0 or hi != t:
            continue
        if lo == t - 1:
            return n, grid, lo, hi
        if best is None:
            best = (n, grid, lo, hi)
    assert best is not None, (kind, n_cu, t)
    return best


# ------------------------------------------------------------------------------------------------ references and bounds
def _act64(y, act):
    return torch.clamp(y, min=0.0) if act == ACT_RELU else y


def wk_of(w):
    """[Co, C, 3, 3] -> [Co, 9 C], K in (tap, channel) order."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv_ref(x, w, b, act):
    """The dense 3x3 (pad 1) with bias and none / ReLU in float64, rows."""
    return rows_of(_act64(F.conv2d(x.double(), w.double(), b.double(), 1, 1), act))


def conv_bound(x, w, b, act):
    """gemm_bound on the im2col matrix, f16x2 with a T output."""
    a = im2col(x, (1, 1))
    return gemm_bound(a.reshape(a.shape[0], -1), wk_of(w), b, None, act, 0, DT, 0)


def bneck_ref(t1, idn, wb, round_t2=False):
    """(t2, y, t1') of the layer1 chain in float64, rows.  round_t2: t2 rounded to f16x2 (the rounding probe's reference)."""
    w2, b2, w3, b3, w1, b1 = wb
    t2 = conv_ref(t1, w2, b2, ACT_RELU)
    if round_t2:
        t2 = round_to(t2.float(), DT).double()
    y = gemm_ref(t2, w3, b3, rows_of(idn), ACT_RELU, 0)
    return t2, y, gemm_ref(y, w1, b1, None, ACT_RELU, 0)


def bneck_bound(t1, idn, wb):
    """(e_t2, e_y, e_t1'): the conv2 bound, then gemm_bound with the stage before as a_err, twice.  The rounding of t2 and of y to f16x2
    is inside the stage's own bound (its T output)."""
    w2, b2, w3, b3, w1, b1 = wb
    t2, y, _ = bneck_ref(t1, idn, wb)
    e2 = conv_bound(t1, w2, b2, ACT_RELU)
    ey = gemm_bound(t2, w3, b3, rows_of(idn), ACT_RELU, 0, DT, 0, a_err=e2)
    return e2, ey, gemm_bound(y, w1, b1, None, ACT_RELU, 0, DT, 0, a_err=ey)


def stem_a8(x):
    """[n CH CW, 8, 8, 4]: per conv pixel the 8 rows x 8 pixels x 4 channels of the zero-padded NHWC4 input from its window's corner (the
    kernel's K-step r is row r: 8 pixels x 4 channels, pixel 7 and channel 3 being the pad slots; row 7 is what a filter row shifted down
    by one would read).  The image sits at (3, 3) of the padded input."""
    n, _, H, W = x.shape
    CH, CW = H // 2, W // 2
    xp = torch.zeros(n, 4, H + 8, W + 8, dtype=x.dtype)
    xp[:, :3, 3:3 + H, 3:3 + W] = x
    rows = [torch.stack([rows_of(xp[:, :, r:r + 2 * CH:2, s:s + 2 * CW:2]) for s in range(8)], 1) for r in range(8)]
    return torch.stack(rows, 1)


def stem_wk(w):
    """[64, 3, 7, 7] -> [64, 7, 8, 4] (pack_conv's AM_ROWS order: filter row, pixel, channel; the pad slots zero)."""
    wk = torch.zeros(w.shape[0], 7, 8, 4, dtype=w.dtype)
    wk[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    return wk


def _pool_rows(v, n, CH, CW):
    """max-pool 3x3 / 2 / pad 1 (-inf padding) of conv rows [n CH CW, 64] -> rows [n CH/2 CW/2, 64]."""
    return rows_of(F.max_pool2d(v.reshape(n, CH, CW, -1).permute(0, 3, 1, 2), 3, 2, 1))


def stem_ref(x, w, b):
    y = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3))
    return rows_of(F.max_pool2d(y, 3, 2, 1))


def stem_bound(x, w, b, dt=DT):
    """The conv bound per conv pixel (gemm_bound for `dt` with a T output), then its maximum over each pool window: max is 1-Lipschitz in
    the sup norm, and rounding to T commutes with max."""
    n, _, H, W = x.shape
    e = gemm_bound(stem_a8(x)[:, :7].reshape(-1, 224), stem_wk(w).reshape(-1, 224), b, None, ACT_RELU, 0, dt, 0)
    return _pool_rows(e, n, H // 2, W // 2)


# ------------------------------------------------------------------------------------------------ fp32 emulations
MUTANTS = (
    "taps (r, s) exchanged", "last tap dropped", "patch stage not switched", "halo clamped, not zeroed", "halo row of the neighbouring image",
    "ragged tile's halo zeroed one pixel early", "second column tile with the first's weights", "second column tile with the first's bias",
    "bias of the next 4-channel block", "activation lo halves dropped", "weight lo halves dropped", "quartet halves exchanged",
    "second tile from the first tile's patch",
    "bneck: conv3 k-slots in natural order", "bneck: identity of group q + 1", "bneck: t2 not rounded", "bneck: y-only fed the full stream",
    "stem: pool padding 0", "stem: halo conv row not recomputed", "stem: filter row r against input row r + 1", "stem: pad slot times a live weight",
)
EQUIVALENT = ("stem: pool padding 0",)      # the pool runs behind a ReLU: every window holds a value >= 0, so 0 and -inf padding give one result


def _chain3(a, w, swap_k=None):
    """mlp_refs._mfma_chain for f16x2 written out on the split operands, so that a mutant can reach the halves: per 32 k the three products
    w_lo a_hi, w_hi a_lo, w_hi a_hi.  swap_k: k-slots whose weight hi and lo halves change places."""
    s = _x2_scale(w)
    w64, a64 = w.double() * s, a.double()
    wH = w64.float().half().double()
    wL = (w64 - wH).float().half().double()
    if swap_k is not None:
        wH, wL = wH.clone(), wL.clone()
        wH[:, swap_k], wL[:, swap_k] = wL[:, swap_k].clone(), wH[:, swap_k].clone()
    aH = a.half().double()
    aL = (a64 - aH).float().half().double()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(0, a.shape[1], 32):
        for wp, ap in ((wL, aH), (wH, aL), (wH, aH)):
            acc = (acc.double() + ap[:, k:k + 32] @ wp[:, k:k + 32].t()).float()
    return (acc.double() / s).float()


def _cb_order(t):
    """[.., 9, C] -> [.., 9 C] in the kernel's K order (channel block of 32, tap, channel)."""
    C = t.shape[-1]
    return t.reshape(*t.shape[:-2], 9, C // 32, 32).transpose(-3, -2).reshape(*t.shape[:-2], 9 * C)


def _drop_lo_w(w):
    s = _x2_scale(w)
    return ((w.double() * s).float().half().double() / s).float()


def _tile_shift(a, n, H, W, gm):
    """Rows [n H W, ...] where tile t >= gm takes the rows of tile t - gm at the same place in the tile (zero where that tile has none)."""
    tx, ty = cdiv(W, TILE), cdiv(H, TILE)
    rest = a.shape[1:]
    full = torch.zeros(n, ty * TILE, tx * TILE, *rest, dtype=a.dtype)
    full[:, :H, :W] = a.reshape(n, H, W, *rest)
    tiles = full.reshape(n, ty, TILE, tx, TILE, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(n * ty * tx, TILE, TILE, *rest)
    moved = tiles.clone()
    moved[gm:] = tiles[:-gm] if gm < tiles.shape[0] else moved[gm:]
    back = moved.reshape(n, ty, tx, TILE, TILE, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(n, ty * TILE, tx * TILE, *rest)
    return back[:, :H, :W].reshape(n * H * W, *rest)


def _conv_acc(x, w, mut, n_cu):
    """conv3_halo's accumulators times wscale: [n H W, Co] fp32 (before the bias), with the mutants of the unit loop."""
    x, w = x.float(), w.float()
    n, C, H, W = x.shape
    Co = w.shape[0]
    pad = {"halo clamped, not zeroed": "replicate", "halo row of the neighbouring image": "images"}.get(mut, "zeros")
    a = im2col(x, (1, 1), pad).clone()                                   # [M, 9, C]
    wk = w.permute(0, 2, 3, 1).reshape(Co, 9, C).clone()
    if mut == "taps (r, s) exchanged":
        a = a[:, [3 * (t % 3) + t // 3 for t in range(9)]]
    elif mut == "last tap dropped":                                       # tap 8 of the last channel block
        a[:, 8, C - 32:] = 0
    elif mut == "patch stage not switched" and C > 32:                    # channel block cb >= 1 reads the stage of cb - 1
        a[:, :, 32:] = a[:, :, :C - 32].clone()
    elif mut == "ragged tile's halo zeroed one pixel early":
        oy = torch.arange(H).repeat_interleave(W).repeat(n)
        ox = torch.arange(W).repeat(H * n)
        for t in range(9):
            iy, ix = oy + t // 3 - 1, ox + t % 3 - 1
            early = ((W % TILE != 0) & (ox >= W // TILE * TILE) & (ix == W - 1)) | ((H % TILE != 0) & (oy >= H // TILE * TILE) & (iy == H - 1))
            a[early, t] = 0
    elif mut == "activation lo halves dropped":
        a = a.half().float()
    elif mut == "weight lo halves dropped":
        wk = _drop_lo_w(wk)
    elif mut == "second column tile with the first's weights" and Co > 128:
        wk[128:] = wk[:Co - 128].clone()
    gm = halo_plan(n, H, W, Co, n_cu)[4] // halo_plan(n, H, W, Co, n_cu)[1]
    if mut == "second tile from the first tile's patch" or (mut == "patch stage not switched" and C == 32):
        a = _tile_shift(a, n, H, W, gm)                                   # (one channel block: the stage switches at every tile)
    ak, wkk = _cb_order(a), _cb_order(wk)
    if mut == "quartet halves exchanged":                                 # slots 4..7 of the middle unit's second lane group
        k0 = (9 * C // 32 // 2) * 32 + 8
        return _chain3(ak, wkk, swap_k=torch.arange(k0 + 4, k0 + 8))
    return _mfma_chain(ak, wkk, DT)


def _epilogue(acc, b, act, mut):
    b = b.float()
    if mut == "bias of the next 4-channel block":
        b = torch.roll(b, -4)
    elif mut == "second column tile with the first's bias" and b.shape[0] > 128:
        b = torch.cat([b[:128], b[:b.shape[0] - 128]])
    v = acc + b
    return round_to(torch.clamp(v, min=0.0) if act == ACT_RELU else v, DT)


def emulate_conv(x, w, b, act, mut=None, n_cu=256):
    """conv3_halo_kernel in float32, rows: K summed in (channel block, tap, channel) order, one MFMA per 32 k with the accumulator rounded
    to fp32 after each of the three partial products on weights scaled by f16x2_weight_scale and split; acc * ws + bias, ReLU, packed to
    hi + lo.  Not followed: the order inside an MFMA, the fma of the epilogue.  A mutant that names a feature the launch does not have (a
    second column tile, a second tile of a workgroup, a ragged tile) is the identity."""
    assert mut is None or mut in MUTANTS, mut
    return _epilogue(_conv_acc(x, w, mut, n_cu), b, act, mut)


def _lane_order():
    """Position (lane group g, slot i) of a K-step of the tail -> channel of the 32: i < 4: 4 g + i, else 16 + 4 g + i - 4 (pack_bneck_tail)."""
    return torch.tensor([4 * g + i if i < 4 else 16 + 4 * g + i - 4 for g in range(4) for i in range(8)])


def emulate_bneck(t1, idn, wb, y_only=False, mut=None, n_cu=256):
    """bneck_tail_kernel in float32: (y, t1' or None) rows.  Phase A is emulate_conv's loop; t2 = ReLU(acc + b2) rounded with the pack;
    conv3 over K = 64 as two MFMA steps whose 32 k-slots are pack_bneck_tail's (a permutation inside a step, invisible to a model that
    sums a step exactly -- but not to the mutant that packs them in another order than the lanes hold them); + b3, + identity (the fp32 sum
    of its halves: the value), ReLU, pack; y's groups of 32 channels are conv1's K-steps."""
    assert mut is None or mut in MUTANTS, mut
    w2, b2, w3, b3, w1, b1 = (t.float() for t in wb)
    t2 = _epilogue(_conv_acc(t1, w2, mut, n_cu), b2, ACT_RELU, mut if mut in ("bias of the next 4-channel block",) else None)
    if mut == "bneck: t2 not rounded":
        t2 = torch.clamp(_conv_acc(t1, w2, None, n_cu) + b2, min=0.0)
    idr = rows_of(idn.float())
    w3m = w3.clone()
    if mut == "bneck: conv3 k-slots in natural order":                    # the lanes hold channel lane_order[p] at position p; the weights sit at p
        lo = _lane_order()
        for j in range(2):
            w3m[:, 32 * j + lo] = w3[:, 32 * j:32 * j + 32]
    elif mut == "bneck: identity of group q + 1":
        idr = torch.roll(idr, -32, 1)
    elif mut == "bneck: y-only fed the full stream" and y_only:           # units B0 C0 B1 C1 .. read as B0 .. B7
        f = _x2_scale(w1) / _x2_scale(w3)
        for q in range(8):
            if q % 2 == 0:
                w3m[32 * q:32 * q + 32] = w3[32 * (q // 2):32 * (q // 2) + 32]
            else:
                for j in range(2):
                    w3m[32 * q:32 * q + 32, 32 * j:32 * j + 32] = w1[32 * j:32 * j + 32, 32 * (q // 2):32 * (q // 2) + 32] * f
    if mut == "bneck: t2 not rounded":                                    # (the halves cannot carry an unrounded t2: the chain is run in float64)
        ya = (t2.double() @ w3m.double().t()).float()
    else:
        ya = _mfma_chain(t2, w3m, DT)
    y = round_to(torch.clamp((ya + b3) + idr, min=0.0), DT)
    if y_only:
        return y, None
    return y, round_to(torch.clamp(_mfma_chain(y, w1, DT) + b1, min=0.0), DT)


def emulate_stem(x, w, b, dt=DT, fused=True, mut=None, n_cu=256):
    """stem_pool_kernel (fused; f16x2) or the two-kernel stem of element type `dt` in float32, rows of pooled pixels.  K-step = filter row
    (8 pixels x 4 channels; the 16-bit types' 64-element K-steps take two rows: the same chain of 32); bias, ReLU; the fused kernel pools
    its fp32 staging and packs, the two-kernel form rounds the conv map to T and pools that: one result, rounding being monotone."""
    assert mut is None or mut in MUTANTS, mut
    x, w, b = x.float(), w.float(), b.float()
    n, _, H, W = x.shape
    CH, CW = H // 2, W // 2
    a8, wk = stem_a8(x), stem_wk(w)
    a = a8[:, 1:8] if mut == "stem: filter row r against input row r + 1" else a8[:, :7]
    if mut == "stem: pad slot times a live weight":
        wk = wk.clone()
        wk[:, :, 7, :3] = wk[:, :, 6, :3]
    K = 224 if dt in ("f32", "f16x2") else 256
    ak, wkk = torch.zeros(a.shape[0], K), torch.zeros(64, K)
    ak[:, :224], wkk[:, :224] = a.reshape(-1, 224), wk.reshape(64, 224)
    conv = round_to(torch.clamp(_mfma_chain(ak, wkk, dt) + b, min=0.0), "f32" if fused else dt)
    c4 = conv.reshape(n, CH, CW, 64).permute(0, 3, 1, 2)
    if mut == "stem: pool padding 0":
        out = rows_of(F.max_pool2d(F.pad(c4, (1, 1, 1, 1)), 3, 2, 0))
    elif mut == "stem: halo conv row not recomputed" and fused:
        # tile (ty > 0)'s first staging row is left from the workgroup's tile before (t - grid; nothing before its first: zeros)
        _, _, txN, tyN, grid, _, _ = stem_plan(n, H, W, n_cu)
        cp = F.pad(c4, (1, 2 * SP_PW * txN, 1, 2 * SP_PH * tyN), value=float("-inf"))     # conv (r, c) at cp[r + 1, c + 1]
        out4 = torch.empty(n, 64, H // 4, W // 4)
        stage = lambda t: cp[t // (tyN * txN), :, 2 * SP_PH * (t // txN % tyN):, 2 * SP_PW * (t % txN):][:, :2 * SP_PH + 1, :2 * SP_PW + 1]
        for t in range(n * tyN * txN):
            st = stage(t).clone()
            if t // txN % tyN > 0:
                st[:, 0] = stage(t - grid)[:, 0].clamp(min=0.0) if t >= grid else 0.0
            py0, px0 = SP_PH * (t // txN % tyN), SP_PW * (t % txN)
            p = F.max_pool2d(st[None], 3, 2, 0)[0]
            hh, ww = min(SP_PH, H // 4 - py0), min(SP_PW, W // 4 - px0)
            out4[t // (tyN * txN), :, py0:py0 + hh, px0:px0 + ww] = p[:, :hh, :ww]
        out = rows_of(out4)
    else:
        out = rows_of(F.max_pool2d(c4, 3, 2, 1))
    return round_to(out, dt)


# ------------------------------------------------------------------------------------------------ input families
def routed_dense(Co, K, seed, nc=128, extra=3):
    """w [Co, K] of 0 / +-1.  Column c of a column tile of nc columns (nl of them live: nc, or what is left of Co) has a weight at every
    k = c (mod nl), so inside EVERY column tile every k is used by some column, one more at k = (c + 1 + the tile's index) mod nl, which
    keeps the channels of different tiles apart, and 0 .. `extra` seeded entries; the signs are seeded."""
    g = _gen(seed)
    n = torch.arange(Co)
    tile0 = n // nc * nc
    nl = torch.clamp(Co - tile0, max=nc)
    k = torch.arange(K)
    cover = (k[None, :] % nl[:, None]) == (n - tile0)[:, None]
    cover |= k[None, :] == ((n - tile0 + 1 + n // nc) % nl)[:, None]
    want = cover.sum(1) + (n * 7 + seed) % (extra + 1)
    score = torch.rand(Co, K, generator=g)
    score[cover] = 2.0
    rank = score.argsort(1, descending=True).argsort(1)
    sign = torch.randint(0, 2, (Co, K), generator=g) * 2.0 - 1.0
    return torch.where(rank < want[:, None], sign, torch.zeros(()))


def routed_conv_case(n, C, H, W, Co, seed):
    """(x, w, b): integers in [-7, 7], routed_dense in (tap, channel) order over the launch's column tiles, integer bias in [-8, 8]."""
    g = _gen(seed + 1)
    x = torch.randint(-7, 8, (n, C, H, W), generator=g).float()
    nc = 64 if np_of(Co) == 64 else 128
    w = routed_dense(Co, 9 * C, seed, nc).reshape(Co, 3, 3, C).permute(0, 3, 1, 2).contiguous()
    return x, w, torch.randint(-8, 9, (Co,), generator=g).float()


def routed_bneck_case(n, H, W, seed):
    """(t1, identity, (w2, b2, w3, b3, w1, b1)): t1 in [-7, 7]; conv2 routed over its 64 columns, conv3 over every group of 32 channels
    (each group is a unit of the tail: every t2 channel is used in every group), conv1 over its 64; integer biases; identity in [0, 32]."""
    g = _gen(seed + 1)
    t1 = torch.randint(-7, 8, (n, 64, H, W), generator=g).float()
    idn = torch.randint(0, 33, (n, 256, H, W), generator=g).float()
    w2 = routed_dense(64, 576, seed, 64).reshape(64, 3, 3, 64).permute(0, 3, 1, 2).contiguous()
    w3 = routed_dense(256, 64, seed + 2, 32, 2)
    w1 = routed_dense(64, 256, seed + 3, 64, 2)
    b2, b3, b1 = (torch.randint(-8, 9, (c,), generator=g).float() for c in (64, 256, 64))
    return t1, idn, (w2, b2, w3, b3, w1, b1)


def routed_stem_case(n, H, W, seed):
    g = _gen(seed + 1)
    x = torch.randint(-7, 8, (n, 3, H, W), generator=g).float()
    w = routed_dense(64, 147, seed, 64).reshape(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()
    return x, w, torch.randint(-8, 9, (64,), generator=g).float()


def value_conv_case(n, C, H, W, Co, seed):
    """conv_refs.value_case without its residual."""
    x, w, b, _ = R.value_case(n, C, H, W, Co, (1, 1), 1, DT, 0, seed)
    return x, w, b


def _halves(N, K, g, dt=DT):
    w1 = torch.randn(N, K // 2, generator=g) / K ** 0.5
    return round_to(torch.cat([w1, w1], 1), dt)


def value_bneck_case(n, H, W, seed):
    """t1 and conv2 of value_conv_case; conv3 and conv1 Gaussian with two equal halves; the biases sweep [-12, 12]; a non-negative identity."""
    t1, w2, b2 = value_conv_case(n, 64, H, W, 64, seed)
    g = _gen(seed + 3)
    idn = round_to(torch.randn(n, 256, H, W, generator=g).abs(), DT)
    return t1, idn, (w2, b2, _halves(256, 64, g), torch.linspace(-12.0, 12.0, 256), _halves(64, 256, g), torch.linspace(-12.0, 12.0, 64))


def value_stem_case(n, H, W, dt, seed):
    """x by image row as conv_refs.value_case (the cancelling rows: channel 1 = -channel 0 + 2^-6 Gaussian, channel 2 = 2^-6 Gaussian, all
    times 8, against weights whose channels 0 and 1 are equal); w Gaussian / sqrt(147); the bias sweeps [-12, 12].  Rounded to `dt`."""
    g = _gen(seed)
    x = torch.randn(n, 3, H, W, generator=g)
    noise = torch.randn(n, 3, H, W, generator=g) * 2.0 ** -6
    for y in range(H):
        kind = ROW_KINDS[y % 4]
        if kind == "cancel":
            x[:, 1, y] = -x[:, 0, y] + noise[:, 1, y]
            x[:, 2, y] = noise[:, 2, y]
            x[:, :, y] *= 8.0
        elif kind == "small":
            x[:, :, y] *= 2.0 ** -10
        elif kind == "outlier":
            x[:, y % 3, y, (7 * y) % W] = 100.0
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    w[:, 1] = w[:, 0]
    return round_to(x, dt), round_to(w, dt), torch.linspace(-12.0, 12.0, 64)


def _impulse_sites(n, H, W, step):
    """Pixels (image, y, x) with y = x = step // 2 (mod step) -- or row / column 0 where the map is too small for that."""
    ys = [y for y in range(H) if y % step == step // 2] or [0]
    xs = [x for x in range(W) if x % step == step // 2] or [0]
    return [(i, y, x) for i in range(n) for y in ys for x in xs]


def probe_a_launches(n, C, H, W, step=3):
    """Launches the impulse probe needs for the impulse channel to run over all C."""
    return cdiv(C, len(_impulse_sites(n, H, W, step)))


def probe_a_x(n, C, H, W, launch, step=3):
    """Impulses +-2^e, e in 0 .. 5 (an f16x2-exact weight times 2^e is f16x2-exact: both halves scale; 2^-e would push lo halves under
    fp16's subnormal spacing), at _impulse_sites; site i of launch l carries channel (i + l sites) mod C."""
    x = torch.zeros(n, C, H, W)
    sites = _impulse_sites(n, H, W, step)
    for i, (im, y, xx) in enumerate(sites):
        j = i + launch * len(sites)
        x[im, j % C, y, xx] = (-1.0) ** (j // 2) * 2.0 ** (j % 6)
    return x


def probe_a_conv_case(n, C, H, W, Co, launch, seed):
    g = _gen(seed)
    w = round_to(torch.randn(Co, C, 3, 3, generator=g) / (9 * C) ** 0.5, DT)
    return probe_a_x(n, C, H, W, launch), w, torch.zeros(Co)


def probe_a_stem_case(n, H, W, launch, dt, seed):
    """Impulses 7 apart: no 7x7 window holds two."""
    g = _gen(seed)
    w = round_to(torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5, dt)
    return probe_a_x(n, 3, H, W, launch, 7), w, torch.zeros(64)


def probe_b_launches(K, Co):
    return cdiv(K, Co)


def probe_b_weights(Co, K, launch):
    """[Co, K]: channel c has 2^(c mod 3), negative for every third launch-channel, at k = (launch Co + c) mod K."""
    w = torch.zeros(Co, K)
    c = torch.arange(Co)
    w[c, (launch * Co + c) % K] = (1.0 - 2.0 * ((c + launch) % 3 == 2)) * 2.0 ** (c % 3)
    return w


def probe_b_conv_case(n, C, H, W, Co, launch, seed):
    x, _, _ = value_conv_case(n, C, H, W, Co, seed)
    w = probe_b_weights(Co, 9 * C, launch).reshape(Co, 3, 3, C).permute(0, 3, 1, 2).contiguous()
    return x, w, torch.zeros(Co)


def probe_b_stem_case(n, H, W, launch, dt, seed):
    x, _, _ = value_stem_case(n, H, W, dt, seed)
    w = probe_b_weights(64, 147, launch).reshape(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()
    return x, w, torch.zeros(64)


def probe_c_bneck_case(n, H, W, launch, seed):
    """Pass-through: t2 = t1 (>= 0), y = [t2 | t2 | identity's channels 128 ..], t1'[m] = 2^(m mod 2) y[64 launch + m]."""
    t1, _, _ = value_conv_case(n, 64, H, W, 64, seed)
    t1 = t1.abs()
    g = _gen(seed + 5)
    idn = round_to(torch.randn(n, 256, H, W, generator=g).abs(), DT)
    idn[:, :128] = 0
    w2 = torch.zeros(64, 64, 3, 3)
    w2[torch.arange(64), torch.arange(64), 1, 1] = 1.0
    w3 = torch.zeros(256, 64)
    w3[torch.arange(128), torch.arange(128) % 64] = 1.0
    w1 = torch.zeros(64, 256)
    w1[torch.arange(64), 64 * launch + torch.arange(64)] = 2.0 ** (torch.arange(64) % 2)
    return t1, idn, (w2, torch.zeros(64), w3, torch.zeros(256), w1, torch.zeros(64))


def probe_a_bneck_case(n, H, W, launch, seed):
    """Probe a through the chain: impulses into t1, conv2 full-width Gaussian, the tail passing through as in probe c:
    y[c] = relu(one conv2 weight times a power of two) for c < 128."""
    _, idn, (_, b2, w3, b3, w1, b1) = probe_c_bneck_case(n, H, W, launch % 4, seed)
    w2 = round_to(torch.randn(64, 64, 3, 3, generator=_gen(seed)) / 24.0, DT)
    return probe_a_x(n, 64, H, W, launch), idn, (w2, b2, w3, b3, w1, b1)


def probe_b_bneck_case(n, H, W, launch, seed):
    """Probe b through the chain: conv2 one-hot at every (tap, channel) in nine launches on full-width value data (not made non-negative:
    t2 = relu of a shifted copy of +-2^e t1), the tail passing through as in probe c."""
    _, idn, (_, b2, w3, b3, w1, b1) = probe_c_bneck_case(n, H, W, launch % 4, seed)
    t1, _, _ = value_conv_case(n, 64, H, W, 64, seed)
    w2 = probe_b_weights(64, 576, launch).reshape(64, 3, 3, 64).permute(0, 3, 1, 2).contiguous()
    return t1, idn, (w2, b2, w3, b3, w1, b1)


def rounding_bneck_case(n, H, W):
    """t2[2 i] = 512.25 + m 2^-14 with m = 1, 3, 5, .. by pixel (24 significant bits: the fp32 accumulator holds it; as hi + lo it is
    512 + (0.25 + m 2^-14), a lo half of 13 bits that the pack rounds to 11, never on a tie), t2[2 i + 1] = 512.25;
    y[c] = t2[2 i] - t2[2 i + 1] for c < 128 (i = c mod 32), 0 above; t1'[m] = 2^12 y[m].  Reference: bneck_ref(round_t2=True)."""
    t1 = torch.zeros(n, 64, H, W)
    m = (2 * torch.arange(n * H * W) + 1).reshape(n, H, W) % 64
    t1[:, 0] = 512.25
    t1[:, 1] = m * 2.0 ** -14
    w2 = torch.zeros(64, 64, 3, 3)
    w2[:, 0, 1, 1] = 1.0
    w2[0::2, 1, 1, 1] = 1.0
    w3 = torch.zeros(256, 64)
    c = torch.arange(128)
    w3[c, 2 * (c % 32)] = 1.0
    w3[c, 2 * (c % 32) + 1] = -1.0
    w1 = torch.zeros(64, 256)
    w1[torch.arange(64), torch.arange(64)] = 2.0 ** 12
    return t1, torch.zeros(n, 256, H, W), (w2, torch.zeros(64), w3, torch.zeros(256), w1, torch.zeros(64))


# ------------------------------------------------------------------------------------------------ the cases of the GPU files
CONV_SHAPES = (            # n, Cin, H, W, Co
    (1, 32, 16, 16, 64),        # one tile, one channel block
    (1, 64, 1, 1, 64),          # every outer tap in the halo
    (1, 32, 17, 16, 128),       # a second tile of one row
    (1, 32, 16, 17, 128),       # ... of one column
    (2, 96, 21, 18, 120),       # three channel blocks, 120 of 128 columns
    (3, 64, 17, 23, 36),        # 36 of 64 columns
    (1, 64, 5, 70, 132),        # two column tiles, the second with four live columns, a ragged last pixel tile
    (2, 256, 19, 33, 256),      # eight channel blocks, an image boundary inside the batch
)
BNECK_SHAPES = ((1, 16, 16), (1, 1, 1), (1, 17, 16), (1, 16, 17), (3, 17, 23), (1, 5, 70))      # n, H, W
STEM_SHAPES = ((1, 8, 8), (1, 32, 28), (1, 36, 28), (1, 32, 32), (3, 36, 52), (1, 132, 88))      # n, H, W of the image
LATER_CONV = ((32, 64), (64, 128), (64, 256))      # Cin, Co on 48 x 48 images
STEM_DTS = G.DTS
