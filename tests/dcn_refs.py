"""The modulated deformable 3x3 convolution (csrc/dcn_pipe.h for bf16 / f16 / f16x2, conv_gemm.h's AM_DCN mode for fp32) in plain float64, a
per-element error bound derived from the reference's own intermediates, an fp32 emulation of the kernels' order of operations with sixteen
deliberate errors, and the input families and cases of tests/test_gpu_dcn_sampling.py.  tests/test_dcn_refs_cpu.py shows on the CPU that the
reference is the oracle's, that the emulation equals it on the probe cases and stays inside the bound on the value cases, that every wrong
kernel is caught by a case of the GPU list, and -- through ocrvi_test_dcn_plan, which touches no device -- which patch, tile and K-step
count every case reaches.  No GPU, no library: torch and numpy only.

    out[m, :] = relu(columns[m, :] W^T + b (+ res))      m = (image, oh, ow), columns = the 9 C masked bilinear samples of pixel m

Offsets lie on a 2^-10 grid with |offset| <= 64 and masks on a 2^-8 grid (every builder asserts it): sampling positions and the bilinear
weights hy hx are then exact in fp32 and in float64 alike, and the inside / outside decisions of kernel and reference cannot differ for
rounding reasons.  The wild offsets of the "wild" probe case (+-1e9, +-3e38, +-inf, NaN) are the one exception: all of them sample nothing.
"""
import functools
import math

import torch

from aux_refs import U32, half_ulp, round_to
from gemm_refs import ACT_NONE, ACT_RELU, DT_CODE, DTS, bke, err_ratio, gemm_bound
from mlp_refs import _mfma_chain

OFF_GRID, MASK_GRID, OFF_MAX = 2.0 ** -10, 2.0 ** -8, 64.0
PIPE = ("bf16", "f16", "f16x2")          # the types the default dispatch sends to dcn_pipe.h; fp32 goes to conv_gemm


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def patch_lw(Ho, Wo):
    """launch_dcn_pipe's rule (dcn_pipe_plan): the (128 >> lw) x (1 << lw) patch that covers the map with the fewest pixels, ties to the
    squarer one.  The plan hook is the authority; tests/test_dcn_refs_cpu.py holds this copy to it."""
    best, best_lw = None, 4
    for lw in (4, 3, 5, 2, 6, 7):
        pw, ph = 1 << lw, 128 >> lw
        covered = -(-Ho // ph) * ph * -(-Wo // pw) * pw
        if best is None or covered < best:
            best, best_lw = covered, lw
    return best_lw


def _base(N, Ho, Wo, stride, dtype=torch.float64):
    """Unshifted sampling positions [M, 9] of every (pixel, tap): (oh s - 1 + r, ow s - 1 + c), and the image index [M]."""
    m = torch.arange(N * Ho * Wo)
    ow, oh, img = m % Wo, (m // Wo) % Ho, m // (Ho * Wo)
    tap = torch.arange(9)
    by = (oh * stride - 1)[:, None] + (tap // 3)[None, :]
    bx = (ow * stride - 1)[:, None] + (tap % 3)[None, :]
    return by.to(dtype), bx.to(dtype), img


def _rows(t):
    """[N, C, Ho, Wo] -> [N Ho Wo, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------ float64 reference
def sample_columns(x, off, mask, stride):
    """(columns, Sabs), both [N Ho Wo, 9 C] float64 in (tap, channel) order.  torchvision's rule as both kernels state it: the sample of
    tap (r, c) of output pixel (oh, ow) lies at (oh s - 1 + r + dy, ow s - 1 + c + dx); each of the four corners of its bilinear cell
    contributes only if it lies inside the image; everything outside (-1, H) x (-1, W) is 0, and so is a non-finite position.
    Sabs = sum over corners of |weight mask| |x|: what the rounding errors of the blend are relative to."""
    N, C, H, W = x.shape
    Ho, Wo = off.shape[-2:]
    by, bx, img = _base(N, Ho, Wo, stride)
    o = _rows(off.double()).reshape(-1, 9, 2)
    mk = _rows(mask.double())
    py, px = by + o[..., 0], bx + o[..., 1]
    ok = (py.abs() < 2.0 ** 30) & (px.abs() < 2.0 ** 30)         # (false for NaN and inf; a finite position this far out samples nothing either)
    py, px = torch.where(ok, py, torch.zeros(())), torch.where(ok, px, torch.zeros(()))
    inside = ok & (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    hy, hx = 1 - ly, 1 - lx
    y0, x0 = y0.long(), x0.long()
    xr = x.double().permute(0, 2, 3, 1).reshape(N * H * W, C)
    cols = torch.zeros(N * Ho * Wo, 9, C, dtype=torch.float64)
    sabs = torch.zeros_like(cols)
    for yy, xx, wgt in ((y0, x0, hy * hx), (y0, x0 + 1, hy * lx), (y0 + 1, x0, ly * hx), (y0 + 1, x0 + 1, ly * lx)):
        use = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        wm = torch.where(use, wgt * mk, torch.zeros(()))
        v = xr[(img[:, None] * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1)]
        cols += wm[..., None] * v
        sabs += wm.abs()[..., None] * v.abs()
    return cols.reshape(-1, 9 * C), sabs.reshape(-1, 9 * C)


def weight_rows(w):
    """[Co, C, 3, 3] -> [Co, 9 C] in (tap, channel) order."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def dcn_ref(x, off, mask, w, b, res, stride, relu=True):
    """relu(columns W^T + b (+ res)) in float64, [N Ho Wo, Co]."""
    cols, _ = sample_columns(x, off, mask, stride)
    y = cols @ weight_rows(w).double().t() + b.double()
    if res is not None:
        y = y + _rows(res.double())
    return torch.clamp(y, min=0.0) if relu else y


def blend_roundings(dt):
    """Roundings between the exact masked bilinear sample and the fp32 value the kernel packs (dcn_pipe.h: geometry loop and blend();
    conv_gemm.h: issue() and commit()): hy = 1 - ly, hx = 1 - lx (or none: ly, lx), their product, the product with the mask -- four on a
    corner's weight --, then one fmaf per corner, four in the chain.  f16x2 (Chunk<f16x2_t>::fma) adds a corner's lo half and its hi half
    in two fmas: eight in the chain."""
    return 12 if dt == "f16x2" else 8


def dcn_bound(x, off, mask, w, b, res, stride, dt, relu=True):
    """Bound on |kernel - dcn_ref| per element, in the manner of gemm_refs.gemm_bound.  x, w and res must be exact in `dt` (the builders
    pre-round them), so the hook's casts are exact.  Two parts, u = 2^-24:
      blend   a column element is sum_q w_q x_q over the corners, w_q = hy hx mask.  The kernel computes w_q with four roundings
              (blend_roundings) -- w'_q = w_q (1 + d)^4 -- and then acc_q = fl(w'_q x_q + acc_(q-1)), each rounding at most u |acc_q| <=
              u (1 + u)^q sum |w'_q x_q|.  Together at most g_k Sabs with g_k = k u / (1 - k u), k = 8 (Higham's gamma).  f16x2 feeds
              x_q as lo then hi, eight fmas, over sum |w| (|hi| + |lo|) <= (1 + 2^-10) Sabs: k = 12.
              The result is packed to T: half_ulp(|column| + that, T) (f16x2: f16x2_round; fp32: nothing).
      GEMM    what the MFMAs multiply is therefore some a' with |a' - column| <= a_err, exact in T: gemm_bound with a_err carries
              a_err |W|^T and bounds products, sum, bias, residual, ReLU and the output rounding as for the ring GEMM.  (It charges
              the fp32 and f16x2 accumulators with the bias from the start, which these kernels add in the epilogue: S is only larger.)"""
    assert torch.equal(round_to(x.float(), dt), x.float()), f"x must be exact in {dt}"
    cols, sabs = sample_columns(x, off, mask, stride)
    k = blend_roundings(dt)
    if dt == "f16x2":
        sabs = sabs * (1 + 2.0 ** -10)
    be = k * U32 / (1 - k * U32) * sabs
    a_err = be + half_ulp(cols.abs() + be, dt)
    rr = None if res is None else _rows(res)
    return gemm_bound(cols, weight_rows(w), b, rr, ACT_RELU if relu else ACT_NONE, 0, dt, 0, a_err=a_err)


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
MUTANTS = ("oy0 check missing", "y1 <= H for y1 <= H-1", "dx bit dropped", "dy bit dropped", "lx and hx exchanged", "dy and dx channels exchanged",
           "mask of the next tap", "tap row and column transposed", "stride ignored", "padding off by one", "truncation for floorf",
           "image index dropped", "offsets of pixel m + 1", "weights (tap, ch) against columns (block, tap, ch)", "f16x2 pack without lo",
           "patch row and column exchanged")


def _fma(a, b, c):
    """fmaf in float32 (the product of two fp32 numbers is exact in float64; the sum is rounded to float64 and then to float32, which
    differs from one rounding only at a float32 tie that the float64 rounding created)."""
    return (a.double() * b.double() + c.double()).float()


def emulate(x, off, mask, w, b, res, stride, dt, relu=True, mut=None):
    """The kernel in float32, [N Ho Wo, Co]: the geometry as written in dcn_pipe.h's per-tile loop and conv_gemm.h's issue() (position,
    inside test, clamp, floorf, the corner predicates, the clamped corner (y0, x0) with its dx / dy bits), the fmaf chain over the four
    corners (f16x2: lo then hi), the pack to T, gemm_refs' MFMA chain over the kernel's K order ((channel block, tap, channel) on dcn_pipe,
    (tap, channel) on conv_gemm), bias, residual and ReLU in the epilogue, the output rounded to T.  Not followed: the order inside an
    MFMA, and fp32's individual product roundings.  `mut`: one of MUTANTS, a deliberately wrong kernel.  An element that a wrong kernel
    never stores is NaN, as it is in the GPU test's pre-filled output."""
    assert mut is None or mut in MUTANTS, mut
    N, C, H, W = x.shape
    Ho, Wo = off.shape[-2:]
    Co = w.shape[0]
    M = N * Ho * Wo
    f32 = torch.float32
    o = _rows(off.float()).reshape(M, 9, 2)
    mk = _rows(mask.float())
    if mut == "offsets of pixel m + 1":
        o, mk = torch.roll(o, -1, 0), torch.roll(mk, -1, 0)
    dy, dx = (o[..., 1], o[..., 0]) if mut == "dy and dx channels exchanged" else (o[..., 0], o[..., 1])
    if mut == "mask of the next tap":
        mk = torch.roll(mk, -1, 1)
    m = torch.arange(M)
    ow, oh, img = m % Wo, (m // Wo) % Ho, m // (Ho * Wo)
    tap = torch.arange(9)
    r, s = (tap % 3, tap // 3) if mut == "tap row and column transposed" else (tap // 3, tap % 3)
    st = 1 if mut == "stride ignored" else stride
    pad = 0 if mut == "padding off by one" else 1
    py = ((oh * st - pad)[:, None] + r[None, :]).to(f32) + dy
    px = ((ow * st - pad)[:, None] + s[None, :]).to(f32) + dx
    inside = (py > -1.0) & (py < float(H)) & (px > -1.0) & (px < float(W))
    cy = torch.where(torch.isnan(py), torch.full_like(py, -2.0), py).clamp(-2.0, H + 1.0)      # fminf(fmaxf(NaN, -2), H + 1) = -2
    cx = torch.where(torch.isnan(px), torch.full_like(px, -2.0), px).clamp(-2.0, W + 1.0)
    rnd = torch.trunc if mut == "truncation for floorf" else torch.floor
    fy, fx = rnd(cy), rnd(cx)
    ly, lx = cy - fy, cx - fx
    hy, hx = 1.0 - ly, 1.0 - lx
    if mut == "lx and hx exchanged":
        lx, hx = hx, lx
    y0, x0 = fy.long(), fx.long()
    y1, x1 = y0 + 1, x0 + 1
    oy0 = torch.ones_like(inside) if mut == "oy0 check missing" else y0 >= 0
    oy1 = (y1 <= H) if mut == "y1 <= H for y1 <= H-1" else (y1 <= H - 1)
    ox0, ox1 = x0 >= 0, x1 <= W - 1
    mm = torch.where(inside, mk, torch.zeros(()))
    zero = torch.zeros((), dtype=f32)
    wq = (torch.where(oy0 & ox0, hy * hx * mm, zero), torch.where(oy0 & ox1, hy * lx * mm, zero),
          torch.where(oy1 & ox0, ly * hx * mm, zero), torch.where(oy1 & ox1, ly * lx * mm, zero))
    yc0, yc1, xc0, xc1 = y0.clamp(0, H - 1), y1.clamp(0, H - 1), x0.clamp(0, W - 1), x1.clamp(0, W - 1)
    dxb = torch.zeros_like(xc0) if mut == "dx bit dropped" else xc1 - xc0
    dyb = torch.zeros_like(yc0) if mut == "dy bit dropped" else yc1 - yc0
    p00 = (torch.zeros_like(img) if mut == "image index dropped" else img)[:, None] * (H * W) + yc0 * W + xc0
    xr = x.float().permute(0, 2, 3, 1).reshape(N * H * W, C)
    acc = torch.zeros(M, 9, C, dtype=f32)
    for q, idx in enumerate((p00, p00 + dxb, p00 + dyb * W, p00 + dyb * W + dxb)):
        v = xr[idx]
        wv = wq[q][..., None]
        if dt == "f16x2":
            hi = v.half().float()
            acc = _fma(wv, hi, _fma(wv, v - hi, acc))
        else:
            acc = _fma(wv, v, acc)
    a = acc.half().float() if (mut == "f16x2 pack without lo" and dt == "f16x2") else round_to(acc, dt)
    cb = bke(dt)
    wr = w.float().permute(0, 2, 3, 1).reshape(Co, 9, C)
    blocked = lambda t: t.reshape(t.shape[0], 9, C // cb, cb).permute(0, 2, 1, 3).reshape(t.shape[0], 9 * C)
    flat = lambda t: t.reshape(t.shape[0], 9 * C)
    if mut == "weights (tap, ch) against columns (block, tap, ch)":
        ak, wk = blocked(a), flat(wr)
    elif dt in PIPE:
        ak, wk = blocked(a), blocked(wr)
    else:
        ak, wk = flat(a), flat(wr)
    v = _mfma_chain(ak, wk, dt) + b.float()
    if res is not None:
        v = v + _rows(res.float())
    if relu:
        v = torch.clamp(v, min=0.0)
    out = round_to(v, dt)
    if mut == "patch row and column exchanged" and dt in PIPE:
        # pixel_of(row) = (oh0 + (row & (PW - 1)), ow0 + (row >> lw)): a tile covers PW rows x PH columns from its origin; geometry and
        # epilogue agree with each other, so every pixel that is stored is right, and the pixels no tile covers are never stored
        lw = patch_lw(Ho, Wo)
        pw, ph = 1 << lw, 128 >> lw
        covered = ((oh % ph) < pw) & ((ow % pw) < ph)
        out = torch.where(covered[:, None], out, torch.full((), float("nan")))
    return out


# ------------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_grid(off, mask, stride, wild=None):
    """The condition of the module docstring: offsets on the 2^-10 grid within +-64, masks on the 2^-8 grid, positions exact in fp32.
    `wild`: a boolean tensor like off marking the entries of the wild case that are exempt."""
    o = off.double() if wild is None else torch.where(wild, torch.zeros((), dtype=torch.float64), off.double())
    assert torch.equal(o / OFF_GRID, torch.round(o / OFF_GRID)) and float(o.abs().max()) <= OFF_MAX
    mk = mask.double()
    assert torch.equal(mk / MASK_GRID, torch.round(mk / MASK_GRID)) and float(mk.min()) >= 0 and float(mk.max()) <= 1
    N, _, Ho, Wo = off.shape
    by, bx, _ = _base(N, Ho, Wo, stride)
    oo = _rows(o).reshape(-1, 9, 2)
    for base, d in ((by, oo[..., 0]), (bx, oo[..., 1])):
        assert torch.equal((base.float() + d.float()).double(), base + d)


TARGET_KINDS = ("-1", "-1 + 1/4", "-1/4", "0", "interior", "interior + 3/4", "L-1", "L-1 + 1/4", "L - 1/4", "L", "L + 5")
WILD = (1e9, -1e9, 3e38, -3e38, float("inf"), float("-inf"), float("nan"))


def _targets(L, base):
    """[.., 11] sampling positions of TARGET_KINDS on an axis of L pixels; "interior" is the integer nearest the unshifted position that
    has both neighbours inside (on an axis of one or two pixels there is none: the nearest pixel)."""
    inter = base.clamp(min(1, L - 1), max(L - 2, 0))
    c = lambda v: torch.full_like(base, float(v))
    return torch.stack([c(-1), c(-0.75), c(-0.25), c(0), inter, inter + 0.75, c(L - 1), c(L - 0.75), c(L - 0.25), c(L), c(L + 5)], -1)


def probe_offsets(N, H, W, stride):
    """Constructed offsets [N, 18, Ho, Wo]: tap t of pixel m (counted over the whole batch) is sent to target kind (m + 3 t) % 11 on the y
    axis and (m + m // 11 + 5 t) % 11 on the x axis, so that any 121 consecutive pixels pair every kind with every kind in every tap.  Where
    that target is more than 64 pixels away its mirror image (kind 10 - k) is taken, and the interior kind where that is too.  Asserted:
    on both axes every tap reaches every kind, and every (y kind, x kind) pair occurs in every tap (on a map wider than 64 pixels, where
    targets were replaced: in some tap); corner, edge and interior output pixels each reach every target value on both axes."""
    Ho, Wo = out_hw(H, W, stride)
    by, bx, _ = _base(N, Ho, Wo, stride)
    m = torch.arange(N * Ho * Wo)[:, None]
    t = torch.arange(9)[None, :]
    out, kinds = [], []
    for L, base, k in ((H, by, (m + 3 * t) % 11), (W, bx, (m + m // 11 + 5 * t) % 11)):
        tg = _targets(L, base)
        far = lambda kk: (tg.gather(-1, kk[..., None])[..., 0] - base).abs() > OFF_MAX
        k = torch.where(far(k), 10 - k, k)
        k = torch.where(far(k), torch.full_like(k, 4), k)
        out.append(tg.gather(-1, k[..., None])[..., 0] - base)
        kinds.append(k)
        for tap in range(9):
            assert set(k[:, tap].tolist()) == set(range(11)), (L, tap)
    pairs = [set((kinds[0][:, tap] * 11 + kinds[1][:, tap]).tolist()) for tap in range(9)]
    if max(H, W) <= OFF_MAX:
        assert all(len(p) == 121 for p in pairs), [len(p) for p in pairs]
    else:               # (a map wider than 64 pixels replaces the targets that are too far: every pair occurs, not in every tap)
        assert len(set().union(*pairs)) == 121, [len(p) for p in pairs]
    # corner, edge and interior output pixels (as far as the map has them) each reach every target value on both axes
    ow, oh = m[:, 0] % Wo, (m[:, 0] // Wo) % Ho
    borders = ((oh == 0) | (oh == Ho - 1)).long() + ((ow == 0) | (ow == Wo - 1)).long()
    for (L, base), d in zip(((H, by), (W, bx)), out):
        at = _targets(L, base) == (base + d)[..., None]
        for cls in (0, 1, 2):
            assert not bool((borders == cls).any()) or bool(at[borders == cls].any(0).any(0).all()), (L, cls)
    o = torch.stack(out, -1).reshape(N, Ho, Wo, 18).permute(0, 3, 1, 2).contiguous().float()
    return o


def probe_period(dt):
    """(P, fraction bits f): x takes the values i + j 2^-f, i in 0 .. P - 1, j in 0 .. 2^f - 1.  A blended sample is a sum of (weights from
    {1, 1/4, 3/4}^2 x masks from {1, 1/2}) x these: a multiple of 2^-(5 + f) below P; with a bias in {-1, 0, 1} and a residual in {0, 1, 2}
    an output is a multiple of 2^-(5 + f) below P + 3.  bf16 has 8 significant bits: P = 4, f = 0 (below 8: 3 + 5 bits), the coarsest
    grid.  fp16 has 11: P = 32, f = 0 (below 64: 6 + 5 bits).  f16x2 and fp32: P = 4, f = 11 (below 8: 3 + 16 bits, which hi + lo and
    fp32's 24 bits hold): nearly every value needs its lo half, so a pack or a blend that loses it is not equal."""
    return {"bf16": (4, 0), "f16": (32, 0)}.get(dt, (4, 11))


@functools.lru_cache(maxsize=None)
def probe_case(N, C, H, W, Co, stride, dt, kind="plain", with_res=False):
    """(x, off, mask, w, b, res): equalities.  x[n, c, y, x] = (coordinate + n + c // 2) % P (+ a fraction (37 coordinate + 11 c + 5 n) % 2^f
    of f bits, probe_period) with the coordinate y for even c and x for odd c: it encodes its own row and column in two groups of
    channels and differs between images and channels.  Output channel n has one
    weight of 1 at tap p % 9 of a channel of block p // 9, p = n % (9 blocks): every (tap, channel block) pair is probed, so output
    (m, n) IS one blended sample (+ bias + residual), and a failure names pixel, tap and channel (probe_where).  Offsets: probe_offsets;
    masks 1 and 1/2.  kind "wild": +-1e9, +-3e38, +-inf and NaN in dy or dx of every seventh (pixel, tap); "mask0": mask 0 on taps 1, 4, 8.
    Asserted: every column element and every output is exact in `dt`."""
    P, fb = probe_period(dt)
    Ho, Wo = out_hw(H, W, stride)
    n, c, y, xx = torch.meshgrid(torch.arange(N), torch.arange(C), torch.arange(H), torch.arange(W), indexing="ij")
    co = torch.where(c % 2 == 0, y, xx)
    x = ((co + n + c // 2) % P).float() + ((37 * co + 11 * c + 5 * n) % (1 << fb)).float() / (1 << fb)
    cb = bke(dt)
    npairs = 9 * (C // cb)
    assert Co >= npairs
    w = torch.zeros(Co, C, 3, 3)
    for j in range(Co):
        tap, ch = probe_where(j, C, dt)
        w[j, ch, tap // 3, tap % 3] = 1.0
    b = (torch.arange(Co) % 3 - 1).float()
    off = probe_offsets(N, H, W, stride)
    m = torch.arange(N * Ho * Wo)[:, None]
    t = torch.arange(9)[None, :]
    mask = torch.where((m + t) % 2 == 0, 1.0, 0.5).reshape(N, Ho, Wo, 9).permute(0, 3, 1, 2).contiguous()
    wild = None
    if kind == "wild":
        hit = ((m * 9 + t) % 7 == 3)
        val = torch.tensor(WILD)[(m * 9 + t) // 7 % 7]
        axis = ((m + t) % 2)                                       # which of dy / dx goes wild
        o = off.permute(0, 2, 3, 1).reshape(-1, 9, 2).clone()
        wild = torch.zeros_like(o, dtype=torch.bool)
        for ax in (0, 1):
            sel = hit & (axis == ax)
            o[..., ax] = torch.where(sel, val, o[..., ax])
            wild[..., ax] = sel
        off = o.reshape(N, Ho, Wo, 18).permute(0, 3, 1, 2).contiguous()
        wild = wild.reshape(N, Ho, Wo, 18).permute(0, 3, 1, 2)
    elif kind == "mask0":
        mask[:, [1, 4, 8]] = 0.0
    res = (torch.arange(N * Co * Ho * Wo).reshape(N, Co, Ho, Wo) % 3).float() if with_res else None
    assert_grid(off, mask, stride, wild)
    cols, _ = sample_columns(x, off, mask, stride)
    assert torch.equal(round_to(cols.float(), dt).double(), cols), "a probe sample is not exact in the type"
    ref = dcn_ref(x, off, mask, w, b, res, stride)
    assert torch.equal(round_to(ref.float(), dt).double(), ref), "a probe output is not exact in the type"
    return x, off, mask, w, b, res


def probe_where(j, C, dt):
    """(tap, channel) that output channel j of a probe case reads."""
    cb = bke(dt)
    npairs = 9 * (C // cb)
    p = j % npairs
    return p % 9, (p // 9) * cb + (5 * (j // npairs) + j) % cb


def _snap(t, grid):
    return torch.round(t / grid) * grid


@functools.lru_cache(maxsize=None)
def value_case(N, C, H, W, Co, stride, dt, seed, band=False, with_res=False):
    """(x, off, mask, w, b, res): bounded.  Gaussian x, w / sqrt(9 C) and residual, rounded to `dt`; offsets N(0, 3) and masks U(0, 1) snapped
    to their grids.  band: every sample is sent to within one pixel of one of the four border lines of its axis (-1, 0, L - 1, L), where the
    corner predicates decide; a border more than 64 pixels away keeps the Gaussian offset."""
    g = _gen(seed)
    Ho, Wo = out_hw(H, W, stride)
    x = round_to(torch.randn(N, C, H, W, generator=g), dt)
    w = round_to(torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(9 * C), dt)
    b = torch.randn(Co, generator=g) * 0.5
    off = _snap(torch.randn(N, 18, Ho, Wo, generator=g) * 3.0, OFF_GRID).clamp(-OFF_MAX, OFF_MAX)
    mask = _snap(torch.rand(N, 9, Ho, Wo, generator=g), MASK_GRID)
    if band:
        by, bx, _ = _base(N, Ho, Wo, stride)
        o = _rows(off.double()).reshape(-1, 9, 2).clone()
        for ax, (L, base) in enumerate(((H, by), (W, bx))):
            line = torch.tensor([-1.0, 0.0, L - 1.0, float(L)], dtype=torch.float64)[torch.randint(0, 4, base.shape, generator=g)]
            d = line + _snap(torch.rand(base.shape, generator=g, dtype=torch.float64) * 2 - 1, OFF_GRID) - base
            o[..., ax] = torch.where(d.abs() <= OFF_MAX, d, o[..., ax])
        off = o.reshape(N, Ho, Wo, 18).permute(0, 3, 1, 2).contiguous().float()
    res = round_to(torch.randn(N, Co, Ho, Wo, generator=g), dt) if with_res else None
    assert_grid(off, mask, stride)
    return x, off, mask, w, b, res


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_dcn_sampling.py
def chans(dt):
    """(Cin with an odd number of K-steps, Cin with an even number): nk = 9 Cin / (64 or 32)."""
    return (64, 128) if dt in ("bf16", "f16") else (96, 64)


# name, N, H, W, stride, Cin selector (0: odd nk, 1: even nk), Co, residual.  With stride 1 the six ragged maps select patch_lw 2 .. 7; Co
# selects the 128-column build with an N tail (72), exact (128) and with three tiles (320), and the 256-column build likewise (200, 256, 512).
MAPS = (
    ("33x3", 2, 33, 3, 1, 0, 72, False),
    ("9x17", 3, 9, 17, 1, 1, 128, False),
    ("10x13", 2, 10, 13, 1, 0, 320, True),
    ("3x65", 2, 3, 65, 1, 1, 200, False),
    ("2x130", 2, 2, 130, 1, 0, 256, False),
    ("1x129", 3, 1, 129, 1, 1, 512, False),
    ("13x19s2", 2, 13, 19, 2, 0, 128, False),
)
MAP_LW = {"33x3": 2, "9x17": 3, "10x13": 4, "3x65": 5, "2x130": 6, "1x129": 7}
PERSIST = ("31x127", 2, 31, 127, 1, 64, 640)      # 2 x 31 patches of 1 x 128 pixels x 5 column tiles = 310 tiles on at most 304 CUs; Cin = 64 in every type


def cases(dt):
    """(name, N, C, H, W, Co, stride, with_res) of the main list."""
    return [(name, N, chans(dt)[ci], H, W, Co, stride, wr) for (name, N, H, W, stride, ci, Co, wr) in MAPS]


def small_case(dt):
    """The one small map per path of the wild, mask-0 and independence tests."""
    return ("9x17", 3, chans(dt)[0], 9, 17, 72, 1, False)


def plan_of(lib, dt, N, C, H, W, Co, stride, n_cu):
    """ocrvi_test_dcn_plan through the loaded library `lib`: (pipe?, BM, BN, patch_lw, tiles, grid, most tiles per workgroup, nk)."""
    import ctypes
    plan = (ctypes.c_int32 * 8)()
    rc = lib.ocrvi_test_dcn_plan(DT_CODE[dt], N, C, H, W, Co, stride, n_cu, plan)
    assert rc == 0, rc
    return tuple(plan)


def expect_plan(dt, N, C, H, W, Co, stride, n_cu):
    """What the case list means to reach, from the rules as the launchers' comments state them."""
    Ho, Wo = out_hw(H, W, stride)
    Np = -(-Co // 128) * 128
    bn = 256 if Np % 256 == 0 else 128
    M = N * Ho * Wo
    if dt in PIPE:
        lw = patch_lw(Ho, Wo)
        tiles = N * -(-Ho // (128 >> lw)) * -(-Wo // (1 << lw)) * (Np // bn)
        per = -(-tiles // min(tiles, n_cu))
        grid = -(-tiles // per)
        return (1, 128, bn, lw, tiles, grid, -(-tiles // grid), 9 * C // bke(dt))
    bm = 32 if (bn == 256 and -(-M // 64) * (Np // 256) < 3 * n_cu) else 64
    tiles = -(-M // bm) * (Np // bn)
    return (0, bm, bn, 0, tiles, tiles, 1, 9 * C // bke(dt))


def persist_case(dt):
    name, N, H, W, stride, C, Co = PERSIST
    return (name, N, C, H, W, Co, stride, False)


def gpu_list(dt):
    """(family, case, kind) of every launch whose output tests/test_gpu_dcn_sampling.py compares with the reference: both families on the
    main list, the wild and mask-0 probes on the small map, and -- on dcn_pipe -- both families on the map whose tiles outnumber the CUs."""
    runs = [(fam, c, "plain") for c in cases(dt) for fam in ("probe", "value")]
    runs += [("probe", small_case(dt), "wild"), ("probe", small_case(dt), "mask0")]
    if dt in PIPE:
        runs += [("probe", persist_case(dt), "plain"), ("value", persist_case(dt), "plain")]
    return runs


def inputs(family, dt, case, kind="plain"):
    """(x, off, mask, w, b, res) of one run of gpu_list.  Every third map of the value family is a band map."""
    name, N, C, H, W, Co, stride, wr = case
    if family == "probe":
        return probe_case(N, C, H, W, Co, stride, dt, kind, wr)
    names = [m[0] for m in MAPS]
    i = names.index(name) if name in names else 0
    return value_case(N, C, H, W, Co, stride, dt, 100 + i, name in names and i % 3 == 2, wr)


@functools.lru_cache(maxsize=None)
def ref_and_bound(family, dt, case, kind="plain"):
    """(reference, bound) of one run, computed once and shared; the probe family is held to equality and has no bound."""
    x, off, mask, w, b, res = inputs(family, dt, case, kind)
    stride = case[6]
    ref = dcn_ref(x, off, mask, w, b, res, stride)
    return ref, (dcn_bound(x, off, mask, w, b, res, stride, dt) if family == "value" else None)
