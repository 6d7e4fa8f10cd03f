"""Plain float64 statements of the memory-bound operations of csrc/kernels.hip: what tests/test_gpu_aux_kernels.py holds the HIP kernels
to, one short function each.  tests/test_aux_refs_cpu.py pins them to torch.nn.functional, to the oracle and to a reference-generated
golden, so that they are not a third opinion.  No GPU, no library: torch and numpy only.
The last section is attention (csrc/attention.hip): the float64 reference, a per-element error bound derived from the reference's own
softmax weights, and the input families of tests/test_gpu_attention.py; tests/test_attention_refs_cpu.py pins all three."""
import numpy as np
import torch
import torch.nn.functional as F


def f16x2_round(x: torch.Tensor) -> torch.Tensor:
    """The value an f16x2 element holds for the fp32 value x: hi = fp16(x), lo = fp16(x - hi), hi + lo in float32 (include/ocrvi.h)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.float() + lo.float()


def round_to(x: torch.Tensor, dt: str) -> torch.Tensor:
    """x rounded to something the element type `dt` holds exactly (float32 result)."""
    if dt == "bf16":
        return x.to(torch.bfloat16).float()
    if dt == "f16":
        return x.half().float()
    if dt == "f16x2":
        return f16x2_round(x)
    return x.float()


def half_ulp(y, dt):
    """Half an ulp of element type `dt` at the float64 values y: the error of one round-to-nearest."""
    a = y.abs().double()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -60)))
    if dt == "bf16":
        return torch.exp2(e - 8)                                   # 8 significant bits
    if dt == "f16":
        return torch.exp2(torch.clamp(e, min=-14.0) - 11)          # 11 significant bits; subnormal spacing 2^-24 below 2^-14
    if dt == "f16x2":
        return torch.clamp(a * 2.0 ** -23, min=2.0 ** -25)
    return torch.zeros_like(a)


def layernorm_ref(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the last dim (svtrv2.py:93,95,446): two-pass mean / biased variance.  Returns (y, sigma) in float64."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double(), var.sqrt().squeeze(-1)


def log_softmax_ref(x):
    """log_softmax over the last dim in float64.  A row holding NaN or +inf, or nothing but -inf, is NaN throughout (as torch's is)."""
    x = x.double()
    mx = x.max(-1, keepdim=True).values
    return (x - mx) - torch.log(torch.exp(x - mx).sum(-1, keepdim=True))


def maxpool_ref(x):
    """MaxPool2d(3, stride 2, padding 1) (backbone.py:34): the padding never wins, i.e. it is -inf."""
    N, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(x.double(), (1, 2, 1, 2), value=float("-inf"))
    taps = [p[:, :, r:r + 2 * OH:2, q:q + 2 * OW:2] for r in range(3) for q in range(3)]
    return torch.stack(taps).max(0).values


def frm_vertical_ref(kv, vq, B, H, W, D):
    """FRM vertical cross-attention with the precomputed query (svtrv2.py:236-243): kv [B*H*W][2D] (token = h*W + w; k | v), vq [D],
    heads of 32 -> out [B*W][D] in float64: softmax over the H keys of a column of q.k / sqrt(32), times v."""
    h = D // 32
    kv = kv.double().reshape(B, H, W, 2, h, 32)
    s = (kv[:, :, :, 0] * vq.double().reshape(h, 32)).sum(-1) * 32 ** -0.5      # [B, H, W, h]
    p = torch.softmax(s, 1)
    return (p.unsqueeze(-1) * kv[:, :, :, 1]).sum(1).reshape(B * W, D)


def _taps_align_corners(n_in, n_out):
    """Tap indices and the weight of the second tap of F.interpolate(mode="bilinear", align_corners=True) along one axis.  The source
    coordinate is float32((in - 1) / (out - 1)) * dst in float32, as ATen's fp32 kernel (and asf_blend_kernel) computes it; the rest is exact."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = src.astype(np.float64) - i0
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam)


def bilinear_up_ref(p, H, W):
    """F.interpolate(p, (H, W), mode="bilinear", align_corners=True) in float64 with the fp32 tap coordinates (neck.py:65)."""
    p = p.double()
    y0, y1, ly = _taps_align_corners(p.shape[2], H)
    x0, x1, lx = _taps_align_corners(p.shape[3], W)
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)
    rows = p[:, :, y0] * (1 - ly) + p[:, :, y1] * ly
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def asf_ref(p2, p3, p4, p5, w, b):
    """ScaleFeatureSelection.forward, the literal form of neck.py:57-79: upsample p3..p5 to p2's size, concatenate, 1x1 conv (w [4][1024],
    b [4]), softmax over the 4 scores, weighted sum.  Returns (fused, attention [N,4,H,W]) in float64."""
    H, W = p2.shape[-2:]
    ups = [p2.double()] + [bilinear_up_ref(p, H, W) for p in (p3, p4, p5)]
    score = torch.einsum("oc,nchw->nohw", w.double().reshape(4, 1024), torch.cat(ups, 1)) + b.double().view(1, 4, 1, 1)
    att = torch.softmax(score, 1)
    return sum(u * att[:, i:i + 1] for i, u in enumerate(ups)), att


def db_maps_ref(bin_logits, thresh_logits):
    """binary, thresh = sigmoid of the two logit maps (head.py:34,38) in float64."""
    return torch.sigmoid(bin_logits.double()), torch.sigmoid(thresh_logits.double())


def db_step_ref(binary, thresh, k):
    """The DB step function 1 / (1 + exp(-k (binary - thresh))) (head.py:28-30) in float64."""
    return torch.reciprocal(1 + torch.exp(-float(k) * (binary.double() - thresh.double())))


def ctc_collapse_ref(argmax_ids, blank=0):
    """Greedy CTC path of argmax ids [B][T] (svtrv2.py:559-566): collapse repeats, drop the blank -> (ids [B][T] padded with -1, lens [B])."""
    a = np.asarray(argmax_ids)
    ids = np.full(a.shape, -1, np.int32)
    lens = np.zeros(a.shape[0], np.int32)
    for b, row in enumerate(a):
        keep = [int(c) for t, c in enumerate(row) if c != blank and (t == 0 or c != row[t - 1])]
        ids[b, :len(keep)] = keep
        lens[b] = len(keep)
    return ids, lens


# ------------------------------------------------------------------------------------------------ attention (csrc/attention.hip)
ATTN_SCALE = 32 ** -0.5
U32 = 2.0 ** -24                                   # unit roundoff of fp32
# What attention.hip dispatches on (tests/test_attention_refs_cpu.py reads the same figures out of the source and compares):
ATTN_MAXT = (4, 5, 8, 15, 16, 30, 32)              # key-tile counts of the register-resident builds (attn_range)
ATTN_STREAM_ABOVE = 256                            # 16-bit types: the streaming kernel above this many keys (k_attention)
ATTN_CHUNK = 512                                   # 4-byte types: key chunks of at most this many keys (attn_chunks, attn_dt)
ATTN_MAX_KEYS = {"f32": 4096, "f16x2": 4096, "bf16": 1024, "f16": 1024}


def attention_chunks(N):
    """[(first key, key count)] of the launches attn_dt makes for N keys in a 4-byte type: one below ATTN_CHUNK, else cdiv(N, 512)
    chunks of align_up(cdiv(N, chunks), 32) keys (attn_chunks, attn_chunk_keys)."""
    if N <= ATTN_CHUNK:
        return [(0, N)]
    nc = (N + ATTN_CHUNK - 1) // ATTN_CHUNK
    ck = ((N + nc - 1) // nc + 31) // 32 * 32
    return [(c * ck, min(ck, N - c * ck)) for c in range(nc)]


def attention_plan(N, dt):
    """The kernel builds one call runs: [("stream", None, MASK)] or [("reg", MAXT, MASK)] per key chunk."""
    if dt in ("bf16", "f16") and N > ATTN_STREAM_ABOVE:
        return [("stream", None, N % 32 != 0)]
    plan = []
    for _, nk in attention_chunks(N):
        maxt = next(m for m in ATTN_MAXT if (nk + 15) // 16 <= m)
        plan.append(("reg", maxt, nk != 16 * maxt))
    return plan


def _qkv_heads(qkv, B, N, heads):
    q, k, v = qkv.double().reshape(B, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    return q, k, v                                                   # [B, heads, N, 32] each


def attention_ref(qkv, B, N, heads, scale=ATTN_SCALE):
    """softmax(q k^T / sqrt(32)) v in float64 on the packed layout of ocrvi_test_attention: qkv [B, N, 3 * heads * 32] =
    qkv.reshape(B, N, 3, heads, 32).  Returns (out [B, N, heads * 32], weights [B, heads, N, N])."""
    q, k, v = _qkv_heads(qkv, B, N, heads)
    w = torch.softmax((q @ k.transpose(-2, -1)) * scale, -1)
    return (w @ v).transpose(1, 2).reshape(B, N, heads * 32), w


def _weighted_l1(W, v, o, budget=1 << 24):
    """sum_j W_ij |v_jd - o_id| for W [B, h, N, N], v and o [B, h, N, 32], in blocks of queries."""
    B, h, N, _ = W.shape
    qb = max(1, budget // (B * h * N * 32))
    out = torch.empty_like(o)
    for i in range(0, N, qb):
        d = (v[:, :, None, :, :] - o[:, :, i:i + qb, None, :]).abs()
        out[:, :, i:i + qb] = torch.einsum("bhqj,bhqjd->bhqd", W[:, :, i:i + qb], d)
    return out


def attn_acc_terms(K, dt):
    """(PV, row sum): the error of a K-term fp32 accumulation relative to the sum of the terms' magnitudes, in units of 2^-24.  The
    order in which an MFMA adds its 4 (fp32) or 32 (16-bit) products to the accumulator is not in the source, and the worst case over
    all orders, K, is far from what any order gives (1000 ulps at 1000 keys), so these are MEASURED, float64 against an fp32
    evaluation of the same sums on the CPU in the least favourable order there is, one sequential chain over all keys
    (test_attention_refs_cpu.py repeats the measurement): over 256 rows per case, q x tau in (1, 4, 16),
        K = 16: PV 6.1, sum 4.1     K = 100: PV 14.1, sum 9.1     K = 512: PV 24.4, sum 35.7     K = 1024: PV 29.7, sum 61.4
    (chains of 4- or 32-term blocks, which is closer to the hardware: PV 17.9 and 8.6 at K = 1024).  They grow as sqrt(K); twice the
    measured figures are covered by 4 + 2 sqrt(K) (12 / 24 / 49.3 / 68) and 4 + 4 sqrt(K) (20 / 44 / 94.5 / 132), capped by the
    worst case K.  f16x2 accumulates three products per key (hi lo, lo hi, hi hi): 3 K terms in the PV chain."""
    kpv = 3 * K if dt == "f16x2" else K
    return min(kpv, 4 + 2 * kpv ** 0.5), min(K, 4 + 4 * K ** 0.5)


def attention_bound(qkv, B, N, heads, dt, ref=None, device=None):
    """Per-element bound [B, N, heads * 32] on |kernel - attention_ref| for inputs the element type `dt` holds exactly, from the
    reference's own weights w_ij and output o_i.  With u = 2^-24 and c = 32^-0.5:

        |err_i| <= sum_j (w_ij e_ij + P0 max_j w_ij) |v_j - o_i| / (1 - max_j e_ij - N P0)  +  a sum_j w_ij |v_j|  +  half an ulp of dt

    A kernel computes p_j = exp2(fma(s_j, c2, -fl(max c2))) (c2 = c log2 e in fp32), rounds it to the element type, and returns
    (sum_j p_j v_j) / (sum_j p_j) with the SAME rounded p_j in both sums.  A relative error e_j of p_j therefore moves the output by
    sum_j w_j e_j (v_j - o) / sum_j w_j (1 + e_j) -- exactly, since sum_j w_j (v_j - o) = 0 -- which is the first term; anything common to
    a row (the rounding of max c2, f16x2's factor 2^12) cancels.  e_ij = rP + 2 c g M_i + k |a_ij| + x:
      rP   rounding p to the type, half an ulp at the bottom of a binade: 2^-8 bf16 (8 significant bits), 2^-11 fp16 (11 bits), 2^-22
           f16x2 (hi = RNE(p), lo = RNE(p - hi): 2^-11 of 2^-11), 0 fp32.  (2^-9 and 2^-12 hold at the top of a binade only: an fp32
           emulation of the kernel on the CPU exceeds a bound built on them by 1.39 x in bf16 at tau = 4, as the kernel does);
      g    error of the 32-term dot s_j relative to M_ij = sum_d |q_id k_jd|, M_i its maximum over j: 32 u for any order of fp32
           additions (16-bit products are exact in fp32; the fp32 build is a chain of eight 4-term MFMAs); f16x2 adds three such
           products and drops lo lo <= 2^-22 = 4 u: 100 u.  (Measured on the CPU, sequential fp32: 5.3 u.)  Times c for the exponent,
           times 2: the error of key j and that of the key the row is normalised by;
      k    a_ij = (s_ij - max_j s_ij) c <= 0 is the exponent: the fma rounds it once (u |a|) and c2 differs from c log2 e by
           0.151 u (computed): k = 2 u.  w_ij |a_ij| <= w_max / e, so this charges the keys that carry weight, not the far tail;
      x    v_exp_f32, 1 ulp by the ISA manual (the CPU's fp32 exp2 measures 1.74 u): 4 u; chunked sequences (4-byte types above 512
           keys) take a second exp2 for the chunk weight, exp2((m_c - m) c2), whose argument error is again within k |a_ij|: 8 u.
    P0 is the absolute error of a rounded p below the type's normal range: 2^-25 in fp16, 2^-37 in f16x2 (2^-25 of 4096 p), and
    2^-126 for the flush of v_exp_f32 everywhere; p_max is within 2^-13 of 1 (|fl(max c2) - max c2| <= ulp / 2 <= 2^-14 below 2^11).
    a = (A_pv + A_sum + 4) u + f16x2's dropped lo lo of P V (4 u) + (chunks + 4) u: attn_acc_terms for the longest chain (the keys of
    one chunk, or all of them), the product, the division (correctly rounded: no fast-math; 2 u allowed) and the final product;
    the merge adds one product and one addition per chunk and its own division.  These scale o_i, and |o_i| <= sum_j w_ij |v_j|.
    The output rounding is taken at |o| + the arithmetic error.
    `device`: where to evaluate the bound (the same float64 torch code; the sum over (i, j, d) is 32 N^2 terms per head); the
    reference itself is not moved."""
    out, w = ref if ref is not None else attention_ref(qkv, B, N, heads)
    q, k, v = _qkv_heads(qkv, B, N, heads)
    if device is not None:
        out, w, q, k, v = (t.to(device) for t in (out, w, q, k, v))
    split, four = dt == "f16x2", dt in ("f32", "f16x2")
    chunks = attention_chunks(N) if four else [(0, N)]
    s = (q @ k.transpose(-2, -1)) * ATTN_SCALE
    a = (s - s.max(-1, keepdim=True).values).abs()
    M = (q.abs() @ k.abs().transpose(-2, -1)).max(-1).values
    rP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f16x2": 2.0 ** -22, "f32": 0.0}[dt]
    P0 = ({"f16": 2.0 ** -25, "f16x2": 2.0 ** -37}.get(dt, 0.0) + 2.0 ** -126) * (1 + 2.0 ** -12)
    g = (100 if split else 32) * U32
    e_row = rP + 2 * ATTN_SCALE * g * M + (8 if len(chunks) > 1 else 4) * U32
    E = a.mul_(2 * U32).add_(e_row.unsqueeze(-1))
    den = 1 - E.max(-1).values - N * P0
    assert float(den.min()) > 0.5
    W2 = E.mul_(w).add_(P0 * w.max(-1, keepdim=True).values)
    o = out.reshape(B, N, heads, 32).transpose(1, 2)
    t1 = _weighted_l1(W2, v, o) / den.unsqueeze(-1)
    apv, asum = attn_acc_terms(max(nk for _, nk in chunks), dt)
    acc = (apv + asum + 4 + (4 if split else 0) + (len(chunks) + 4 if len(chunks) > 1 else 0)) * U32
    arith = (t1 + acc * (w @ v.abs())).transpose(1, 2).reshape(B, N, heads * 32)
    return (arith + half_ulp(out.abs() + arith, dt)).cpu()


# ---- input families of the attention tests.  Every one returns qkv [B, N, 3 * heads * 32] (float32) already rounded to `dt`.
def _pack_qkv(q, k, v, dt):
    B, h, N, _ = q.shape
    return round_to(torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * h * 32).float(), dt)


def attn_routing(B, N, heads, dt, perm, seed):
    """Query i attends to key pi(i) alone.  Keys are sign codes of the key index: `copies` copies of the `nb` low bits of j as +-a (the
    other channels 0), q_i = k_pi(i); two keys differ in a bit, so the scores (a^2 copies (nb - 2 hamming)) have a gap of at least
    2 a^2 copies: 600 for (nb, copies, a) = (10, 3, 10) up to 1024 keys, 676 for (12, 2, 13) up to 4096 -- the runner-up's exp2
    argument is below -153 (-172).  Every entry is a small integer.  v is random with no zero component (and not fp16-representable in
    the 4-byte types).  Returns (qkv, pi [B, heads, N])."""
    g = torch.Generator().manual_seed(seed)
    nb, copies, a = (10, 3, 10.0) if N <= 1024 else (12, 2, 13.0)
    assert N <= 1 << nb
    j = torch.arange(N)
    code = torch.zeros(N, 32)
    for c in range(copies):
        for b in range(nb):
            code[:, c * nb + b] = a * (2.0 * ((j >> b) & 1) - 1.0)
    if perm == "identity":
        pi = j.expand(B, heads, N)
    elif perm == "reversal":
        pi = (N - 1 - j).expand(B, heads, N)
    else:
        pi = torch.stack([torch.randperm(N, generator=g) for _ in range(B * heads)]).reshape(B, heads, N)
    k = code.expand(B, heads, N, 32)
    q = code[pi]
    v = torch.randn(B, heads, N, 32, generator=g)
    v = torch.where(v.abs() < 2.0 ** -6, torch.full_like(v, 0.75), v)
    return _pack_qkv(q, k, v, dt), pi


def attn_temperature(B, N, heads, dt, tau, seed):
    """randn q, k, v with q times tau: tau = 1 is the flat rows of test_attention_kernel, 64 nearly one-hot rows with real runner-ups."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(3, B, heads, N, 32, generator=g)
    return _pack_qkv(q * tau, k, v, dt)


def attn_shift(B, N, heads, dt, shift, seed):
    """Flat randn rows whose scores all move by `shift` (+-45 or +-450 after scaling): channel 0 of every key is 16 and of every query
    +-16 (16 * 16 / sqrt(32) = 45.25) or +-160.  The zero-filled padding keys past N score 0: far above every real key when the shift is negative."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(3, B, heads, N, 32, generator=g)
    k[..., 0] = 16.0
    q[..., 0] = {45: 16.0, 450: 160.0}[abs(shift)] * (1 if shift > 0 else -1)
    return _pack_qkv(q, k, v, dt)


def attn_peak_positions(N, dt):
    """Keys to raise: the corners of lane groups, tiles and 32-key steps, the last key, the first key of the last tile, and the last key
    of chunk 0 / the first of chunk 1 where the type chunks the sequence."""
    pos = [0, 3, 4, 15, 16, 31, 32, N - 1, 16 * ((N - 1) // 16)]
    ch = attention_chunks(N) if dt in ("f32", "f16x2") else [(0, N)]
    if len(ch) > 1:
        pos += [ch[0][1] - 1, ch[1][0]]
    return sorted({p for p in pos if 0 <= p < N})


def attn_peak(N, heads, dt, positions, seed):
    """One sequence per entry of `positions`: flat randn rows in which that key alone is raised -- channel 0 is 4 in every query, 0 in
    every key but the raised one, where it is (ln N + 0.5) sqrt(32) / 4 -- to a weight of about one half in every row."""
    g = torch.Generator().manual_seed(seed)
    B = len(positions)
    q, k, v = torch.randn(3, B, heads, N, 32, generator=g)
    q[..., 0] = 4.0
    k[..., 0] = 0.0
    for b, p in enumerate(positions):
        k[b, :, p, 0] = (np.log(N) + 0.5) * 32 ** 0.5 / 4
    return _pack_qkv(q, k, v, dt)


ATTN_LENGTHS = (16, 64, 70, 80, 100, 128, 200, 240, 250, 256, 257, 300, 480, 500, 512, 513, 640, 960, 1000, 1024)
ATTN_LENGTHS_4BYTE = (1025, 1537, 2000, 4096)
ATTN_GRIDS = ((1, 1), (1, 3), (7, 1), (3, 4), (64, 8))      # B x heads: 1, 3, 7, 12 and 512 (sequence, head) pairs


def attn_lengths(dt):
    return ATTN_LENGTHS + (ATTN_LENGTHS_4BYTE if dt in ("f32", "f16x2") else ())


def attn_grid(N, i):
    """The i-th B x heads of ATTN_GRIDS whose float64 weights [B, heads, N, N] stay within 2^23 elements (64 MB); one or two
    (sequence, head) pairs above 1024 keys."""
    grids = ATTN_GRIDS if N <= 1024 else ((1, 1), (2, 1), (1, 2))
    ok = [gr for gr in grids if gr[0] * gr[1] * N * N <= 1 << 23] or [(1, 1)]
    return ok[i % len(ok)]


def attn_families(N, dt, li=0, grid=None):
    """[(tag, B, heads, builder)]: the bound-checked input families at length N; builder() -> qkv.  `li` rotates the grids of ATTN_GRIDS
    over the families; `grid` = (B, heads) fixes one for all (the peak family has one sequence per raised key and one head)."""
    fams = []
    pick = (lambda N, i: grid) if grid else attn_grid
    for i, tau in enumerate((1, 4, 16, 64)):
        B, h = pick(N, li + i)
        fams.append((f"tau={tau}", B, h, lambda B=B, h=h, tau=tau: attn_temperature(B, N, h, dt, tau, 11 * N + tau)))
    for i, sh in enumerate((-45, -450, 45, 450)):
        B, h = pick(N, li + i + 1)
        fams.append((f"shift={sh}", B, h, lambda B=B, h=h, sh=sh: attn_shift(B, N, h, dt, sh, 13 * N + abs(sh) + (sh > 0))))
    for i, perm in enumerate(("identity", "reversal", "random")):
        B, h = pick(N, li + i + 2)
        fams.append((f"route={perm}", B, h, lambda B=B, h=h, perm=perm, i=i: attn_routing(B, N, h, dt, perm, 17 * N + i)[0]))
    pos = attn_peak_positions(N, dt)
    per = max(1, min(len(pos), (1 << 23) // (N * N)))
    for i in range(0, len(pos), per):
        grp = pos[i:i + per]
        fams.append((f"peak@{','.join(map(str, grp))}", len(grp), 1, lambda grp=grp: attn_peak(N, 1, dt, grp, 19 * N + grp[0])))
    return fams
