"""The fused MixingBlock MLP (csrc/mlp_fused.hip for bf16 / fp16, csrc/mlp_x2.hip for f16x2) in plain float64, a per-element error bound
derived from the reference's own intermediates, an fp32 emulation of the kernels' order of operations, and the input families of
tests/test_gpu_mlp_fused.py.  tests/test_mlp_refs_cpu.py shows on the CPU that the emulation stays inside the bound on every family and
that sixteen wrong kernels land 10x or more outside it.  No GPU, no library: torch and numpy only.

    x_new = x + b2 + w2 gelu(w1 LN(x; ln_g, ln_b) + b1)            xn = LN(x_new; next_g, next_b) | x_new rounded to T | nothing

Routed weights (routed_weights): w1 has one non-zero per row, w2 four per row, so
    x_new[t, n] = x[t, n] + b2[n] + sum_{j < 4} c_h gelu(a_h LN(x)[t, pi1(h)] + b1[h]),   h = H[n, j]
and an index slip in b1, b2, the norm vectors, the fc2 k-slot permutation or the chunk order moves identifiable outputs by order 0.1."""
import math

import numpy as np
import torch

from aux_refs import U32, half_ulp, round_to

EPS = 1e-5
MODES = ("ln", "cast", "none")
CHUNK = {"bf16": 64, "f16": 64, "f16x2": 32}          # hidden units per chunk of the software pipeline (NCH = 4 D / CHUNK)
COEF = (0.5, 1.0, 2.0, 3.0)                            # |a_h|, |c_h|: exact in bf16, fp16 and f16x2 (the f16x2 pack scale is 2^12 for them)
GELU_XMIN = -0.7517915246                              # argmin of x Phi(x): gelu' = Phi(x) + x phi(x) has its one zero there
ROW_KINDS = ("randn", "const", "mean10", "mean100", "mean1000", "mean3000", "tiny", "outlier")


def gelu64(x):
    """x Phi(x) with Phi(x) = erfc(-x / sqrt 2) / 2: accurate in the negative tail, where 1 + erf cancels."""
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def _ln64(v, g, b):
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = d.pow(2).mean(-1, keepdim=True)
    return d * torch.rsqrt(var + EPS) * g.double() + b.double(), d, var


def mlp_trace(x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode):
    """Every intermediate of the block in float64 (what mlp_bound is computed from)."""
    x = x.double()
    z, d, var = _ln64(x, ln_g, ln_b)
    pre = z @ w1.double().t() + b1.double()
    h = gelu64(pre)
    o = h @ w2.double().t()
    y = x + b2.double() + o
    xn = {"ln": lambda: _ln64(y, next_g, next_b)[0], "cast": lambda: y.clone(), "none": lambda: None}[mode]()
    return {"x": x, "z": z, "pre": pre, "h": h, "o": o, "y": y, "xn": xn}


def mlp_ref(x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode):
    """(x_new, xn) in float64; xn is None for mode "none"."""
    t = mlp_trace(x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode)
    return t["y"], t["xn"]


# ------------------------------------------------------------------------------------------------ the bound
def _exact_rows(v, e_in, D):
    """Rows for which the kernels' LayerNorm is exact: every entry the same integer c with |c| D < 2^24 and no input error.  Every
    partial sum is then an integer below 2^24, so the mean is c, every difference is 0 and the output is fl(0 rstd g + b) = b."""
    c = v[:, :1]
    return ((v == c).all(-1, keepdim=True) & (c == c.round()) & (c.abs() * D < 2.0 ** 24) & (e_in == 0).all(-1, keepdim=True))


def _ln_err(v, e_in, g, b):
    """(z, e): LayerNorm(v) in float64 and a bound on |kernel - z| for a kernel that holds v + delta, |delta| <= e_in, in fp32 and
    computes as both kernels do: a two-pass mean and variance, each a sum of D / 4 terms per lane in sequence followed by two
    shuffle-adds (depth n = D / 4 + 2), rstd = rsqrtf(var + eps), out = (v - mean) rstd g + b.  u = 2^-24.
      mean   |dm| <= mean(e_in) + (n + 1) u mean(|v| + e_in): the worst case of a depth-n fp32 sum, n u sum |v_i|, and the division;
      d_i    |dd_i| <= e_in_i + dm + u |d_i| (one subtraction);
      var    |dvar| <= mean(2 |d| dd + dd^2) + (n + 3) u var: the perturbed terms, then the squares, the depth-n sum and the division
             (the part of dd common to a row would cancel to first order, sum d_i = 0; it is not used);
      rstd   r = (dvar + u (var + eps)) / (var + eps); |(1 + r)^-1/2 - 1| <= r / (2 (1 - r)); v_rsq_f32 is 1 ulp = 2 u, taken twice: rel
      out    |g| rstd (dd (1 + rel) + |d| rel) + 3 u |d rstd g| (two products, second order) + u |z| (the last addition)."""
    D = v.shape[-1]
    n = D // 4 + 2
    g, b = g.double(), b.double()
    z, d, var = _ln64(v, g, b)
    s2 = var + EPS
    rstd = torch.rsqrt(s2)
    dm = e_in.mean(-1, keepdim=True) + (n + 1) * U32 * (v.abs() + e_in).mean(-1, keepdim=True)
    dd = e_in + dm + U32 * (d.abs() + e_in + dm)
    dvar = (2 * d.abs() * dd + dd * dd).mean(-1, keepdim=True)
    dvar = dvar + (n + 3) * U32 * (var + dvar)
    r = (dvar + U32 * s2) / s2
    assert float(r.max()) < 0.5, float(r.max())
    rel = 0.5 * r / (1 - r) + 4 * U32
    e = g.abs() * rstd * (dd * (1 + rel) + d.abs() * rel) + 3 * U32 * (d * rstd * g).abs() + U32 * z.abs()
    return z, torch.where(_exact_rows(v, e_in, D), torch.zeros_like(e), e)


def _rounded(v, e, dt):
    """|T(v + delta) - v| for |delta| <= e: e + half an ulp at |v| + e; where e is exactly 0 the rounding error itself."""
    exact = (round_to(v.float(), dt).double() - v).abs() + (v.float().double() - v).abs()
    return torch.where(e == 0, exact, e + half_ulp(v.abs() + e, dt))


def _gelu_err(pre, e_pre):
    """|gelu_erf(pre + delta) - gelu64(pre)| for |delta| <= e_pre: the image of the interval under gelu64, plus the error of common.h's
    gelu_erf = max(x, 0) - |x| h, h = q(t) t E, t = rcp(1 + p |x| / sqrt 2), E = exp2(-x^2 log2(e) / 2), q the Horner form of A&S 7.1.26:
      interval  gelu64 decreases left of GELU_XMIN and increases right of it: the image's extremes are at the ends or at GELU_XMIN;
      A&S       |erfc error| <= 1.5e-7 (7.1.26), so |dh| <= 0.75e-7; also 0 < h, erfc / 2 <= E / 2 (q t falls from 0.5), so |dh| <= E / 2;
      fp32      t: one fma (u), the rounded constant (u), v_rcp_f32 1 ulp (2 u): 4 u.  q: four fmas, |error| <= 8 u S0 + 4 u S1 with
                S0 = sum |c_k| t^k <= 2.24, S1 = sum k |c_k| t^k <= 5.87 (the half coefficients of common.h at t = 1): 41.4 u.  h = q t E adds
                t's 4 u, two products 2 u, v_exp_f32 1 ulp = 2 u and its argument (two products and the constant, 3 u |arg| ln 2), times
                h <= t E / 2 and h |arg| <= 0.75 t E x^2 / 2:  |dh| <= t E (41.4 + 4 + 0.25 x^2 + ...) u -> t E (48 + 0.75 x^2) u with t, E at the
                near end of the interval and x at the far end;
      last      the product |x| h (u |x| E / 2) and the subtraction (u |result|).  (A v_exp_f32 result flushed to zero is below 2^-126.)"""
    lo, hi = pre - e_pre, pre + e_pre
    g0 = gelu64(pre)
    img = torch.maximum((gelu64(lo) - g0).abs(), (gelu64(hi) - g0).abs())
    gmin = float(gelu64(torch.tensor(GELU_XMIN, dtype=torch.float64)))
    img = torch.where((lo < GELU_XMIN) & (hi > GELU_XMIN), torch.maximum(img, (gmin - g0).abs()), img)
    am, aM = torch.clamp(pre.abs() - e_pre, min=0.0), pre.abs() + e_pre
    E = torch.exp(-0.5 * am * am)
    t = 1.0 / (1.0 + 0.3275911 / math.sqrt(2.0) * am)
    dh = torch.clamp(0.5 * E, max=0.75e-7) + t * E * (48 + 0.75 * aM * aM) * U32
    return img + aM * dh + U32 * (0.5 * aM * E + g0.abs() + img)


def mlp_bound(x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode, dt, ref=None):
    """(bound on |x_new - ref|, bound on |xn - ref| or None), per element, for either kernel in element type `dt`, from the float64
    intermediates `ref` (mlp_trace; computed here if None).  The weights must be exact in `dt`.  With u = 2^-24, step by step:
      LN        _ln_err with an exact input; rounded to T: half an ulp at |z| + e (_rounded; f16x2: hi = RNE(z), lo = RNE(z - hi)).
                A constant integer row gives z = ln_b exactly, and then only ln_b's own rounding to T is charged;
      fc1       the products are exact in fp32 (at most 11 x 11 significant bits); n1 - 1 additions of non-zero terms, n1 = the most
                non-zeros in a row of w1 (three products per weight in f16x2: lo hi, hi lo, hi hi), 2 u each relative to sum |w| |z|: the
                order and the rounding of the additions inside an MFMA are not documented, 1 ulp covers a truncating adder.  f16x2 drops
                lo lo <= 2^-22 |w| |z| = 4 u (zero for weights without a lo half; kept for generality);  + b1: one rounding, u |pre|;
      gelu      _gelu_err;  rounded to T: half an ulp, with fp16's subnormal spacing (aux_refs.half_ulp: 2^-25 in fp16 and for f16x2's lo);
      fc2       as fc1 with the four terms of a routed row (n2 - 1 additions);
      out       fl(o ws2 + b2 + x): two additions in either association, u (|o| + |b2| + |x|) + u |x_new|;
      xn        "cast": half an ulp at |x_new| + e.  "ln": _ln_err with the input error e (the statistics are taken over x_new as the kernel
                holds it), then half an ulp of T."""
    p = (x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode)
    tr = ref if ref is not None else mlp_trace(*p)
    split = dt == "f16x2"
    W1, W2 = w1.double().abs(), w2.double().abs()
    for w in (w1, w2):
        assert torch.equal(round_to(w.float(), dt), w.float()), "weights must be exact in the element type"
    terms = 3 if split else 1
    n1 = int((w1 != 0).sum(-1).max()) * terms
    n2 = int((w2 != 0).sum(-1).max()) * terms
    ll = 4 * U32 if split else 0.0
    z, e_z = _ln_err(tr["x"], torch.zeros_like(tr["x"]), ln_g, ln_b)
    e_zT = _rounded(z, e_z, dt)
    zmag = (z.abs() + e_zT) @ W1.t()
    e_pre = e_zT @ W1.t() + (2 * max(n1 - 1, 0) * U32 + ll) * zmag
    e_pre = e_pre + U32 * (tr["pre"].abs() + e_pre)
    e_h = _gelu_err(tr["pre"], e_pre)
    e_hT = e_h + half_ulp(tr["h"].abs() + e_h, dt)
    hmag = (tr["h"].abs() + e_hT) @ W2.t()
    e_o = e_hT @ W2.t() + (2 * max(n2 - 1, 0) * U32 + ll) * hmag
    e_y = e_o + U32 * (tr["o"].abs() + e_o + b2.double().abs() + tr["x"].abs()) + U32 * (tr["y"].abs() + e_o)
    if mode == "none":
        return e_y, None
    if mode == "cast":
        return e_y, e_y + half_ulp(tr["y"].abs() + e_y, dt)
    z2, e2 = _ln_err(tr["y"], e_y, next_g, next_b)
    return e_y, e2 + half_ulp(z2.abs() + e2, dt)


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def gelu_erf32(x):
    """common.h's gelu_erf in float32 (separate multiply and add where the kernel has an fma)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ax = x.abs()
    t = 1.0 / (ax * f(0.3275911 * 0.70710678118654752440) + 1.0)
    q = f(0.5 * 1.061405429) * t + f(0.5 * -1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        q = q * t + f(0.5 * c)
    h = q * t * torch.exp2(x * x * f(-0.5 * 1.44269504088896340736))
    return torch.clamp(x, min=0.0) - ax * h


def _ln32(v, g, b, mut, row0_last=False):
    D = v.shape[-1]
    mean = v.sum(-1, keepdim=True) / D
    if "one_pass_var" in mut:
        var = (v * v).sum(-1, keepdim=True) / D - mean * mean
    else:
        var = ((v - mean) ** 2).sum(-1, keepdim=True) / D
    rstd = 1.0 / (var.sqrt() + 1e-5) if "eps_outside" in mut else torch.rsqrt(var + 1e-5)
    if row0_last:
        mean, rstd = mean.clone(), rstd.clone()
        mean[-1], rstd[-1] = mean[0], rstd[0]
    return (v - mean) * rstd * g + b


def _x2_scale(w):
    """mlp_x2.hip's pack scale: the power of two that puts the largest |w| into [2^13, 2^14) (1 for an all-zero matrix)."""
    mx = float(w.abs().max())
    return 2.0 ** (14 - math.frexp(mx)[1]) if mx > 0 else 1.0


def _mfma_chain(a, w, dt, acc0=None):
    """a [M, K] (values T holds) times w [N, K]^T as a chain of MFMAs over 32 consecutive k each, the accumulator rounded to fp32 once per
    MFMA (products and the sum inside one MFMA exact: an assumption, the adder's inner order and rounding are not documented, and the
    16-bit kernel's fc1 takes its 32 k of a 64-wide K-step from four 8-element groups, not consecutively).  f16x2 runs mlp_x2.hip's
    three products per step in its order -- w_lo a_hi, w_hi a_lo, w_hi a_hi -- on weights scaled by _x2_scale and split into fp16 halves,
    and undoes the scale (a power of two) at the end, as the kernel does in the fma that adds the bias.  acc0: what the accumulators start
    at instead of zero, in the result's scale ([N] or [M, N]; the ring GEMM's fp32 and f16x2 builds start at the bias, tests/gemm_refs.py)."""
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    a64, w64 = a.double(), w.double()
    if acc0 is not None:
        acc = (acc.double() + acc0.double() * (_x2_scale(w) if dt == "f16x2" else 1.0)).float()
    if dt != "f16x2":
        for k in range(0, K, 32):
            acc = (acc.double() + a64[:, k:k + 32] @ w64[:, k:k + 32].t()).float()
        return acc
    s = _x2_scale(w)
    wH = (w64 * s).float().half().double()
    wL = (w64 * s - wH).float().half().double()
    aH = a.half().double()
    aL = (a64 - aH).float().half().double()
    for k in range(0, K, 32):
        for wp, ap in ((wL, aH), (wH, aL), (wH, aH)):
            acc = (acc.double() + ap[:, k:k + 32] @ wp[:, k:k + 32].t()).float()
    return (acc.double() / s).float()


def mlp_emulate(x, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, mode, dt, mut=()):
    """The kernel of element type `dt` in float32, rounded to T where it rounds (the LN output and h; xn): (x_new, xn) float32.  The two
    kernels differ in _mfma_chain (one product per step, or f16x2's three on split, scaled operands); LN, GELU and the epilogue are the
    same arithmetic in both.  What is NOT followed: the lanes' summation order in the LN statistics (torch's fp32 sum), fmas (separate
    multiply and add), and the order inside an MFMA.  With routed coefficients the weights have no lo half, so f16x2's w_lo products are
    zeros in every case of these files: lo-half weights are exercised only by the dense test_mlp_fused_kernel_f16x2.
    `mut`: names of deliberate errors in the arithmetic -- "one_pass_var", "eps_outside", "row0_stats" (the last token takes row 0's
    mean and rstd), "norm2_branch" (the epilogue norm sees the branch without the residual), "gelu_tanh", "round_h_first" (fc1's
    accumulator is rounded to T before b1 is added).  Errors in an index are made by permuting the parameters instead
    (tests/test_mlp_refs_cpu.py)."""
    x = x.float()
    zT = round_to(_ln32(x, ln_g.float(), ln_b.float(), mut, "row0_stats" in mut), dt)
    acc = _mfma_chain(zT, w1.float(), dt)
    if "round_h_first" in mut:
        acc = round_to(acc, dt)
    pre = acc + b1.float()
    h = torch.nn.functional.gelu(pre, approximate="tanh") if "gelu_tanh" in mut else gelu_erf32(pre)
    o = _mfma_chain(round_to(h, dt), w2.float(), dt)
    y = o + (b2.float() + x)
    if mode == "none":
        return y, None
    if mode == "cast":
        return y, round_to(y, dt)
    src = o + b2.float() if "norm2_branch" in mut else y
    return y, round_to(_ln32(src, next_g.float(), next_b.float(), mut), dt)


# ------------------------------------------------------------------------------------------------ parameters and routed weights
def param_vector(n, seed):
    """n pairwise distinct values, magnitudes 0.25 .. 2 on an even grid visited with a stride of about 0.38 n (neighbours in index are far
    apart in value), seeded signs."""
    s = int(0.382 * n)
    while math.gcd(s, n) != 1:
        s += 1
    k = (torch.arange(n) * s + 101 * seed) % n
    sign = torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(1000 + seed)) * 2.0 - 1.0
    return ((0.25 + 1.75 * k.double() / (n - 1)) * sign).float()


def _perm(D, perm, seed):
    if perm == "identity":
        return torch.arange(D)
    if perm == "reversal":
        return D - 1 - torch.arange(D)
    return torch.randperm(D, generator=torch.Generator().manual_seed(seed))


def routing_tables(D, perm, seed):
    """(pi1 [4 D], H [D, 4]): hidden unit h reads input channel pi1[h]; output n sums hidden units H[n, 0..3].
    H[n, j] = j D + rho_j(p(n)) with p the permutation and rho_j the map that adds j to both 2-bit fields of the low nibble: inside a
    chunk a hidden unit is 16 a + 4 g + r (g the lane group, r the k-slot / accumulator register, in both kernels), so the four units of
    an output sit in four different quarters of the hidden dimension (different chunks under either chunking), lane groups and k-slots.
    pi1[h] = (p'(h mod D) + 37 (h div D)) mod D: a bijection per quarter, so every input channel is read by four hidden units."""
    p = _perm(D, perm, seed)
    H = torch.empty(D, 4, dtype=torch.long)
    for j in range(4):
        g, r = (p >> 2) & 3, p & 3
        H[:, j] = j * D + ((p & ~15) | (((g + j) & 3) << 2) | ((r + j) & 3))
    p1 = _perm(D, perm, seed + 1)
    h = torch.arange(4 * D)
    return (p1[h % D] + 37 * (h // D)) % D, H


def routed_weights(D, perm, seed, dt):
    """(w1 [4 D, D], w2 [D, 4 D], info): w1[h, pi1[h]] = a_h, w2[n, H[n, j]] = c_H[n, j], all else zero; a, c = +-COEF, seeded."""
    pi1, H = routing_tables(D, perm, seed)
    g = torch.Generator().manual_seed(seed + 7)
    coef = torch.tensor(COEF)
    draw = lambda: coef[torch.randint(0, len(COEF), (4 * D,), generator=g)] * (torch.randint(0, 2, (4 * D,), generator=g) * 2.0 - 1.0)
    a, c = draw(), draw()
    w1 = torch.zeros(4 * D, D)
    w1[torch.arange(4 * D), pi1] = a
    w2 = torch.zeros(D, 4 * D)
    w2[torch.arange(D).repeat_interleave(4), H.reshape(-1)] = c[H.reshape(-1)]
    assert torch.equal(round_to(w1, dt), w1) and torch.equal(round_to(w2, dt), w2)
    return w1, w2, {"pi1": pi1, "H": H, "a": a, "c": c}


def std_params(D, perm, seed, dt):
    """[ln_g, ln_b, w1, b1, w2, b2, next_g, next_b] with routed weights and param_vector vectors, and the routing info."""
    w1, w2, info = routed_weights(D, perm, seed, dt)
    v = [param_vector(n, seed + i) for i, n in enumerate((D, D, 4 * D, D, D, D))]
    return [v[0], v[1], w1, v[2], w2, v[3], v[4], v[5]], info


# ------------------------------------------------------------------------------------------------ input families
def edge_rows(M, D, seed):
    """[M, D] fp32 rows, row t of kind ROW_KINDS[t % 8] (every kind in every 16-token block): randn; a constant integer -3 .. 3 (variance 0:
    LN gives ln_b exactly); mean / std = 10, 100, 1000, 3000 with alternating sign (3000 is where the fp32 two-pass statistics' worst case,
    (D / 4 + 3) u 3000 = 0.018 standard deviations at D = 384, is still small; a one-pass variance has lost every digit at 1000);
    std 1e-3 around 0 (variance 1e-6 < eps); randn with one entry of 1000."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    for t in range(M):
        kind = ROW_KINDS[t % len(ROW_KINDS)]
        if kind == "const":
            x[t] = float((t // len(ROW_KINDS)) % 7 - 3)
        elif kind.startswith("mean"):
            x[t] += float(kind[4:]) * (1 if (t // len(ROW_KINDS)) % 2 == 0 else -1)
        elif kind == "tiny":
            x[t] *= 1e-3
        elif kind == "outlier":
            x[t, (7 * t) % D] = 1000.0
    return x


def rows_case(M, D, perm, seed, dt):
    """The edge rows through routed weights and the standard vectors."""
    params, info = std_params(D, perm, seed, dt)
    return edge_rows(M, D, seed + 50), params, info


def gelu_targets(D):
    """Pre-activation targets [D, 4], one row per output channel: its four hidden units get T_n (1 + j / 16), all in one band, so that an
    output's bound is as small as its own band's.  T_n: 0 (an exact +0), +-1e-4, +-3e-4, +-1e-3, then an even sweep of [-12, 12]."""
    special = [0.0, 1e-4, -1e-4, 3e-4, -3e-4, 1e-3, -1e-3]
    T = torch.tensor(special + np.linspace(-12.0, 12.0, D - len(special)).tolist(), dtype=torch.float64)
    return T[:, None] * (1 + torch.arange(4, dtype=torch.float64) / 16)


def gelu_case(M, D, perm, seed, dt):
    """Constant integer rows, so that LN(x) = ln_b exactly, with ln_b rounded to T: the pre-activation of hidden unit h = H[n, j] is
    a_h ln_b[pi1[h]] + b1[h] with no rounding before the addition, and b1[h] = fp32(target - a_h ln_b[pi1[h]]) puts it on gelu_targets
    to within one fp32 rounding: +0, 1e-4, the band -6 .. -3 of tiny negative results (fp16 subnormals), 6 .. 13 where the result is the
    argument.  |a_h ln_b| reaches 6 beside targets of 1e-4: a pre-activation rounded to T before the bias is added is off by 2^-7 there."""
    params, info = std_params(D, perm, seed, dt)
    params[1] = round_to(params[1], dt)
    tgt = torch.empty(4 * D, dtype=torch.float64)
    tgt[info["H"].reshape(-1)] = gelu_targets(D).reshape(-1)
    params[3] = (tgt - info["a"].double() * params[1].double()[info["pi1"]]).float()
    x = ((torch.arange(M) % 7).float() - 3.0)[:, None].expand(M, D).contiguous()
    return x, params, info


def epilogue_case(M, D, perm, seed, dt):
    """w2 = 0 and x = fp32(edge row - b2): x_new = x + b2 is the edge row again (to one rounding), so the epilogue's LayerNorm and cast see
    the constant, shifted, tiny and outlier rows that the prologue sees in rows_case."""
    params, info = std_params(D, perm, seed, dt)
    params[4] = torch.zeros_like(params[4])
    return (edge_rows(M, D, seed + 50).double() - params[5].double()).float(), params, info


FAMILIES = {"rows": rows_case, "gelu": gelu_case, "epilogue": epilogue_case}
PERMS = ("identity", "reversal", "random")


def make_case(family, M, D, perm, dt):
    """(x, params, info) of one family with the seed both test files use."""
    return FAMILIES[family](M, D, perm, 3 * D + PERMS.index(perm), dt)


# ------------------------------------------------------------------------------------------------ token tiling
TAIL_M = (1, 15, 16, 17, 33, 127, 128, 129, 257)


def tokens_per_wave(dt, D):
    """16 in every build but the 4-wave f16x2 build of D = 384, whose waves own two 16-token blocks."""
    return 32 if (dt == "f16x2" and D == 384) else 16


def last_token_place(M, dt, D):
    """(tile, wave, 16-token block of the wave, row in the block) of token M - 1."""
    t = M - 1
    tpw = tokens_per_wave(dt, D)
    return t // 128, (t % 128) // tpw, (t % tpw) // 16, t % 16


def later_tiles_M(n_cu):
    """128 (2 n_cu + 3) + 41 tokens: 2 n_cu + 4 tiles on a grid of at most n_cu workgroups, so every workgroup walks two or three tiles
    (the launchers even the tile counts out: grid = cdiv(tiles, cdiv(tiles, n_cu)))."""
    return 128 * (2 * n_cu + 3) + 41
