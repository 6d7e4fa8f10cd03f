"""CPU: the float64 attention reference, the per-element bound and the input families of tests/aux_refs.py, which
tests/test_gpu_attention.py holds csrc/attention.hip to.  Four things are pinned here, none of which needs a GPU:

* attention_ref is the oracle's _mhsa and F.scaled_dot_product_attention in float64;
* the measured constants of the bound (attn_acc_terms, the exp2 and dot figures its docstring quotes) are re-measured, float64 against
  an fp32 evaluation of the same formula, and must keep their factor of two;
* the bound cannot hide a fault: six wrong kernels, built in float64, each land a factor of 10 or more outside it in at least one
  input family, for every element type and length;
* the length table reaches every build attention.hip can dispatch, with the thresholds read out of the source."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_refs as R
from oracle import svtrv2_cpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DTS = ["f32", "f16x2", "bf16", "f16"]
U = R.U32


def test_attention_ref_is_the_oracle_and_torch_sdpa_in_float64():
    g = torch.Generator().manual_seed(3)
    for B, N, heads, tau in [(2, 16, 1, 1.0), (1, 100, 3, 4.0), (3, 257, 2, 16.0), (1, 513, 1, 1.0)]:
        qkv = torch.randn(B, N, 3 * heads * 32, generator=g)
        qkv[..., :heads * 32] *= tau
        out, w = R.attention_ref(qkv, B, N, heads)
        q, k, v = qkv.double().reshape(B, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
        for want in (svtrv2_cpu._mhsa(q, k, v), F.scaled_dot_product_attention(q, k, v)):
            want = want.transpose(1, 2).reshape(B, N, heads * 32)
            assert float((out - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert out.dtype == torch.float64 and w.shape == (B, heads, N, N) and float((w.sum(-1) - 1).abs().max()) < 1e-12
        # the packed layout: head h of q / k / v is columns [h * 32, (h + 1) * 32) of the first / second / third block of heads * 32
        D = heads * 32
        h = heads - 1
        one = torch.cat([qkv[..., c * D + h * 32:c * D + (h + 1) * 32] for c in range(3)], -1)
        assert torch.equal(R.attention_ref(one, B, N, 1)[0], out[..., h * 32:])


def _seq32(x, axis):
    """fp32 sum along `axis` in one sequential chain (numpy's cumsum adds in order)."""
    return np.take(np.cumsum(x.astype(np.float32), axis=axis, dtype=np.float32), -1, axis=axis).astype(np.float64)


def test_measured_constants_of_the_bound_keep_their_margin():
    """attention_bound takes three figures from a measurement, not from the source: the accumulation error of P V and of the row sum
    (attn_acc_terms) and the accuracy of exp2.  Measured again here -- float64 against fp32 on the CPU, sequential chains -- each constant
    must be at least twice what is measured; the 32-term dot, whose constant (32 u) is the worst case over all orders, is printed beside."""
    rng = np.random.default_rng(0)
    for K in (16, 100, 512, 1024):
        worst = [0.0, 0.0, 0.0]
        for tau in (1, 4, 16):
            q, k, v = rng.standard_normal((64, 32)) * tau, rng.standard_normal((K, 32)), rng.standard_normal((K, 32))
            s = (q @ k.T) * R.ATTN_SCALE
            p = np.exp(s - s.max(1, keepdims=True)).astype(np.float32).astype(np.float64)
            v = v.astype(np.float32).astype(np.float64)
            terms = p[:, :, None] * v[None]
            worst[0] = max(worst[0], float((np.abs(_seq32(terms, 1) - terms.sum(1)) / np.abs(terms).sum(1)).max()))
            worst[1] = max(worst[1], float((np.abs(_seq32(p, 1) - p.sum(1)) / p.sum(1)).max()))
            q32, k32 = q.astype(np.float32).astype(np.float64), k.astype(np.float32).astype(np.float64)
            dots = q32[:, None, :] * k32[None]
            worst[2] = max(worst[2], float((np.abs(_seq32(dots, 2) - dots.sum(2)) / np.abs(dots).sum(2)).max()))
        apv, asum = R.attn_acc_terms(K, "f32")
        print(f"\n[attention constants K={K}] fp32 chain / float64, in 2^-24: P V {worst[0] / U:.1f} (bound {apv:.1f}), row sum {worst[1] / U:.1f} "
              f"(bound {asum:.1f}), 32-term dot {worst[2] / U:.1f} (bound 32)")
        assert apv * U >= 2 * worst[0] and asum * U >= 2 * worst[1] and 32 * U >= 2 * worst[2]
        assert R.attn_acc_terms(K, "f16x2")[0] >= apv and R.attn_acc_terms(K, "bf16") == (apv, asum)
    x = rng.uniform(-126.0, 0.01, 200000).astype(np.float32)
    e = float((np.abs(np.exp2(x).astype(np.float64) - np.exp2(x.astype(np.float64))) / np.exp2(x.astype(np.float64))).max())
    c2 = float(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))          # attention.hip's constant, as fp32 forms it
    ec = abs(c2 - 32 ** -0.5 * np.log2(np.e)) / (32 ** -0.5 * np.log2(np.e))
    print(f"\n[attention constants] fp32 exp2 {e / U:.2f} (bound 4), c2 off by {ec / U:.3f} (k = 2 leaves 1 for it)")
    assert 4 * U >= 2 * e and ec <= U


# ------------------------------------------------------------------------------------------------ the bound cannot hide a fault
P_MAX = {"f32": 2.0 ** 128, "bf16": 2.0 ** 128, "f16": 65520.0, "f16x2": 65520.0 / 4096}    # where a rounded p (f16x2: 4096 p) turns infinite


def _mutant(kind, qkv, B, N, heads, dt):
    """The output [B, N, heads * 32] of a kernel with one fault, in float64."""
    q, k, v = R._qkv_heads(qkv, B, N, heads)
    scale = 33 ** -0.5 if kind == "scale" else R.ATTN_SCALE
    if kind == "swap":                                               # (a) the values of two keys exchanged
        idx = torch.arange(N)
        idx[5], idx[N - 2] = N - 2, 5
        v = v[:, :, idx]
    if kind == "drop":                                               # (b) the last valid key masked
        k, v = k[:, :, :N - 1], v[:, :, :N - 1]
    if kind == "pad":                                                # (c) one zero-filled padding key not masked
        k, v = F.pad(k, (0, 0, 0, 1)), F.pad(v, (0, 0, 0, 1))
    s = (q @ k.transpose(-2, -1)) * scale
    if kind == "max":                                                # (e) the row maximum misses lane group 1 of key tile 0 (keys 4 .. 7)
        keep = torch.ones(N, dtype=torch.bool)
        keep[4:8] = False
        m = s[..., keep].max(-1, keepdim=True).values
        p = torch.exp(s - m)                                         # the shift cancels in exact arithmetic: what is left is the range
        p = torch.where(p >= P_MAX[dt], torch.full_like(p, float("inf")), p)
        out = (p @ v) / p.sum(-1, keepdim=True)                      # inf / inf: the row is NaN
    elif kind == "merge":                                            # (f) chunk 1 merged with weight 1 instead of exp(m_1 - m)
        chunks = R.attention_chunks(N)
        ms = [s[..., a:a + n].max(-1, keepdim=True).values for a, n in chunks]
        m = torch.stack(ms).max(0).values
        num, den = 0.0, 0.0
        for c, (a, n) in enumerate(chunks):
            p = torch.exp(s[..., a:a + n] - ms[c])
            wc = torch.ones_like(m) if c == 1 else torch.exp(ms[c] - m)
            num, den = num + wc * (p @ v[:, :, a:a + n]), den + wc * p.sum(-1, keepdim=True)
        out = num / den
    else:
        out = torch.softmax(s, -1) @ v
    return out.transpose(1, 2).reshape(B, N, heads * 32)


MUTANTS = ["swap", "drop", "pad", "scale", "max", "merge"]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [100, 480, 1000])
def test_bound_rejects_every_mutant_by_a_factor_of_ten(N, dt):
    """For every wrong kernel, the largest |mutant - reference| / bound over the elements of each input family; a non-finite mutant
    output counts as infinitely far out.  At least one family must reach 10.  (f) needs key chunks: the 4-byte types above 512 keys."""
    table = {m: {} for m in MUTANTS}
    for tag, B, heads, make in R.attn_families(N, dt, grid=(2, 2)):
        qkv = make()
        ref = R.attention_ref(qkv, B, N, heads)
        bound = R.attention_bound(qkv, B, N, heads, dt, ref)
        assert float(bound.min()) > 0
        for m in MUTANTS:
            if m == "merge" and (dt in ("bf16", "f16") or N <= R.ATTN_CHUNK):
                continue
            out = _mutant(m, qkv, B, N, heads, dt)
            ratio = (out - ref[0]).abs() / bound
            table[m][tag] = float("inf") if not bool(torch.isfinite(out).all()) else float(ratio.max())
    print(f"\n[attention mutants N={N} {dt}] largest |mutant - ref| / bound per family")
    for m in MUTANTS:
        if table[m]:
            best = max(table[m], key=table[m].get)
            print(f"  {m:6s} best {table[m][best]:10.3g} ({best})   " + "  ".join(f"{t} {r:.3g}" for t, r in table[m].items()))
            assert table[m][best] >= 10.0, (m, table[m])
    assert ("merge" in [m for m in MUTANTS if table[m]]) == (dt in ("f32", "f16x2") and N > R.ATTN_CHUNK)


def test_input_families_are_what_they_claim():
    """Routing: every non-target weight is below 2^-60 and v has no zero component; the temperature sweep goes from flat to nearly
    one-hot; a common shift leaves the weights alone; the raised key holds about half of every row."""
    for N, dt in [(16, "bf16"), (1000, "f16"), (1024, "f32"), (1537, "f16x2")]:
        for perm in ("identity", "reversal", "random"):
            qkv, pi = R.attn_routing(2, N, 1, dt, perm, N)
            assert torch.equal(R.round_to(qkv, dt), qkv)
            out, w = R.attention_ref(qkv, 2, N, 1)
            target = torch.zeros_like(w, dtype=torch.bool).scatter_(-1, pi.unsqueeze(-1), True)
            assert float(w[~target].max()) < 2.0 ** -60 and float(w[target].min()) > 1 - 2.0 ** -50
            v = qkv.reshape(2, N, 3, 1, 32)[:, :, 2, 0]
            assert float(v.abs().min()) >= 2.0 ** -7
            assert torch.equal(out.float(), torch.gather(v, 1, pi[:, 0].unsqueeze(-1).expand(-1, -1, 32)))
            if dt in ("f32", "f16x2"):
                assert float((v.half().float() != v).float().mean()) > 0.9       # the lo half of V has to arrive
        assert sorted(pi[0, 0].tolist()) == list(range(N))
    top = [float(R.attention_ref(R.attn_temperature(1, 480, 2, "f32", tau, 1), 1, 480, 2)[1].max(-1).values.median()) for tau in (1, 4, 16, 64)]
    assert top[0] < 0.1 and top[1] > 0.2 and top[2] > 0.8 and top[3] > 0.99, top
    base = R.attn_shift(1, 200, 1, "f16", 45, 2)
    for sh, q0 in ((-45, -16.0), (450, 160.0), (-450, -160.0)):
        other = R.attn_shift(1, 200, 1, "f16", sh, 2)
        assert float(other[0, 0, 0]) == q0 and float(other[0, 0, 32]) == 16.0
        assert float((R.attention_ref(other, 1, 200, 1)[1] - R.attention_ref(base, 1, 200, 1)[1]).abs().max()) < 1e-10
    assert abs(16 * 16 * R.ATTN_SCALE - 45.25) < 0.01
    for N, dt in [(100, "bf16"), (1000, "f32")]:
        pos = R.attn_peak_positions(N, dt)
        assert {0, 3, 4, 15, 16, 31, 32, N - 1, 16 * ((N - 1) // 16)} <= set(pos)
        assert (N <= 512) or {511, 512} <= set(pos)
        w = R.attention_ref(R.attn_peak(N, 1, dt, pos, 1), len(pos), N, 1)[1]
        for b, p in enumerate(pos):
            share = w[b, 0, :, p]
            assert 0.3 < float(share.median()) < 0.7 and float(share.min()) > 0.005, (N, p, float(share.median()), float(share.min()))


# ------------------------------------------------------------------------------------------------ dispatch coverage
def _thresholds_in_source():
    src = open(os.path.join(REPO, "ocr_vi_invoice_amd", "csrc", "attention.hip"), encoding="utf-8").read()
    ladder = re.findall(r"if \(NT <= (\d+)\) return launch_attn<T, (\d+)>", src)
    last = re.findall(r"\n    return launch_attn<T, (\d+)>", src)
    stream = set(re.findall(r"streaming && N > (\d+)\) \|\| N > (\d+)", src))
    chunk = re.findall(r"attn_chunks\(int N\) \{ return \(N \+ (\d+)\) / (\d+); \}", src)
    single = re.findall(r"if \(N <= (\d+)\) return attn_range<T>", src)
    limit = re.findall(r"N <= \(dtype_size\(dtype\) == 2 \? (\d+) : (\d+)\)", src)
    align = re.findall(r"align_up\(\(size_t\)cdiv\(N, attn_chunks\(N\)\), (\d+)\)", src)
    return ladder, last, stream, chunk, single, limit, align


def test_length_table_reaches_every_build_the_source_dispatches():
    ladder, last, stream, chunk, single, limit, align = _thresholds_in_source()
    assert ladder and all(a == b for a, b in ladder) and len(last) == 1
    assert tuple(int(a) for a, _ in ladder) + (int(last[0]),) == R.ATTN_MAXT
    assert stream == {(str(R.ATTN_STREAM_ABOVE), str(R.ATTN_CHUNK))}
    assert chunk == [(str(R.ATTN_CHUNK - 1), str(R.ATTN_CHUNK))] and single == [str(R.ATTN_CHUNK)] and align == ["32"]
    assert limit == [(str(R.ATTN_MAX_KEYS["bf16"]), str(R.ATTN_MAX_KEYS["f32"]))]
    assert R.attention_chunks(1000) == [(0, 512), (512, 488)] and R.attention_chunks(513) == [(0, 288), (288, 225)]
    for dt in DTS:
        lengths = R.attn_lengths(dt)
        assert max(lengths) == R.ATTN_MAX_KEYS[dt]
        reached = {b for N in lengths for b in R.attention_plan(N, dt)}
        four = dt in ("f32", "f16x2")
        maxts = R.ATTN_MAXT if four else tuple(m for m in R.ATTN_MAXT if 16 * m <= R.ATTN_STREAM_ABOVE)
        want = {("reg", m, mask) for m in maxts for mask in (False, True)}
        if not four:
            want |= {("stream", None, False), ("stream", None, True)}
        assert reached == want, reached ^ want
        counts = {len(R.attention_plan(N, dt)) for N in lengths}
        assert counts == ({1, 2, 3, 4, 8} if four else {1})
        # unmasked and masked builds inside key chunks too (partial mode), not only in single launches
        if four:
            partial = {b for N in lengths if N > R.ATTN_CHUNK for b in R.attention_plan(N, dt)}
            assert {m for _, m, _ in partial} >= {15, 30, 32} and {mask for _, _, mask in partial} == {False, True}
    # the B x heads grids: 1, 3, 7, 12 and one large count, none but the last a multiple of 8 (xcd_remap's remainder path)
    assert sorted(b * h for b, h in R.ATTN_GRIDS) == [1, 3, 7, 12, 512]
    for N in R.ATTN_LENGTHS + R.ATTN_LENGTHS_4BYTE:
        grids = {R.attn_grid(N, i) for i in range(8)}
        assert all(b * h * N * N <= 1 << 23 or (b, h) == (1, 1) for b, h in grids)
        assert N <= 1024 or max(b * h for b, h in grids) <= 2
