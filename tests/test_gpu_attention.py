"""GPU: the three kernels of csrc/attention.hip -- the register-resident attention_kernel (seven key-tile counts x masked / unmasked x four
element types, and its PARTIAL mode for key chunks), the streaming attention16_kernel of the 16-bit types above 256 keys, and
attention_combine_kernel, which merges the chunks of sequences beyond 512 keys in the 4-byte types -- through ocrvi_test_attention, on
score rows the flat randn rows of test_gpu_kernels.py::test_attention_kernel never show them: routed (one-hot), peaked, shifted by a
constant, and with the maximum placed at the corners of the kernels' key tiling.

Every input is rounded to something the element type holds exactly (aux_refs.round_to); the reference is aux_refs.attention_ref in float64
(on the CPU) and the error is held ELEMENT BY ELEMENT to aux_refs.attention_bound, computed from the reference's own softmax weights (the
same float64 torch code evaluated on the GPU: 32 N^2 terms per head is most of this file's run time otherwise; derivation
in its docstring; tests/test_attention_refs_cpu.py shows on the CPU that six kinds of wrong kernel land 10x or more outside it and that the
length table below reaches every build the source dispatches).  Every case runs twice into NaN-filled buffers and must be bit-identical;
no element is skipped.  The routing family is additionally held to its exact answer, out[i] = v[pi(i)]: bit-equal in bf16 and fp16 (p rounds
to 1 and so does the row sum), and in the 4-byte types within the roundings that are left when every other key contributes an exact zero:
  fp32   fl(fl(v p) fl(1 / p)), p = 2^r (1 + e): the product, the division (2 u allowed) and the final product; p's own error cancels: 4 u |v|
  f16x2  p and v enter as (hi, lo) pairs: lo of p is rounded (2^-22 = 4 u), lo lo is dropped (4 u), three products are accumulated (3 u),
         the row sum is that of the unsplit p, then the division and the product as above (3 u): 14 u |v|, plus the output's own rounding.

Not covered: the builds behind the A/B switches OCRVI_ATTN_STREAM, OCRVI_ATTN_F32_W8 and OCRVI_ATTN_X2_W8 (the register-resident 16-bit
kernel at 257 - 512 keys, the 4-wave fp32 / f16x2 builds).  They are read once per process and are not what production runs.

Largest err / bound per family and type, measured on the MI355X over all lengths of the table (365 tests, 19 s; the aux-kernel file takes 28 s):
              f32     f16x2   bf16    f16
  routing     0.062   0.091   0 (bit-equal)
  tau         0.233   0.963   0.994   0.991
  shift       0.088   0.019   0.766   0.600
  peak        0.247   0.067   0.953   0.914
(the figures near 1 are elements whose whole error is the output's one rounding: half an ulp is what the bound allows there.  The first run
of this file, with the P rounding taken as 2^-9 / 2^-12, failed 15 temperature cases by up to 1.39 x in bf16 and 1.03 x in fp16; an fp32
emulation of the kernel's order of operations on the CPU gave the same ratios to four digits, i.e. the kernels were right and the constant
was the top-of-binade figure: see rP in aux_refs.attention_bound.)"""
import os
import time

import pytest
import torch

import aux_refs as R
from test_gpu_kernels import DT

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

DTS = ["f32", "f16x2", "bf16", "f16"]
CASES = [(N, dt) for dt in DTS for N in R.attn_lengths(dt)]
WORST = {}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def run_attention(qkv, B, N, heads, dt):
    L = _L()
    qd = qkv.cuda().contiguous()
    out = torch.full((B, N, heads * 32), float("nan"), device="cuda")
    L.check(L.load().ocrvi_test_attention(0, DT[dt], qd.data_ptr(), B, N, heads, out.data_ptr(), 0, None))
    return out.cpu()


def _run_twice(qkv, B, N, heads, dt, tag):
    got = run_attention(qkv, B, N, heads, dt)
    assert torch.isfinite(got).all(), tag
    assert torch.equal(got, run_attention(qkv, B, N, heads, dt)), tag
    return got


def _check(qkv, B, N, heads, dt, family, tag):
    """One case against the float64 reference and its per-element bound.  Returns (got, reference output)."""
    ref = R.attention_ref(qkv, B, N, heads)
    bound = R.attention_bound(qkv, B, N, heads, dt, ref, device="cuda")
    got = _run_twice(qkv, B, N, heads, dt, tag)
    err = (got.double() - ref[0]).abs()
    ratio = float((err / bound).max())
    WORST[(family, dt)] = max(WORST.get((family, dt), 0.0), ratio)
    print(f"\n[attention {tag} B={B} heads={heads} {dt}] max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (tag, float(err.max()), ratio)
    return got, ref[0]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[attention summary] {time.time() - t0:.0f} s; largest err / bound per family and type")
    for fam in sorted({f for f, _ in WORST}):
        print(f"[attention summary] {fam:8s} " + "  ".join(f"{dt} {WORST[(fam, dt)]:.3f}" for dt in DTS if (fam, dt) in WORST))


def _li(N, dt):
    return R.attn_lengths(dt).index(N)


@pytest.mark.parametrize("N,dt", CASES)
def test_attention_routing_is_exact(N, dt):
    """Query i attends to key pi(i) alone, so out[i] = v[pi(i)]: the shared key order of the P and V operands, V's staging (transposed,
    half-swapped, (hi, lo) quartets), the masked tail and chunk merging with weights 0 and 1.  Identity, reversal and a random
    permutation make every key tile, lane group, the last valid key and the first key of every chunk somebody's target."""
    for i, perm in enumerate(("identity", "reversal", "random")):
        B, heads = R.attn_grid(N, _li(N, dt) + i + 2)
        qkv, pi = R.attn_routing(B, N, heads, dt, perm, 17 * N + i)
        got, ref = _check(qkv, B, N, heads, dt, "route", f"route={perm} N={N}")
        v = qkv.reshape(B, N, 3, heads, 32)[:, :, 2].transpose(1, 2)                          # [B, heads, N, 32]
        want = torch.gather(v, 2, pi.unsqueeze(-1).expand(-1, -1, -1, 32)).transpose(1, 2).reshape(B, N, heads * 32)
        assert torch.equal(ref.float(), want)                                                # the reference routes exactly
        if dt in ("bf16", "f16"):
            bad = (got != want).any(-1).nonzero()
            assert torch.equal(got, want), (perm, bad[:8].tolist(), float((got - want).abs().max()))
        else:
            lim = (4 if dt == "f32" else 14) * R.U32 * want.double().abs()
            lim = lim + R.half_ulp(want.double().abs() + lim, dt)
            err = (got.double() - want.double()).abs()
            assert bool((err <= lim).all()), (perm, float((err / lim).max()))


@pytest.mark.parametrize("N,dt", CASES)
def test_attention_temperature_sweep(N, dt):
    """randn rows with q times 1, 4, 16 and 64: from the flat rows of test_attention_kernel to nearly one-hot rows with real runner-ups
    and scaled scores of a few hundred."""
    for tag, B, heads, make in R.attn_families(N, dt, _li(N, dt)):
        if tag.startswith("tau="):
            _check(make(), B, N, heads, dt, "tau", f"{tag} N={N}")


@pytest.mark.parametrize("N,dt", CASES)
def test_attention_common_shift(N, dt):
    """All scores of a row moved by -45, -450, +45 or +450.  Negative: the zero-filled padding keys past N score 0, far above every real
    key, so one of them unmasked takes the whole row.  Positive: exp2 overflows unless the maximum is subtracted, and the shift has to be
    one fma, not the difference of two rounded products."""
    for tag, B, heads, make in R.attn_families(N, dt, _li(N, dt)):
        if tag.startswith("shift="):
            _check(make(), B, N, heads, dt, "shift", f"{tag} N={N}")


@pytest.mark.parametrize("N,dt", CASES)
def test_attention_position_of_the_maximum(N, dt):
    """Flat rows with one key raised to about half the weight, that key swept over the corners of lane groups, key tiles, 32-key steps,
    the masked tail and the chunk boundary: a maximum that is not reduced over every lane group or tile gives weights above 1."""
    for tag, B, heads, make in R.attn_families(N, dt):
        if tag.startswith("peak@"):
            _check(make(), B, N, heads, dt, "peak", f"{tag} N={N}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [200, 480, 1000])
def test_attention_batch_and_head_independence(N, dt):
    """One length per kernel (register-resident masked; register-resident / streaming; chunked / streaming masked): sequence b, head h of
    a 3 x 4 launch is bit-equal to the same sequence run alone with one head."""
    B, heads = 3, 4
    D = heads * 32
    qkv = R.attn_temperature(B, N, heads, dt, 4, N + 5)
    got = _run_twice(qkv, B, N, heads, dt, f"independence N={N}")
    for b in range(B):
        for h in range(heads):
            one = torch.cat([qkv[b:b + 1, :, c * D + h * 32:c * D + (h + 1) * 32] for c in range(3)], -1).contiguous()
            alone = run_attention(one, 1, N, 1, dt)
            assert torch.equal(alone[0], got[b, :, h * 32:(h + 1) * 32]), (b, h)


def test_attention_rejects_sequences_past_each_type_limit():
    L = _L()
    for dt in DTS:
        N = R.ATTN_MAX_KEYS[dt] + 1
        qkv = torch.zeros(1, N, 96, device="cuda")
        out = torch.zeros(1, N, 32, device="cuda")
        rc = L.load().ocrvi_test_attention(0, DT[dt], qkv.data_ptr(), 1, N, 1, out.data_ptr(), 0, None)
        assert rc == -1, (dt, N, rc)                                  # OCRVI_EINVAL
        with pytest.raises(ValueError):
            L.check(rc)
