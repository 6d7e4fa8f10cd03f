"""GPU: mlp_fused_kernel (csrc/mlp_fused.hip; bf16, fp16) and the three builds of mlp_x2_kernel (csrc/mlp_x2.hip; f16x2 at D = 128, 256 and
the 4-wave split-ring build of D = 384) through the test hooks, on routed weights and edge-case rows, every element held to
mlp_refs.mlp_bound around the float64 reference (derivation in tests/mlp_refs.py; tests/test_mlp_refs_cpu.py shows on the CPU that an
fp32 emulation of the kernels stays inside the bound on exactly these cases and that sixteen wrong kernels land 50x or more outside
it, but for one that stays inside it in f16x2, which the CPU file asserts).  Every case runs twice into NaN-filled xn and must be bit-identical; no element is skipped.
Modes "ln" and "cast" go through ocrvi_test_mlp_raw with 128 guard rows behind x and behind the raw xn buffer, which must come back
bit for bit; mode "none" (no xn) goes through ocrvi_test_mlp with the x guard alone.

  routing       rows_case at M = 129, three permutations, one mode each: which b1 / b2 / norm entry and which fc2 k-slot each output sees
  gelu          gelu_case at M = 160: pre-activations on an even sweep of [-12, 12] times 1 .. 1.19 (to +-14.25), with +0, +-1e-4, the
                fp16-subnormal band and the identity band
  rows          rows_case at M = 160: constant, shifted (mean / std to 3000), tiny-variance and one-outlier rows into the prologue norm
  epilogue      epilogue_case at M = 160: the same rows into the epilogue's norm and cast (w2 = 0)
  tail          every M of mlp_refs.TAIL_M in all three modes, with guard rows
  independence  one row changed: every other row keeps its bits
  later tiles   M = 128 (2 #CU + 3) + 41 rows of period 97: every workgroup walks two or three tiles; the first 97 rows are held to the
                bound, every later occurrence of a row is bit-equal to its first

Largest err / bound per family and type at D = 128 / 256 / 384, measured on the MI355X (54 tests, 6.8 s for the file; the slowest test 0.55 s):
                bf16                    f16                     f16x2
  routing       0.997  0.999  0.999     0.992  0.994  0.994     0.441  0.493  0.440
  gelu          0.992  0.996  0.998     0.992  0.996  0.997     0.449  0.521  0.497
  rows          0.998  0.997  0.999     0.996  0.991  0.993     0.369  0.355  0.325
  epilogue      1.000  1.000  1.000     1.000  1.000  1.000     0.633  0.674  0.713
  tail          0.999  0.999  0.999     0.996  0.996  0.994     0.345  0.465  0.448
  later tiles   0.945  0.974  0.948     0.963  0.989  0.962     0.368  0.355  0.249
(the 16-bit figures near 1 are elements whose whole error is the last rounding to T next to a tie -- 2999.99979 rounded to 2992 in bf16,
ratio 0.99993 --: half an ulp is what the bound allows; the fp32 emulation on the CPU gives the same figures to two or three digits.
Nothing was found wrong in either kernel.  profiles/r14_mlp_kernels.md has the CPU tables.)
"""
import os
import time

import numpy as np
import pytest
import torch

import mlp_refs as R
from test_gpu_kernels import DT

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, os.cpu_count() or 1))

DTS = ["bf16", "f16", "f16x2"]
DS = [128, 256, 384]
CASES = [(dt, D) for dt in DTS for D in DS]
GUARD = 128                      # rows behind x and behind xn
X_GUARD = 0x7FA5C3D2             # a NaN with a payload, as int32
WORST = {}


def _L():
    from ocr_vi_invoice_amd import _lib as L
    return L


def run_mlp(x, params, mode, dt):
    """One application on x [M, D] (CPU or GPU tensor): (x_new, xn or None) as GPU tensors.  The guards are checked here."""
    L = _L()
    lib = L.load()
    M, D = x.shape
    esz = 4 if dt == "f16x2" else 2
    xd = torch.empty((M + GUARD, D), device="cuda", dtype=torch.float32)
    xd[:M] = x
    xd[M:].view(torch.int32).fill_(X_GUARD)
    arrs = [np.ascontiguousarray(p.numpy(), dtype=np.float32) for p in params]
    ptr = [a.ctypes.data for a in arrs]
    ng, nb = (ptr[6], ptr[7]) if mode == "ln" else (None, None)
    xn = None
    if mode == "none":
        L.check(lib.ocrvi_test_mlp(0, DT[dt], xd.data_ptr(), *ptr[:6], None, None, 0, M, D, None, 0, None))
    else:
        raw = torch.full(((M + GUARD) * D * esz,), 0xFF, dtype=torch.uint8, device="cuda")       # every element a NaN
        xn = torch.full((M, D), float("nan"), device="cuda")
        L.check(lib.ocrvi_test_mlp_raw(0, DT[dt], xd.data_ptr(), *ptr[:6], ng, nb, M, D, raw.data_ptr(), xn.data_ptr(), 0, None))
        assert bool((raw[M * D * esz:] == 0xFF).all()), "the guard rows behind xn changed"
        assert bool(torch.isfinite(xn).all()), "an element of xn was not written"
    torch.cuda.synchronize()
    assert bool((xd[M:].view(torch.int32) == X_GUARD).all()), "the guard rows behind x changed"
    assert bool(torch.isfinite(xd[:M]).all())
    return xd[:M], xn


def _run_twice(x, params, mode, dt, tag):
    y, xn = run_mlp(x, params, mode, dt)
    y2, xn2 = run_mlp(x, params, mode, dt)
    assert torch.equal(y, y2) and (xn is None or torch.equal(xn, xn2)), tag
    return y, xn


def _hold(got, ref, bound, family, dt, D, tag):
    worst = 0.0
    for name, g, r, b in zip(("x_new", "xn"), got, ref, bound):
        if r is None:
            continue
        err = (g.cpu().double() - r).abs()
        ratio = float((err / b).max())
        worst = max(worst, ratio)
        bad = (~(err <= b)).nonzero()
        print(f"\n[mlp {tag} D={D} {dt}] {name}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
        assert bad.numel() == 0, (tag, name, ratio, bad[:8].tolist())
    WORST[(family, dt, D)] = max(WORST.get((family, dt, D), 0.0), worst)


def _check(family_fn, M, D, perm, dt, mode, family, tag=None):
    x, params, _ = R.make_case(family_fn, M, D, perm, dt)
    tr = R.mlp_trace(x, *params, mode)
    bound = R.mlp_bound(x, *params, mode, dt, tr)
    got = _run_twice(x, params, mode, dt, tag or family)
    _hold(got, (tr["y"], tr["xn"]), bound, family, dt, D, f"{tag or family} {perm} M={M} {mode}")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print(f"\n[mlp summary] {time.time() - t0:.0f} s; largest err / bound per family, type and D = {DS}")
    for fam in ("routing", "gelu", "rows", "epilogue", "tail", "later"):
        print(f"[mlp summary] {fam:9s} " + "   ".join(dt + " " + " ".join(f"{WORST.get((fam, dt, D), float('nan')):.3f}" for D in DS) for dt in DTS))


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_routing(dt, D):
    """Identity, reversal and a random permutation behind sigma and pi1: each output depends on four hidden units in four different chunks,
    lane groups and k-slots, each hidden unit on one input channel, and all six vectors have pairwise distinct entries."""
    for i, perm in enumerate(R.PERMS):
        _check("rows", 129, D, perm, dt, R.MODES[i], "routing")


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_gelu_sweep(dt, D):
    for mode in R.MODES:
        _check("gelu", 160, D, "random", dt, mode, "gelu")


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_layernorm_edge_rows(dt, D):
    """The edge rows into the prologue norm (rows) and into the epilogue's norm and cast (epilogue): one full and one ragged tile."""
    for fam in ("rows", "epilogue"):
        for mode in R.MODES:
            _check(fam, 160, D, "random", dt, mode, fam)


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_token_tail(dt, D):
    """Every M of TAIL_M (test_mlp_refs_cpu.py lists the lanes they end on) in all three modes, on the first M rows of one 257-row case:
    the bound, and the guard rows behind x (every mode) and behind the raw xn buffer ("ln" and "cast": both store paths at every M)."""
    x, params, _ = R.make_case("rows", max(R.TAIL_M), D, "reversal", dt)
    refs = {}
    for mode in R.MODES:
        tr = R.mlp_trace(x, *params, mode)
        refs[mode] = ((tr["y"], tr["xn"]), R.mlp_bound(x, *params, mode, dt, tr))
    for M in R.TAIL_M:
        for mode in R.MODES:
            ref, bound = refs[mode]
            got = _run_twice(x[:M].contiguous(), params, mode, dt, f"tail M={M}")
            cut = lambda pair: tuple(None if t is None else t[:M] for t in pair)
            _hold(got, cut(ref), cut(bound), "tail", dt, D, f"tail M={M} {mode}")


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_token_independence(dt, D):
    x, params, _ = R.make_case("rows", 160, D, "identity", dt)
    y, xn = _run_twice(x, params, "ln", dt, "independence")
    x2 = x.clone()
    x2[77] = x2[77] * 1.5 + 0.25
    y2, xn2 = run_mlp(x2, params, "ln", dt)
    keep = torch.arange(160, device="cuda") != 77
    assert torch.equal(y[keep], y2[keep]) and torch.equal(xn[keep], xn2[keep])
    assert not torch.equal(y[77], y2[77])


@pytest.mark.parametrize("dt,D", CASES)
def test_mlp_later_tiles_equal_the_first(dt, D):
    """2 #CU + 4 tiles: every workgroup of every build walks two or three of them, the weight ring wraps at a different slot phase in each,
    and row t holds block[t mod 97]: the first 97 rows are held to the float64 bound, every other row is bit-equal to its first occurrence."""
    P = 97
    M = R.later_tiles_M(torch.cuda.get_device_properties(0).multi_processor_count)
    block, params, _ = R.make_case("rows", P, D, "random", dt)
    idx = torch.arange(M, device="cuda") % P
    y, xn = _run_twice(block.cuda()[idx], params, "ln", dt, "later tiles")
    tr = R.mlp_trace(block, *params, "ln")
    _hold((y[:P], xn[:P]), (tr["y"], tr["xn"]), R.mlp_bound(block, *params, "ln", dt, tr), "later", dt, D, f"later tiles M={M}")
    for name, t in (("x_new", y), ("xn", xn)):
        bad = (t != t[:P][idx]).any(-1).nonzero().flatten()
        assert bad.numel() == 0, (name, int(bad.numel()), bad[:8].tolist())
