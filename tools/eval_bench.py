#!/usr/bin/env python3
"""Times the three validation kernels (include/ocrvi.h, "Validation") and, beside each, the same arithmetic written with torch ops on
the device (tests/eval_refs.py).  Prints one JSON line.

  det_eval       16 x 960 x 1280, eight float32 maps; algorithmic bytes = 8 maps x 4 B per pixel, over time, as a share of 8 TB/s
  ctc_loss       T = 64, B = 256, C = 232, target lengths 1..24
  edit_distance  B = 256 pairs, 64 prediction ids against up to 48 ground-truth ids

Each side: `--warmup` calls, then `--reps` timed calls, the two sides alternating call by call; a host clock around a call that ends in a
device synchronise (the torch forms read counts back to the host, so events around the launches would not cover them); the median.
The torch column is context, not a gate.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_refs as ER  # noqa: E402
from ocr_vi_invoice_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8e12


def alternate(ours, theirs, warmup, reps):
    """Median seconds of each side, the two alternating."""
    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for _ in range(warmup):
        once(ours), once(theirs)
    a, b = [], []
    for _ in range(reps):
        a.append(once(ours))
        b.append(once(theirs))
    return statistics.median(a), statistics.median(b), min(a), max(a)


def bench_det_eval(lib, args):
    N, H, W = args.pages, args.height, args.width
    n = N * H * W
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = (torch.rand(N, 1, H, W, device="cuda", generator=g) < 0.1).float()
    mask = (torch.rand(N, 1, H, W, device="cuda", generator=g) < 0.97).float()
    logits = torch.randn(N, 1, H, W, device="cuda", generator=g) * 1.5 + (gt * 4 - 2)
    binary = torch.sigmoid(logits)
    thresh = torch.sigmoid(torch.randn(N, 1, H, W, device="cuda", generator=g))
    thresh_binary = torch.reciprocal(1 + torch.exp(-50 * (binary - thresh)))
    thresh_map = 0.3 + 0.4 * torch.rand(N, 1, H, W, device="cuda", generator=g)
    thresh_mask = (torch.rand(N, 1, H, W, device="cuda", generator=g) < 0.35).float()
    maps = (binary, thresh, thresh_binary, logits, gt, mask, thresh_map, thresh_mask)
    need = C.c_size_t()
    _lib.check(lib.ocrvi_det_eval_workspace_bytes(N, H, W, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    rec = torch.empty(13, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(lib.ocrvi_det_eval(0, *[m.data_ptr() for m in maps], N, H, W, 3.0, rec.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return rec.cpu()

    def theirs():
        return ER.det_eval_torch(*maps)

    raw = ours().numpy()
    want = theirs()
    got_topk = float(raw[7:8].view(np.float64)[0])
    assert int(raw[5]) == want["negative_count"] and abs(got_topk - want["topk_bce"]) <= 2e-6 * want["topk_bce"], (raw, want)
    t, t_torch, lo, hi = alternate(ours, theirs, args.warmup, args.reps)
    return {"shape": [N, H, W], "k": int(raw[5]), "ms": t * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "algorithmic_bytes": 32 * n,
            "share_of_8TBps": 32 * n / t / HBM_BYTES_PER_S, "torch_ms": t_torch * 1e3}


def bench_ctc(lib, args):
    T, B, Cn, Lmax = 64, 256, 232, 24
    rng = np.random.default_rng(2)
    lp = torch.log_softmax(torch.from_numpy(rng.normal(0, 3, (T, B, Cn)).astype(np.float32)).cuda(), -1)
    lens = torch.from_numpy(rng.integers(1, Lmax + 1, B).astype(np.int32)).cuda()
    targets = torch.from_numpy(rng.integers(2, Cn, (B, Lmax)).astype(np.int32)).cuda()
    nll = torch.empty(B, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(lib.ocrvi_ctc_loss(0, lp.data_ptr(), T, B, Cn, targets.data_ptr(), Lmax, lens.data_ptr(), None, 0, nll.data_ptr(), stream))
        return nll.cpu()

    def theirs():
        return ER.ctc_nll_torch(lp, targets, lens).cpu()

    a, b = ours(), theirs()
    assert torch.allclose(a, b, rtol=1e-9, atol=0), (a - b).abs().max()
    t, t_torch, lo, hi = alternate(ours, theirs, args.warmup, args.reps)
    return {"shape": [T, B, Cn], "ms": t * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "torch_ms": t_torch * 1e3}


def bench_edit(lib, args):
    B, T, G = 256, 64, 48
    rng = np.random.default_rng(3)
    pred = torch.from_numpy(rng.integers(0, 40, (B, T)).astype(np.int32)).cuda()
    plen = torch.from_numpy(rng.integers(0, T + 1, B).astype(np.int32)).cuda()
    gt = torch.from_numpy(rng.integers(2, 40, (B, G)).astype(np.int32)).cuda()
    glen = torch.from_numpy(rng.integers(0, G + 1, B).astype(np.int32)).cuda()
    dist = torch.empty(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(lib.ocrvi_edit_distance(0, pred.data_ptr(), T, plen.data_ptr(), gt.data_ptr(), G, glen.data_ptr(), B, dist.data_ptr(), stream))
        return dist.cpu()

    def theirs():
        return ER.edit_distance_torch(pred, plen, gt, glen).cpu()

    a, b = ours(), theirs()
    assert torch.equal(a, b), (a, b)
    t, t_torch, lo, hi = alternate(ours, theirs, args.warmup, args.reps)
    return {"shape": [B, T, G], "ms": t * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "torch_ms": t_torch * 1e3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU")
    lib = _lib.load()
    out = {"det_eval": bench_det_eval(lib, args), "ctc_loss": bench_ctc(lib, args), "edit_distance": bench_edit(lib, args),
           "timing": f"host clock around call + synchronise, median of {args.reps} after {args.warmup} warm-up calls, sides alternating"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
