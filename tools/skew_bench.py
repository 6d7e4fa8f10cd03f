#!/usr/bin/env python3
"""Times the skew estimate (include/ocrvi.h, "Skew estimate") on 64 pages of 960 x 1280 (rows x columns): synthetic invoices turned by a
few degrees, ``--distinct`` different pages repeated (each copy its own device tensor).  Prints one JSON line.

Kernels: the library's per-launch profiler brackets each of the three launches of ``ocrvi_skew_scores_pages`` (all pages in one page table)
with device events; ``--warmup`` calls first, then the median, minimum and maximum of ``--reps``.  ``estimate_skews`` on device tensors:
wall clock around the call (table upload, launches, the copy of the scores, the host pick).  PCIe: the score bytes that come back
against 3 H W.  Engine: ``Engine.run(pages, quads="deskew")`` against ``Engine.run(pages)`` on the same host pages, wall clock, the
median of ``--engine-steps`` after ``--engine-warmup`` (DBNet++ ResNet-50 and SVTRv2-tiny with seeded random weights in f16x2 at
``--det-size``, bars blended into the map so that there are boxes to recognise); the deskewed pages are larger than the originals, so
the detector sees other buckets.  Needs a GPU: there is no fallback."""
import argparse
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

import skew_ref as SR  # noqa: E402
from ocr_vi_invoice_amd import _lib, pipeline, synth  # noqa: E402

WORK_H, H, W = 500, 960, 1280
ANGLES = (2.3, -1.1, 4.0, -6.5, 0.6, -3.2, 9.0, -12.0)
TAGS = ("doc_grey", "skew_edges", "skew_scores")


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def bench_kernels(lib, pages, args):
    for _ in range(args.warmup):
        pipeline.skew_scores(pages, WORK_H)
    torch.cuda.synchronize()
    t = {k: [] for k in TAGS}
    lib.ocrvi_prof_enable(1)
    for _ in range(args.reps):
        lib.ocrvi_prof_reset()
        pipeline.skew_scores(pages, WORK_H)
        torch.cuda.synchronize()
        rep = _lib.prof_report()
        for k in TAGS:
            t[k].append(rep[k]["ms"])
    lib.ocrvi_prof_enable(0)
    lib.ocrvi_prof_reset()
    whole = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        skews = pipeline.estimate_skews(pages)
        if r >= args.warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in t.items()}, spread(whole), skews


def bench_engine(pages, args):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    pp = pipeline.DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)
    bars = {}

    def hook(prob, idx):
        h, w = prob.shape[2], prob.shape[3]
        if (h, w) not in bars:
            k = np.zeros((1, h, w), np.float32)
            for j in range((h - 30) // 40):
                k[0, 20 + 40 * j:32 + 40 * j, w // 8 + 3 * j:w - w // 8] = 0.75
            bars[(h, w)] = torch.from_numpy(k).cuda()
        torch.add(bars[(h, w)].expand(prob.shape[0], 1, h, w), prob, alpha=0.25, out=prob)

    eng = Engine(det, rec, pp, det_size=args.det_size, rec_size=(32, 256), prob_hook=hook)
    out = {}
    for name, kw in (("quads_none", {}), ("quads_deskew", {"quads": "deskew"})):
        ts = []
        for r in range(args.engine_warmup + args.engine_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(pages, **kw)
            if r >= args.engine_warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(spread(ts), deskewed=eng.stats["deskewed"], rectified=eng.stats["rectified"], buckets=eng.stats["buckets"],
                         crops=eng.stats["crops"])
    out["deskew_over_none_ms"] = out["quads_deskew"]["ms"] - out["quads_none"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--det-size", type=int, default=960)
    ap.add_argument("--engine-warmup", type=int, default=1)
    ap.add_argument("--engine-steps", type=int, default=3)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skew_bench needs a GPU")
    lib = _lib.load()
    n = args.pages
    distinct = [SR.rotated(synth.make_invoice(700 + i, H, W, 30)[0], ANGLES[i % len(ANGLES)], enclose=False) for i in range(min(args.distinct, n))]
    host = [distinct[i % len(distinct)] for i in range(n)]
    pages = [torch.from_numpy(p).cuda() for p in host]
    ww, _ = pipeline.doc_working_size(H, W, WORK_H)
    kernels, whole, skews = bench_kernels(lib, pages, args)
    want = [512 * np.tan(np.radians(ANGLES[i % len(ANGLES)])) for i in range(len(distinct))]
    res = {"pages": n, "distinct_pages": len(distinct), "page": [H, W], "working_size": [WORK_H, ww], "kernels": kernels,
           "kernels_ms": sum(kernels[k]["ms"] for k in TAGS), "estimate_skews": whole, "estimate_skews_ms_per_page": whole["ms"] / n,
           "byte_adds": 257 * WORK_H * ww * n,
           "byte_adds_per_s": 257.0 * WORK_H * ww * n / (kernels["skew_scores"]["ms"] * 1e-3),
           "pcie_bytes_per_page": {"scores": 257 * 8, "raw_rgb": 3 * H * W, "ratio": 257 * 8 / (3.0 * H * W)},
           "picked": [{"degrees": ANGLES[i % len(ANGLES)], "k_ideal": round(float(want[i]), 2), "k": skews[i].k, "gain": round(skews[i].gain, 4)}
                      for i in range(len(distinct))]}
    if not args.no_engine:
        res["engine"] = dict(bench_engine(host, args), det_size=args.det_size)
    res["timing"] = (f"kernels: device events of the library profiler around each launch, median of {args.reps} after {args.warmup}; "
                     f"estimate_skews and the engine: wall clock, medians")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
