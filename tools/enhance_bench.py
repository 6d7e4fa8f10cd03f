#!/usr/bin/env python3
"""Times enhance_document on the device (include/ocrvi.h, "enhance_document"): every stage entry and ``ocrvi_enhance_u8`` on a 1000 x 760
and a 1400 x 1000 page, then ``Engine.run`` on a folder of such pages with and without ``enhance``.  Prints one JSON line.

Stages: device events around ``--inner`` back-to-back calls on one stream, ``--warmup`` such groups first, the median of ``--reps`` groups
divided by ``--inner``.  ``nlm_gsqdiff_per_s`` is the definition's work -- h w 441 offsets x 49 template pixels x 3 planes squared
differences -- over the NLM time (the kernel shares each row's 7-sum down an 8-row strip and forms it from packed dot products).
Engine: random weights, f16x2, ``--engine-pages`` noisy synthetic invoices of the two sizes; a host clock around ``run`` (it ends
synchronised), the two settings alternating run by run, the median.  Needs a GPU: there is no fallback."""
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

from ocr_vi_invoice_amd import _lib, synth  # noqa: E402

SIZES = [(1000, 760), (1400, 1000)]


def noisy_page(seed, h, w):
    img = synth.make_invoice(seed, h, w, lines=12)[0]
    noise = np.random.default_rng(seed).normal(0, 6, img.shape)
    return np.ascontiguousarray(np.clip(img + noise, 0, 255).round().astype(np.uint8))


def timed(fn, warmup, reps, inner):
    """Median, minimum and maximum milliseconds of one call of ``fn`` (enqueue-only on the current stream)."""
    for _ in range(warmup):
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def bench_stages(lib, h, w, args):
    page = torch.from_numpy(noisy_page(5, h, w)).cuda()
    n = C.c_size_t()
    _lib.check(lib.ocrvi_enhance_workspace_bytes(h, w, C.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    lab, tmp, out = torch.empty_like(page), torch.empty_like(page), torch.empty_like(page)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ocrvi_rgb_to_lab_u8(0, page.data_ptr(), h, w, lab.data_ptr(), st))           # a real Lab page for the Lab stages
    res = {}
    for name, src in (("rgb_to_lab", page), ("lab_to_rgb", lab), ("nlm_lab", lab), ("sharpen", page)):
        fn = getattr(lib, f"ocrvi_{name}_u8")
        res[name] = timed(lambda: _lib.check(fn(0, src.data_ptr(), h, w, tmp.data_ptr(), st)), args.warmup, args.reps, args.inner)
    res["clahe_lab"] = timed(lambda: _lib.check(lib.ocrvi_clahe_lab_u8(0, lab.data_ptr(), h, w, tmp.data_ptr(), ws.data_ptr(), ws.numel(), st)),
                             args.warmup, args.reps, args.inner)
    res["enhance"] = timed(lambda: _lib.check(lib.ocrvi_enhance_u8(0, page.data_ptr(), h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), st)),
                           args.warmup, args.reps, args.inner)
    res["nlm_gsqdiff_per_s"] = h * w * 441 * 49 * 3 / (res["nlm_lab"]["ms"] * 1e-3) / 1e9
    res["enhance_mpixel_per_s"] = h * w / (res["enhance"]["ms"] * 1e-3) / 1e6
    return res


def bench_engine(args):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    eng = Engine(det, rec, DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6), det_size=960, det_chunk=4)
    pages = [noisy_page(30 + i, *SIZES[i % 2]) for i in range(args.engine_pages)]
    t = {False: [], True: []}
    for r in range(args.engine_warmup + args.engine_reps):
        for enh in (False, True):
            t0 = time.perf_counter()
            eng.run(pages, None, enhance=enh)
            if r >= args.engine_warmup:
                t[enh].append(time.perf_counter() - t0)
            assert eng.stats["enhanced"] == (len(pages) if enh else 0)
    plain, enh = statistics.median(t[False]), statistics.median(t[True])
    return {"pages": len(pages), "sizes": SIZES, "det_size": 960, "dtype": "f16x2", "run_ms": plain * 1e3, "run_enhance_ms": enh * 1e3,
            "run_ms_min_max": [min(t[False]) * 1e3, max(t[False]) * 1e3], "run_enhance_ms_min_max": [min(t[True]) * 1e3, max(t[True]) * 1e3],
            "enhance_ms_per_page": (enh - plain) * 1e3 / len(pages), "crops": eng.stats["crops"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--engine-pages", type=int, default=8)
    ap.add_argument("--engine-warmup", type=int, default=2)
    ap.add_argument("--engine-reps", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("enhance_bench needs a GPU")
    lib = _lib.load()
    _lib.check(lib.ocrvi_enhance_init(0))
    out = {f"{h}x{w}": bench_stages(lib, h, w, args) for h, w in SIZES}
    if not args.no_engine:
        out["engine"] = bench_engine(args)
    out["timing"] = (f"stages: device events around {args.inner} calls, median of {args.reps} after {args.warmup} warm-up groups; engine: host clock "
                     f"around run(), median of {args.engine_reps} after {args.engine_warmup}, settings alternating")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
