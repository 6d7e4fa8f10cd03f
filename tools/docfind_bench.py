#!/usr/bin/env python3
"""Times the document finder (include/ocrvi.h, "Document finder") on 64 pages of 960 x 1280 and on 16 pages of 3000 x 4000 (rows x
columns), synthetic photos of a bright sheet on a dark, noisy table.  Prints one JSON line.

Kernels: the library's per-launch profiler brackets each of the five launches of ``ocrvi_doc_mask_pages`` (all pages in one page table)
with device events; ``--warmup`` calls first, then the median, minimum and maximum of ``--reps``.  Host finish: ``ocrvi_document_contour_bits``
over the pages' bit masks, one core, wall clock.  ``find_document_quads`` on device tensors: wall clock around the call (table upload,
launches, the copy of the bit masks, the host finish).  PCIe: the bit-mask bytes that come back against 3 H W.
Beside them the alternative a caller has without this feature: the pages copied to pageable host memory (``.cpu()``), then
tests/docfind_ref.py's numpy statement of the mask and its Python contour half on the host, on ``--alt-pages`` pages.
The photos of one size are ``--distinct`` different pages repeated (each copy its own device tensor).  Needs a GPU: there is no fallback."""
import argparse
import ctypes
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

import docfind_ref as DR  # noqa: E402
from ocr_vi_invoice_amd import _lib, pipeline  # noqa: E402

WORK_H = 500
SETS = (("960x1280", 960, 1280, 64), ("3000x4000", 3000, 4000, 16))


def make_photo(seed, h, w):
    rng = np.random.default_rng(seed)
    quad = np.array([(0.12, 0.10), (0.86, 0.14), (0.90, 0.88), (0.08, 0.92)]) * (w, h) + rng.integers(-20, 21, (4, 2))
    doc = DR._inside(h, w, quad)
    ys = np.arange(h)[:, None]
    xs = np.arange(w)[None, :]
    text = doc & ((ys // max(h // 90, 4)) % 3 == 0) & ((xs // max(w // 14, 8)) % 4 != 3)
    img = np.where(doc, np.where(text, 70, 225), 45 + 12 * (((xs + 2 * ys) // 24) % 2)) + rng.integers(-10, 11, (h, w))
    img = np.clip(img, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([img, img, img], 2))


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} if v else None


def bench_set(lib, h, w, n, args):
    distinct = [make_photo(500 + i, h, w) for i in range(min(args.distinct, n))]
    pages = [torch.from_numpy(distinct[i % len(distinct)]).cuda() for i in range(n)]
    ww, ratio = pipeline.doc_working_size(h, w, WORK_H)
    wpr = (ww + 31) // 32
    for _ in range(args.warmup):
        bits, _ = pipeline.doc_mask_bits(pages, WORK_H)
    torch.cuda.synchronize()
    tags = ("doc_grey", "doc_smooth", "doc_hist", "doc_otsu", "doc_mask")
    t = {k: [] for k in tags}
    lib.ocrvi_prof_enable(1)
    for _ in range(args.reps):
        lib.ocrvi_prof_reset()
        bits, _ = pipeline.doc_mask_bits(pages, WORK_H)
        torch.cuda.synchronize()
        rep = _lib.prof_report()
        for k in tags:
            t[k].append(rep[k]["ms"])
    lib.ocrvi_prof_enable(0)
    lib.ocrvi_prof_reset()
    host = bits.cpu().numpy()
    quad, found = np.zeros((4, 2), np.int32), ctypes.c_int32(0)
    finish, kinds = [], []
    for r in range(args.reps):
        t0 = time.perf_counter()
        for i in range(n):
            _lib.check(lib.ocrvi_document_contour_bits(host[i].ctypes.data, WORK_H, ww, quad.ctypes.data, ctypes.byref(found)))
            if r == 0:
                kinds.append(found.value)
        finish.append((time.perf_counter() - t0) * 1e3)
    whole = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quads = pipeline.find_document_quads(pages)
        if r >= args.warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    res = {"pages": n, "distinct_pages": len(distinct), "working_size": [WORK_H, ww], "polygons_found": sum(k == 1 for k in kinds),
           "kernels": {k: spread(v) for k, v in t.items()}, "host_finish_one_core": spread(finish), "find_document_quads": spread(whole)}
    res["kernels_ms_per_page"] = sum(res["kernels"][k]["ms"] for k in tags) / n
    res["grey_read_gb_per_s"] = 3.0 * h * w * n / (res["kernels"]["doc_grey"]["ms"] * 1e-3) / 1e9
    res["host_finish_ms_per_page"] = res["host_finish_one_core"]["ms"] / n
    res["find_document_quads_ms_per_page"] = res["find_document_quads"]["ms"] / n
    res["pcie_bytes_per_page"] = {"bit_mask": WORK_H * wpr * 4, "raw_rgb": 3 * h * w, "ratio": WORK_H * wpr * 4 / (3.0 * h * w)}
    # the alternative: pixels to the host, the finder there
    copy, mask_t, contour_t, agree = [], [], [], True
    for i in range(min(args.alt_pages, n)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = pages[i].cpu().numpy()
        t1 = time.perf_counter()
        st = DR.stages(img, WORK_H)
        t2 = time.perf_counter()
        q, _ = DR.document_contour(st["mask"])
        t3 = time.perf_counter()
        copy.append((t1 - t0) * 1e3)
        mask_t.append((t2 - t1) * 1e3)
        contour_t.append((t3 - t2) * 1e3)
        agree = agree and (q is None) == (quads[i] is None) and (q is None or np.array_equal(q.astype(np.float64) * ratio, quads[i]))
    res["alternative_per_page"] = {"pages": len(copy), "copy_to_host": spread(copy), "numpy_mask": spread(mask_t), "python_contours": spread(contour_t),
                                   "same_quads_as_the_device_path": agree}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--alt-pages", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("docfind_bench needs a GPU")
    lib = _lib.load()
    out = {"work_h": WORK_H}
    for name, h, w, n in SETS:
        out[name] = bench_set(lib, h, w, n, args)
    out["timing"] = (f"kernels: device events of the library profiler around each launch, median of {args.reps} after {args.warmup}; host finish, "
                     f"find_document_quads and the alternative: wall clock, medians")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
