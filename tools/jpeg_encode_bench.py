#!/usr/bin/env python3
"""Times the JPEG encoder (include/ocrvi.h, "JPEG encode") on ``--pages`` device-resident synthetic 960 x 1280 invoices at quality 95 in
4:2:0, through ``pipeline.JpegEncodeJob`` (what ``imencode_pages`` runs).  Prints one JSON line.

  kernels        the six launches of ``ocrvi_jpeg_encode_pages`` alone: device events around the call, and each kernel by the library's
                 per-launch profiler (a run of its own); ``--warmup`` calls first, then the median, minimum and maximum of ``--reps``
  device_route   ``imencode_pages`` as a caller sees it: table upload, allocations, launches, the lengths, the copy of the compressed bytes
                 alone, headers -- host clock around the call, the device idle before and after
  kernels_copy   the launches plus the lengths and the copy of the compressed bytes, buffers already allocated
  host_route     what a caller has without the encoder: the pixels copied device -> host (3 H W bytes a page), then PIL's
                 ``save(..., "JPEG", quality=95, subsampling=2)`` on one core and on a pool of ``min(cpus, 16)`` threads; ``null`` where PIL is
                 not importable
  pcie_bytes     what crosses the bus per page on either route
Needs a GPU: there is no fallback."""
import argparse
import concurrent.futures
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocr_vi_invoice_amd import _lib, pipeline, synth  # noqa: E402

H, W, QUALITY = 960, 1280, 95
KERNELS = ("jpeg_fdct", "jpeg_bits", "jpeg_pack", "jpeg_ffcount", "jpeg_ffscan", "jpeg_stuff")


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_bench needs a GPU")
    lib = _lib.load()
    distinct = [torch.from_numpy(synth.make_invoice(100 + i, H, W, lines=30)[0]) for i in range(min(args.pages, 16))]
    pages = [distinct[i % len(distinct)].cuda() for i in range(args.pages)]
    n = len(pages)

    job = pipeline.JpegEncodeJob(pages, QUALITY, "4:2:0").launch()
    files = job.collect()
    for _ in range(args.warmup):
        job.enqueue()
    torch.cuda.synchronize()
    # the launches alone, between two device events
    whole = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        job.enqueue()
        b.record()
        b.synchronize()
        whole.append(a.elapsed_time(b))
    # each kernel, by the library's profiler (its events sit between the launches, so this is a run of its own)
    per = {k: [] for k in KERNELS}
    lib.ocrvi_prof_enable(1)
    for _ in range(args.reps):
        lib.ocrvi_prof_reset()
        job.enqueue()
        torch.cuda.synchronize()
        rep = _lib.prof_report()
        for k in KERNELS:
            per[k].append(rep[k]["ms"])
    lib.ocrvi_prof_enable(0)
    lib.ocrvi_prof_reset()
    # launches + the lengths + the compressed bytes
    copy = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job.enqueue()
        job.collect_scans()
        copy.append((time.perf_counter() - t0) * 1e3)
    # the public call
    route = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipeline.imencode_pages(pages, QUALITY)
        if r >= args.warmup:
            route.append((time.perf_counter() - t0) * 1e3)
    assert out == files
    file_bytes = sum(len(f) for f in files)
    res = {"page": [H, W], "pages": n, "quality": QUALITY, "subsampling": "4:2:0", "file_bytes": file_bytes,
           "workspace_bytes": job._ws.numel(), "output_capacity_bytes": job.out.numel(),
           "kernels": spread(whole), "per_kernel": {k: spread(v) for k, v in per.items()}, "kernels_copy": spread(copy), "device_route": spread(route)}
    for k in ("kernels", "kernels_copy", "device_route"):
        res[k]["ms_per_page"] = res[k]["ms"] / n

    # the host route: pixels to the host, then PIL
    d2h, pil_one, pil_pool = [], [], []
    threads = min(len(os.sched_getaffinity(0)), 16)
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def save(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        return buf.getvalue()

    pool = concurrent.futures.ThreadPoolExecutor(threads)
    pil_files = None
    for r in range(args.host_reps + 1 if args.host_reps else 0):          # --host-reps 0: the device route alone
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [p.cpu().numpy() for p in pages]
        t1 = time.perf_counter()
        if r:
            d2h.append((t1 - t0) * 1e3)
        if Image is None:
            continue
        pil_files = [save(a) for a in host]
        t2 = time.perf_counter()
        list(pool.map(save, host))
        t3 = time.perf_counter()
        if r:
            pil_one.append((t2 - t1) * 1e3)
            pil_pool.append((t3 - t2) * 1e3)
    res["host_route"] = None if not d2h else {"pixels_d2h": spread(d2h), "pool_threads": threads, "pil_one_core": spread(pil_one) if pil_one else None,
                         "pil_pool": spread(pil_pool) if pil_pool else None,
                         "end_to_end_one_core_ms": statistics.median(d2h) + statistics.median(pil_one) if pil_one else None,
                         "end_to_end_pool_ms": statistics.median(d2h) + statistics.median(pil_pool) if pil_pool else None,
                         "same_bytes_as_device": pil_files == files if pil_files is not None else None}
    res["pcie_bytes_per_page"] = {"device_route": file_bytes / n + 8, "host_route": 3 * H * W, "ratio": (file_bytes / n + 8) / (3 * H * W)}
    res["timing"] = (f"kernels: device events around the six launches, per kernel the library profiler, median of {args.reps} after {args.warmup}; "
                     f"kernels_copy, device_route: host clock, device idle at both ends, median of {args.reps}; host route: host clock, median of "
                     f"{args.host_reps} passes after one")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
