#!/usr/bin/env python3
"""Times the result overlay (include/ocrvi.h, "Result overlay") on ``--pages`` device-resident synthetic 960 x 1280 invoices, each with
``--boxes`` polygons of 4..40 vertices, thickness 2.  Prints one JSON line.

  kernel         the one launch of ``ocrvi_overlay_pages`` alone (tables already on the device): device events around the call; painting is
                 idempotent, so the same pages are painted again; ``--warmup`` calls first, then the median, minimum and maximum of ``--reps``
  segments       ``ocrvi_overlay_segments`` through ``pipeline.overlay_segments`` (host only): host clock
  device_route   ``draw_boxes_pages`` as a caller sees it: the segment build, the copies of the pages (device to device), the upload of
                 the tables, the launch -- host clock around the call, the device idle before and after
  host_route     what a caller has without it: the pixels copied device -> host (3 H W bytes a page), the outlines drawn with PIL's
                 ``ImageDraw.line(width=2)`` (no labels) on one core and on a pool of ``min(cpus, 16)`` threads, and the pixels copied back;
                 ``null`` where PIL is not importable
  pcie_bytes     what crosses the bus per page on either route
Needs a GPU: there is no fallback."""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocr_vi_invoice_amd import _lib, pipeline, synth  # noqa: E402

H, W = 960, 1280


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def make_boxes(seed, n):
    """n text-line-like polygons: 4..40 vertices on a flat ellipse around a random centre, unclipped (some cross the page border)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(4, 41))
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        rx, ry = rng.uniform(30, 160), rng.uniform(8, 24)
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        out.append(np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1).astype(np.int32))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--boxes", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench needs a GPU")
    lib = _lib.load()
    distinct = [torch.from_numpy(synth.make_invoice(100 + i, H, W, lines=30)[0]) for i in range(min(args.pages, 16))]
    pages = [distinct[i % len(distinct)].cuda() for i in range(args.pages)]
    boxes = [make_boxes(i, args.boxes) for i in range(args.pages)]
    n = len(pages)

    build = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        segs, prims, offs = pipeline.overlay_segments(boxes, None, [(H, W)] * n)
        build.append((time.perf_counter() - t0) * 1e3)
    # the launch alone, on copies
    work = [p.clone() for p in pages]
    blob, launch_args = pipeline.overlay_upload(work, segs, prims, offs)
    stream = torch.cuda.current_stream().cuda_stream
    kern = []
    for r in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.ocrvi_overlay_pages(0, *launch_args, stream))
        b.record()
        b.synchronize()
        if r >= args.warmup:
            kern.append(a.elapsed_time(b))
    # the public call
    route = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipeline.draw_boxes_pages(pages, boxes)
        torch.cuda.synchronize()
        if r >= args.warmup:
            route.append((time.perf_counter() - t0) * 1e3)
    assert all(torch.equal(a, b) for a, b in zip(out, work))
    painted = sum(int((a != b).any(-1).sum()) for a, b in zip(out[:4], pages[:4])) / min(n, 4)
    res = {"page": [H, W], "pages": n, "boxes_per_page": args.boxes, "thickness": 2, "segments": int(len(segs)), "primitives": int(len(prims)),
           "painted_pixels_per_page": painted, "table_bytes": int(blob.numel() * 4),
           "kernel": spread(kern), "segments_build": spread(build), "device_route": spread(route)}
    for k in ("kernel", "segments_build", "device_route"):
        res[k]["ms_per_page"] = res[k]["ms"] / n

    # the host route: pixels to the host, PIL outlines, pixels back
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        Image = None
    threads = min(len(os.sched_getaffinity(0)), 16)

    def draw(job):
        a, bs = job
        im = Image.fromarray(a)
        d = ImageDraw.Draw(im)
        for b in bs:
            pts = [tuple(int(v) for v in p) for p in b]
            d.line(pts + pts[:1], fill=(0, 255, 0), width=2)
        return np.asarray(im)

    pool = concurrent.futures.ThreadPoolExecutor(threads)
    d2h, pil_one, pil_pool, h2d = [], [], [], []
    for r in range(args.host_reps + 1 if args.host_reps else 0):          # --host-reps 0: the device route alone
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [p.cpu().numpy() for p in pages]
        t1 = time.perf_counter()
        if Image is None:
            drawn, t2, t3 = host, t1, t1
        else:
            drawn = [draw(j) for j in zip(host, boxes)]
            t2 = time.perf_counter()
            list(pool.map(draw, zip(host, boxes)))
            t3 = time.perf_counter()
        back = [torch.from_numpy(a).cuda() for a in drawn]
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        del back
        if r:
            d2h.append((t1 - t0) * 1e3)
            h2d.append((t4 - t3) * 1e3)
            if Image is not None:
                pil_one.append((t2 - t1) * 1e3)
                pil_pool.append((t3 - t2) * 1e3)
    res["host_route"] = None if not d2h else {
        "pixels_d2h": spread(d2h), "pixels_h2d": spread(h2d), "pool_threads": threads,
        "pil_one_core": spread(pil_one) if pil_one else None, "pil_pool": spread(pil_pool) if pil_pool else None,
        "d2h_plus_pil_one_core_ms": statistics.median(d2h) + statistics.median(pil_one) if pil_one else None,
        "d2h_plus_pil_pool_ms": statistics.median(d2h) + statistics.median(pil_pool) if pil_pool else None}
    res["pcie_bytes_per_page"] = {"device_route": blob.numel() * 4 / n, "host_route_d2h": 3 * H * W, "host_route_round_trip": 6 * H * W,
                                  "ratio_to_d2h": blob.numel() * 4 / n / (3 * H * W)}
    res["timing"] = (f"kernel: device events around the launch, median of {args.reps} after {args.warmup}; segments_build, device_route: host "
                     f"clock, device idle at both ends, median of {args.reps}; host route: host clock, median of {args.host_reps} passes after one")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
