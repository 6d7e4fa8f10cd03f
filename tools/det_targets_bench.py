#!/usr/bin/env python3
"""Times ``DetectionDataset`` (ocr_vi_invoice_amd/data.py) on one batch: ``--samples`` synthetic 1000 x 1400 pages with ``--quads``
quadrilateral annotations each, ``S = 640``, with and without the threshold maps.  Prints one JSON line.

* ``host_geometry``: ``ocrvi_db_target_jobs`` for the whole batch (validity, area, perimeter, Clipper's shrinking and dilating offsets
  and their closing unions) on the host pool and on one thread, wall clock.
* ``upload``: the one pinned copy of page table, rows, jobs and points, by device events.
* ``db_target_init`` / ``db_target_fill`` / ``resize_normalize_pad``: the three launches, by the library profiler's device events.
* ``batch``: ``next(ds.batches(n))`` end to end with the pages already on the device, host clock around a synchronised call.
* ``detector_forward``: ``DBNetPP.forward`` (f16x2) on the batch just built, in the same run, for scale.
There is no cv2 / pyclipper / shapely here to time the reference's own dataloader against: ``reference_dataloader`` is "not measured".
Needs a GPU: there is no fallback."""
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

from ocr_vi_invoice_amd import _lib, data, synth  # noqa: E402

H, W, S = 1000, 1400, 640


def make_samples(n, quads):
    rng = np.random.default_rng(13)
    out = []
    cols = 4
    rows = (quads + cols - 1) // cols
    for i in range(n):
        img = synth.make_invoice(300 + i, H, W, lines=30)[0]
        polys = []
        for q in range(quads):
            r, c = divmod(q, cols)
            cx, cy = (c + 0.5) * W / cols, (r + 0.5) * H / rows
            hw, hh = rng.uniform(60, 0.45 * W / cols), rng.uniform(6, 0.4 * H / rows)
            a = rng.uniform(-0.03, 0.03)
            corners = [(-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh)]
            polys.append(np.asarray([(cx + x * np.cos(a) - y * np.sin(a), cy + x * np.sin(a) + y * np.cos(a)) for x, y in corners], np.float32))
        out.append((torch.from_numpy(img).cuda(), polys))
    return out


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def bench(samples, thresh, args):
    lib = _lib.load()
    n = len(samples)
    ds = data.DetectionDataset(samples=samples, image_size=S, thresh_maps=thresh)
    sizes, polys = [(H, W)] * n, [p for _, p in samples]
    host = {"pool": [], "one_thread": []}
    for r in range(args.warmup + args.reps):
        for name, threads in (("pool", None), ("one_thread", 1)):
            t0 = time.perf_counter()
            jobs, points = data.target_jobs(sizes, polys, 0.4, thresh, threads=threads)
            if r >= args.warmup:
                host[name].append((time.perf_counter() - t0) * 1e3)
    words = n * 8 + n * 4 + jobs.size + points.size
    pinned = torch.empty(words, dtype=torch.int32).pin_memory()
    up = []
    for r in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d = pinned.to("cuda", non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            up.append(e0.elapsed_time(e1))
    kernels = {"db_target_init": [], "db_target_fill": [], "resize_normalize_pad": []}
    wall = []
    for r in range(args.warmup + args.reps):
        prof = r >= args.warmup
        torch.cuda.synchronize()
        if prof:
            lib.ocrvi_prof_enable(1)
            lib.ocrvi_prof_reset()
        t0 = time.perf_counter()
        batch = next(ds.batches(n))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if prof:
            rep = _lib.prof_report()
            lib.ocrvi_prof_enable(0)
            for k in kernels:
                kernels[k].append(rep[k]["ms"])
            wall.append((t1 - t0) * 1e3)
    lib.ocrvi_prof_reset()
    res = {"jobs": int(len(jobs)), "points": int(len(points)), "upload_bytes": 4 * words,
           "host_geometry_pool": spread(host["pool"]), "host_geometry_one_thread": spread(host["one_thread"]), "pool_threads": data._threads(),
           "upload": spread(up), "batch": spread(wall)}
    for k, v in kernels.items():
        res[k] = spread(v)
    res["db_target_init"]["bytes"] = 16 * n * S * S
    res["resize_normalize_pad"]["bytes"] = 12 * n * S * S + 3 * n * H * W
    return res, batch


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--quads", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_targets_bench needs a GPU")
    samples = make_samples(args.samples, args.quads)
    out = {"page": [H, W], "S": S, "samples": args.samples, "quads_per_sample": args.quads}
    out["validation"], batch = bench(samples, False, args)
    out["with_thresh_maps"], _ = bench(samples, True, args)
    from ocr_vi_invoice_amd import DBNetPP, weights
    model = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    fwd = []
    for r in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(batch["image"])
        e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            fwd.append(e0.elapsed_time(e1))
    out["detector_forward"] = dict(spread(fwd), dtype="f16x2", shape=list(batch["image"].shape))
    out["reference_dataloader"] = "not measured (cv2, pyclipper and shapely are not importable here)"
    out["timing"] = (f"median, minimum and maximum of {args.reps} after {args.warmup}; kernels by the library profiler's device events, upload and "
                     "detector by device events, host geometry and batch by the host clock")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
