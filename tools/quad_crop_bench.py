#!/usr/bin/env python3
"""Times the oriented text crop (include/ocrvi.h, "Oriented text crops") against the rectangle crop it stands next to.  Prints one JSON line.

Kernels: 256 crops of text lines of about 300 x 24 px on a 1000 x 760 page, out 32 x 256, once tilted by +-6 degrees (descriptors from
``ocrvi_quad_crops``) and once axis-aligned (translation descriptors).  Per case three calls on the same crops, alternating group by group
in one run: ``ocrvi_crop_quad_resize_normalize_pages`` in its tile form (16-byte aligned output), the same entry in its direct form (it
takes that form for an output that is not 16-byte aligned: the output starts 4 bytes in), and ``ocrvi_crop_resize_normalize_pages`` on the
bounding rectangles of the same quads.  Device events around ``--inner`` back-to-back calls, ``--warmup`` groups first, the median of
``--reps`` groups divided by ``--inner``, with the minimum and maximum.
Engine: random weights, f16x2, ``--engine-pages`` synthetic 1000 x 760 invoices whose detector map gets lines tilted by +-6 degrees painted
in; a host clock around ``run`` (it ends synchronised), ``crop="rect"`` and ``crop="quad"`` alternating run by run, the median.
Needs a GPU: there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocr_vi_invoice_amd import _lib, pipeline, synth  # noqa: E402

PAGE_HW = (1000, 760)
OUT = (32, 256)


def line_quads(n, tilt_deg, seed=1):
    """n text lines of about 300 x 24 px inside the page, tilted by +-tilt_deg: float64 [n, 4, 2]."""
    rng = np.random.default_rng(seed)
    H, W = PAGE_HW
    out = []
    for i in range(n):
        a = math.radians(tilt_deg if i % 2 == 0 else -tilt_deg)
        u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
        L, T = rng.uniform(280, 320), rng.uniform(20, 28)
        c = np.array([rng.uniform(200, W - 200), rng.uniform(60, H - 60)])
        if tilt_deg == 0:
            c, L, T = np.rint(c), float(round(L)), float(round(T))
            q0 = c - np.array([L // 2, T // 2])
            out.append([q0, q0 + (L - 1, 0), q0 + (L - 1, T - 1), q0 + (0, T - 1)])
        else:
            out.append([c - u * L / 2 - v * T / 2, c + u * L / 2 - v * T / 2, c + u * L / 2 + v * T / 2, c - u * L / 2 + v * T / 2])
    return np.ascontiguousarray(out, np.float64)


def descriptors(quads, translation):
    n = len(quads)
    crops, mats = np.empty((n, 4), np.int32), np.empty((n, 9), np.float64)
    ids, hw = np.zeros(n, np.int32), np.ascontiguousarray(np.broadcast_to(np.asarray(PAGE_HW, np.int32), (n, 2)))
    flags = np.full(n, 1 if translation else 0, np.int32)       # a flagged quad gets the translation descriptor of its bounding rectangle
    _lib.check(_lib.load().ocrvi_quad_crops(quads.ctypes.data, flags.ctypes.data, n, ids.ctypes.data, hw.ctypes.data, crops.ctypes.data, mats.ctypes.data))
    rects = np.array([(0,) + pipeline.crop_rect(PAGE_HW, np.stack([np.floor(q.min(0)), np.ceil(q.max(0))]).astype(np.int64)) for q in quads], np.int32)
    return crops, mats, rects


def timed_alternating(fns, warmup, reps, inner):
    """{name: median / min / max ms of one call}; the groups of the calls alternate, so drift hits them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            for _ in range(inner):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return {k: {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}


def bench_kernels(args, tilt):
    lib = _lib.load()
    page = torch.from_numpy(synth.make_invoice(5, *PAGE_HW, lines=30)[0]).cuda()
    table = torch.tensor([(page.data_ptr(), PAGE_HW[0], PAGE_HW[1], 0)], dtype=torch.int64, device="cuda")
    crops, mats, rects = descriptors(line_quads(args.crops, tilt), translation=(tilt == 0))
    d_crops, d_mats, d_rects = torch.from_numpy(crops).cuda(), torch.from_numpy(mats).cuda(), torch.from_numpy(rects).cuda()
    B, n = len(crops), len(crops) * 3 * OUT[0] * OUT[1]
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    aligned, offset = buf.data_ptr(), buf.data_ptr() + 4

    def quad(ptr):
        return lambda: _lib.check(lib.ocrvi_crop_quad_resize_normalize_pages(0, table.data_ptr(), 1, d_crops.data_ptr(), d_mats.data_ptr(), B, OUT[0],
                                                                             OUT[1], ptr, st))

    fns = {"quad_tile": quad(aligned), "quad_direct": quad(offset),
           "rect": lambda: _lib.check(lib.ocrvi_crop_resize_normalize_pages(0, table.data_ptr(), 1, d_rects.data_ptr(), B, OUT[0], OUT[1], aligned, st))}
    # the two forms write the same values
    fns["quad_tile"]()
    a = buf[:n].clone()
    fns["quad_direct"]()
    assert torch.equal(a, buf[1:n + 1])
    res = timed_alternating(fns, args.warmup, args.reps, args.inner)
    res["crops"], res["out"] = B, list(OUT)
    res["crop_w_h_median"] = [int(np.median(crops[:, 1])), int(np.median(crops[:, 2]))]
    res["rect_w_h_median"] = [int(np.median(rects[:, 3])), int(np.median(rects[:, 4]))]
    res["out_gbs_quad_tile"] = n * 4 / (res["quad_tile"]["ms"] * 1e-3) / 1e9
    return res


def bench_engine(args):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    from ocr_vi_invoice_amd.engine import plan_buckets
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    pages = [synth.make_invoice(30 + i, *PAGE_HW, lines=12)[0] for i in range(args.engine_pages)]
    (H, W), = set(plan_buckets([PAGE_HW] * len(pages), 960)[0])
    k = np.zeros((1, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for j in range((H - 80) // 80):           # lines of about 0.55 W x 22 px of the map, tilted by +-6 degrees, 80 rows apart (they do not touch)
        a = math.radians(6 if j % 2 == 0 else -6)
        dx, dy = xx - W / 2, yy - (60 + 80 * j)
        k[0][(np.abs(dx * math.cos(a) + dy * math.sin(a)) <= 0.275 * W) & (np.abs(-dx * math.sin(a) + dy * math.cos(a)) <= 11)] = 0.75
    kern = torch.from_numpy(k).cuda()

    def hook(prob, idx):
        torch.add(kern[None].expand(len(idx), -1, -1, -1), prob, alpha=0.25, out=prob)

    pp = DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)
    eng = {c: Engine(det, rec, pp, det_size=960, det_chunk=4, prob_hook=hook, crop=c) for c in ("rect", "quad")}
    t = {"rect": [], "quad": []}
    for r in range(args.engine_warmup + args.engine_reps):
        for c in ("rect", "quad"):
            t0 = time.perf_counter()
            eng[c].run(pages)
            if r >= args.engine_warmup:
                t[c].append(time.perf_counter() - t0)
    out = {"pages": len(pages), "size": list(PAGE_HW), "det_size": 960, "dtype": "f16x2", "crops": eng["quad"].stats["crops"],
           "boxes_per_page": eng["quad"].stats["crops"] / len(pages), "quad_host_ms_per_run": eng["quad"].stats["quad_s"] * 1e3}
    for c in ("rect", "quad"):
        out[f"run_{c}_ms"] = statistics.median(t[c]) * 1e3
        out[f"run_{c}_ms_min_max"] = [min(t[c]) * 1e3, max(t[c]) * 1e3]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--crops", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--engine-pages", type=int, default=16)
    ap.add_argument("--engine-warmup", type=int, default=2)
    ap.add_argument("--engine-reps", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quad_crop_bench needs a GPU")
    out = {"tool": "quad_crop_bench", "tilted_6_degrees": bench_kernels(args, 6), "axis_aligned_translation": bench_kernels(args, 0)}
    if not args.no_engine:
        out["engine"] = bench_engine(args)
    out["timing"] = (f"kernels: device events around {args.inner} calls, median of {args.reps} groups after {args.warmup} warm-up groups, the three "
                     f"calls alternating; engine: host clock around run(), median of {args.engine_reps} after {args.engine_warmup}, modes alternating")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
