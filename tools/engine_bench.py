#!/usr/bin/env python3
"""Throughput of the batched engine (ocr_vi_invoice_amd.engine.Engine) on bench.py's synthetic invoices, and the fused page-table
pre-processing kernel against the two-kernel path it replaces.  Prints ONE JSON line.

  uniform   64 pages of 960x1280 at det_size 1280: the identity resize, bench.py's headline shape
  mixed     64 pages drawn from five aspect ratios (A4 portrait, landscape, tall receipt, square, wide strip) at det_size 960
  preproc   one 16-page chunk: ocrvi_resize_normalize_pages against ocrvi_resize_u8 per page + ocrvi_normalize_u8 (HIP events)

Both runs use SVTRv2-base and DBNet++ with bench.py's seeded weights in f16x2, crops of 48x320 in batches of 256, det_chunk 16, and
bench.py's map blend through ``prob_hook``: every page's ground-truth line boxes, scaled to its bucket and shrunk by the DB shrink rule,
at 0.75 + 0.25 binary (elsewhere 0.25 binary).  Each ``run`` drains at its end (bench.py's timed region carries the recogniser's last
partial batch over into the next step instead).
``--binary-head`` repeats the uniform / mixed sets with ``Engine(binary_head=True)`` under the key ``runs_binary_head``.
``--confidence`` repeats them with ``Engine(confidence=True)`` under the key ``runs_confidence``.
``--quads`` adds the four-point rectification: under ``warp`` the kernel time of one 4000x3000 page warped to about 3586x2567 and of a
16-page chunk of them through ``ocrvi_warp_perspective_pages`` (HIP events around every launch, warm, median), and under ``runs_quads`` the
uniform / mixed sets with a quad on every page (``Engine.run(pages, quads)``: the page's own corners pulled in by a few per cent)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXED = [(1754, 1240), (960, 1280), (1600, 600), (1000, 1000), (700, 1400)]


def inset_quad(h, w):
    """The page's corners pulled in by 1.5 to 4 per cent, each by another amount: a mild perspective, as a phone photo has."""
    return [(0.03 * w, 0.02 * h), (0.97 * w, 0.035 * h), (0.96 * w, 0.98 * h), (0.015 * w, 0.97 * h)]


def make_set(sizes, lines, det_size, with_quads=False):
    import numpy as np
    import torch
    from bench import shrink_box
    from ocr_vi_invoice_amd import pipeline, synth
    from ocr_vi_invoice_amd.engine import plan_rectified
    quads = [inset_quad(h, w) for h, w in sizes] if with_quads else None
    _, _, shapes, scales, _ = plan_rectified(sizes, quads, det_size)
    pages, kern = [], []
    for i, ((h, w), (H, W), (sh, sw)) in enumerate(zip(sizes, shapes, scales)):
        img, boxes = synth.make_invoice(i, h, w, lines)
        pages.append(img)
        k = np.zeros((1, H, W), np.float32)
        fwd = pipeline.four_point_geometry(quads[i])[0] if with_quads else None
        for x, y, bw, bh in boxes:
            if fwd is not None:      # the line box in the rectified page: the bounding rectangle of its image under the forward matrix
                c = np.asarray([(x, y, 1), (x + bw, y, 1), (x + bw, y + bh, 1), (x, y + bh, 1)], np.float64) @ fwd.T
                c = c[:, :2] / c[:, 2:3]
                x, y = max(float(c[:, 0].min()), 0.0), max(float(c[:, 1].min()), 0.0)
                bw, bh = float(c[:, 0].max()) - x, float(c[:, 1].max()) - y
            x0, y0 = int(x * sw), int(y * sh)
            bw, bh = int((x + bw) * sw) - x0, int((y + bh) * sh) - y0
            if bw >= 4 and bh >= 4:
                sx, sy, sw_, sh_ = shrink_box(x0, y0, bw, bh)
                k[0, sy:sy + sh_, sx:sx + sw_] = 0.75
        kern.append(torch.from_numpy(k).cuda())
    return pages, kern, quads


def run_set(name, engine_kw, sizes, det_size, args, det, rec, pp, with_quads=False):
    import torch
    from ocr_vi_invoice_amd import Engine
    pages, kern, quads = make_set(sizes, args.lines, det_size, with_quads)

    def hook(prob, idx):
        torch.add(torch.stack([kern[i] for i in idx]), prob, alpha=0.25, out=prob)

    eng = Engine(det, rec, pp, det_size=det_size, prob_hook=hook, **engine_kw)
    run = (lambda: eng.run(pages, quads)) if with_quads else (lambda: eng.run(pages))
    for _ in range(args.warmup):
        run()
    ts, stats = [], []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        ts.append(time.perf_counter() - t0)
        stats.append(dict(eng.stats))
    ts.sort()
    med = ts[len(ts) // 2]
    st = stats[0]
    per_stage = {k: round(sum(s[k] for s in stats) / len(stats) * 1e3, 2) for k in ("launch_s", "det_wait_s", "post_s", "rec_wait_s", "total_s")}
    extra = {"rectified": st["rectified"], "ms_per_run_all": [round(t * 1e3, 2) for t in ts]} if "rectified" in st else {}
    del eng
    torch.cuda.empty_cache()
    return {"set": name, "det_size": det_size, "pages": len(pages), "pages_per_s": round(len(pages) / med, 3), "ms_per_run_median": round(med * 1e3, 2),
            "ms_per_run_min_max": [round(ts[0] * 1e3, 2), round(ts[-1] * 1e3, 2)], "buckets": st["buckets"], "crops": st["crops"],
            "rec_batches": st["rec_batches"], "boxes_per_page_min_max": [min(len(o[0]) for o in out), max(len(o[0]) for o in out)],
            "host_ms_per_run": {k.replace("_s", ""): v for k, v in per_stage.items()}, **extra,
            "host_stage_note": "launch = staging (host copy into pinned memory) + enqueue; det_wait / rec_wait = host blocked on the device; "
                               "post = ocrvi_db_boxes_pages"}


def time_preproc(iters=50):
    """16-page chunk: the fused kernel against resize_u8 per page + normalize_u8 on the chunk, for three source sizes."""
    import numpy as np
    import torch
    from ocr_vi_invoice_amd import _lib, synth
    lib = _lib.load()
    H, W, n = 960, 1280, 16
    out = []
    for src_h, src_w, dst_w in ((960, 1280, 1280), (1920, 2560, 1280), (1754, 1240, 672)):
        img = torch.from_numpy(synth.make_invoice(1, src_h, src_w, 30)[0]).cuda()
        pages = [img.clone() for _ in range(n)]
        tab = torch.from_numpy(np.asarray([(p.data_ptr(), src_h, src_w, 0) for p in pages], np.int64)).cuda()
        x = torch.empty((n, 3, H, dst_w), device="cuda")
        u8 = torch.empty((n, H, dst_w, 3), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def fused():
            _lib.check(lib.ocrvi_resize_normalize_pages(0, tab.data_ptr(), n, H, dst_w, x.data_ptr(), st))

        def two():
            for i, p in enumerate(pages):
                _lib.check(lib.ocrvi_resize_u8(0, p.data_ptr(), src_h, src_w, u8[i].data_ptr(), H, dst_w, st))
            _lib.check(lib.ocrvi_normalize_u8(0, u8.data_ptr(), n, H, dst_w, x.data_ptr(), st))

        res = {"src": f"{src_h}x{src_w}", "dst": f"{H}x{dst_w}", "pages": n}
        for name, fn in (("fused", fused), ("two_kernel", two)):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / iters
            res[name + "_ms"] = round(ms, 4)
        wbytes = n * H * dst_w * 12                            # fp32 planes: what dominates
        res["fused_write_gbs"] = round(wbytes / (res["fused_ms"] / 1e3) / 1e9, 1)
        res["speedup"] = round(res["two_kernel_ms"] / res["fused_ms"], 3)
        out.append(res)
    return out


def time_warp(iters=30):
    """One 12-megapixel page (4000 x 3000, h x w) warped by a real quad to about 3586 x 2567, and a 16-page chunk of them through the page
    tables.  A pair of events around every launch, warm, the median; bytes = the rectified page written + the source pixels inside the quad."""
    import numpy as np
    import torch
    from ocr_vi_invoice_amd import _lib, pipeline, synth
    lib = _lib.load()
    sh, sw, n = 4000, 3000, 16
    quad = [(300.7, 120.2), (2800.4, 410.9), (2650.1, 3900.3), (90.8, 3700.6)]
    _, m_inv, dw, dh = pipeline.four_point_geometry(quad)
    q = np.asarray(quad)
    area = 0.5 * abs(float(np.dot(q[:, 0], np.roll(q[:, 1], -1)) - np.dot(q[:, 1], np.roll(q[:, 0], -1))))
    tile = synth.make_invoice(1, 1000, 750, 30)[0]
    page = torch.from_numpy(np.ascontiguousarray(np.tile(tile, (4, 4, 1)))).cuda()
    srcs = [page.clone() for _ in range(n)]
    dsts = [torch.empty((dh, dw, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
    st_tab = torch.tensor([(p.data_ptr(), sh, sw, 0) for p in srcs], dtype=torch.int64, device="cuda")
    dt_tab = torch.tensor([(p.data_ptr(), dh, dw, 0) for p in dsts], dtype=torch.int64, device="cuda")
    mats = torch.from_numpy(np.tile(m_inv.reshape(1, 9), (n, 1))).cuda()
    m = np.ascontiguousarray(m_inv.reshape(9))
    st = torch.cuda.current_stream().cuda_stream

    def one():
        _lib.check(lib.ocrvi_warp_perspective_u8(0, srcs[0].data_ptr(), sh, sw, m.ctypes.data, dsts[0].data_ptr(), dh, dw, st))

    def chunk():
        _lib.check(lib.ocrvi_warp_perspective_pages(0, st_tab.data_ptr(), dt_tab.data_ptr(), mats.data_ptr(), n, st))

    res = {"src": f"{sh}x{sw}", "dst": f"{dh}x{dw}", "bytes_written_per_page": dh * dw * 3, "source_footprint_bytes_per_page": int(area * 3),
           "hbm_peak_gbs_design": 8000}
    for name, fn, pages in (("one_page", one, 1), ("chunk_16_pages", chunk, n)):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = ms[len(ms) // 2]
        gbs = pages * (dh * dw * 3 + area * 3) / (med / 1e3) / 1e9
        res[name] = {"ms_median": round(med, 4), "ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "launches": iters,
                     "gbs_written_plus_footprint": round(gbs, 1), "share_of_8_tbs": round(gbs / 8000, 3)}
    assert torch.equal(dsts[0], dsts[n - 1])                   # the two forms wrote the same page
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=30)
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "f16x2", "bf16", "f16"])
    ap.add_argument("--sets", default="uniform,mixed,preproc")
    ap.add_argument("--binary-head", action="store_true",
                    help="run the uniform / mixed sets a second time with Engine(binary_head=True); results under 'runs_binary_head'")
    ap.add_argument("--confidence", action="store_true",
                    help="run the uniform / mixed sets a second time with Engine(confidence=True); results under 'runs_confidence'")
    ap.add_argument("--quads", action="store_true",
                    help="time the perspective warp ('warp') and run the uniform / mixed sets with a quad on every page ('runs_quads')")
    ap.add_argument("--backbone", default="resnet50", choices=["resnet50", "resnet18"], help="the detector's backbone (backbone.py:12-15)")
    ap.add_argument("--no-dcn", action="store_true", help="plain 3x3 convolutions in layers 2-4 instead of the deformable ones (dcn=False)")
    args = ap.parse_args()
    import torch
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, weights
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    assert torch.cuda.is_available(), "engine_bench needs a GPU"
    torch.cuda.set_device(0)
    sets = args.sets.split(",")
    res = {"tool": "engine_bench", "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup, "backbone": args.backbone,
           "dcn": not args.no_dcn}
    if "preproc" in sets:
        res["preproc"] = time_preproc()
    if args.quads:
        res["warp"] = time_warp()
    if "uniform" in sets or "mixed" in sets:
        det = DBNetPP(backbone=args.backbone, pretrained=False, dcn=not args.no_dcn, dtype=args.dtype,
                      state_dict=weights.make_det_state_dict(seed=1234, backbone=args.backbone, dcn=not args.no_dcn))
        rec = SVTRv2("base", state_dict=weights.make_rec_state_dict("base", seed=1234), dtype=args.dtype)
        pp = DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)
        kw = dict(rec_size=(48, 320), det_chunk=16, rec_batch=256)
        runs = []
        if "uniform" in sets:
            runs.append(run_set("uniform 960x1280", kw, [(960, 1280)] * args.pages, 1280, args, det, rec, pp))
        if "mixed" in sets:
            sizes = [MIXED[i % len(MIXED)] for i in range(args.pages)]
            runs.append(run_set("mixed " + ",".join(f"{h}x{w}" for h, w in MIXED), kw, sizes, 960, args, det, rec, pp))
        res["runs"] = runs
        if args.binary_head:   # the same sets with the binarise-branch-only detector forward (ocrvi_det_forward_binary)
            kwb = dict(kw, binary_head=True)
            runs_b = []
            if "uniform" in sets:
                runs_b.append(run_set("uniform 960x1280 binary_head", kwb, [(960, 1280)] * args.pages, 1280, args, det, rec, pp))
            if "mixed" in sets:
                runs_b.append(run_set("mixed binary_head " + ",".join(f"{h}x{w}" for h, w in MIXED), kwb, sizes, 960, args, det, rec, pp))
            res["runs_binary_head"] = runs_b
        if args.confidence:    # the same sets with per-character confidences (ocrvi_rec_forward_conf in the recogniser graph)
            kwc = dict(kw, confidence=True)
            runs_c = []
            if "uniform" in sets:
                runs_c.append(run_set("uniform 960x1280 confidence", kwc, [(960, 1280)] * args.pages, 1280, args, det, rec, pp))
            if "mixed" in sets:
                runs_c.append(run_set("mixed confidence " + ",".join(f"{h}x{w}" for h, w in MIXED), kwc, sizes, 960, args, det, rec, pp))
            res["runs_confidence"] = runs_c
        if args.quads:         # the same sets photographed: every page carries a quad and is rectified on the device first
            runs_q = []
            if "uniform" in sets:
                runs_q.append(run_set("uniform 960x1280 quads", kw, [(960, 1280)] * args.pages, 1280, args, det, rec, pp, with_quads=True))
            if "mixed" in sets:
                runs_q.append(run_set("mixed quads " + ",".join(f"{h}x{w}" for h, w in MIXED), kw, sizes, 960, args, det, rec, pp, with_quads=True))
            res["runs_quads"] = runs_q
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
