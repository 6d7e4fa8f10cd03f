#!/usr/bin/env python3
"""Times the JPEG decoder (include/ocrvi.h, "JPEG decode") on ``--pages`` synthetic 960 x 1280 invoices at quality 85, in 4:2:0 and 4:4:4.
Prints one JSON line.

Per kernel: the library's per-launch profiler brackets ``jpeg_idct_kernel`` and ``jpeg_rgb_kernel`` with device events; ``--warmup``
batched launches first, then the median, minimum and maximum of ``--reps``.  ``bytes`` is what each kernel must move (idct: records,
offsets and tables read, planes written; rgb: planes read, RGB written) and ``hbm_share`` that figure over the time as a share of
8 TB/s.  Host: ``ocrvi_jpeg_parse`` per page on one core and on the pool; PIL's full decode of the same files beside it where PIL is
importable (``null`` otherwise).  PCIe: coefficient-stream bytes against 3 H W.  End to end: ``Engine.run`` on ``--engine-pages`` pages as
JPEG bytes against the same pages as pre-decoded device arrays (no decode at all: the upper bound), the two settings alternating run by
run, median and spread of each.
The files are encoded with PIL (an encoder independent of the library's own); ``--dir`` takes a folder of baseline .jpg files instead.  Needs a GPU: there
is no fallback."""
import argparse
import concurrent.futures
import glob
import io
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

HBM_BYTES_PER_S = 8e12
H, W = 960, 1280


def encode_pages(n, subsampling):
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit("jpeg_bench encodes its pages with PIL, which is not importable here: "
                         "pass --dir with a folder of baseline .jpg files instead") from None
    out = []
    for i in range(n):
        img = synth.make_invoice(100 + i, H, W, lines=30)[0]
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=85, subsampling=subsampling)
        out.append(buf.getvalue())
    return out


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def bench_kernels(lib, files, args):
    infos = [pipeline.jpeg_info_struct(f) for f in files]
    n = len(files)
    s_off, w_off, d_off = [0], [0], [0]
    for info in infos:
        s_off.append(s_off[-1] + (info.stream_bytes + 255) // 256 * 256)
        w_off.append(w_off[-1] + info.workspace_bytes)
        d_off.append(d_off[-1] + (info.out_height * info.out_width * 3 + 255) // 256 * 256)
    h_rec = torch.empty(s_off[-1], dtype=torch.uint8).pin_memory()
    used = [pipeline.jpeg_parse_into(f, h_rec.data_ptr() + s_off[i], infos[i].stream_bytes) for i, f in enumerate(files)]
    table = np.zeros((n, _lib.JPEG_ENTRY), np.int64)
    for i, info in enumerate(infos):
        pipeline.jpeg_table_entry(info, used[i], s_off[i], d_off[i], 3 * info.out_width, w_off[i], table[i])
    d_rec = h_rec.cuda()
    d_tab = torch.from_numpy(table).cuda()
    ws = torch.empty(w_off[-1], dtype=torch.uint8, device="cuda")
    out = torch.empty(d_off[-1], dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.ocrvi_jpeg_decode_pages(0, d_rec.data_ptr(), d_tab.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), st))

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    t = {"jpeg_idct": [], "jpeg_rgb": []}
    lib.ocrvi_prof_enable(1)
    for _ in range(args.reps):
        lib.ocrvi_prof_reset()
        launch()
        torch.cuda.synchronize()
        rep = _lib.prof_report()
        for k in t:
            t[k].append(rep[k]["ms"])
    lib.ocrvi_prof_enable(0)
    lib.ocrvi_prof_reset()
    planes = sum(int(i.workspace_bytes) for i in infos)
    rgb = sum(3 * i.out_height * i.out_width for i in infos)
    streams = sum(used)
    bytes_idct = streams + n * _lib.JPEG_ENTRY * 8 + planes
    bytes_rgb = planes + rgb
    res = {"pages": n, "stream_bytes": streams, "plane_bytes": planes, "rgb_bytes": rgb, "file_bytes": sum(len(f) for f in files)}
    for k, b in (("jpeg_idct", bytes_idct), ("jpeg_rgb", bytes_rgb)):
        res[k] = spread(t[k])
        res[k]["bytes"] = b
        res[k]["hbm_share"] = b / (res[k]["ms"] * 1e-3) / HBM_BYTES_PER_S
    res["pcie_bytes_per_page"] = {"stream": streams / n, "raw_rgb": rgb / n, "ratio": streams / rgb}
    return res


def bench_host(files, args):
    infos = [pipeline.jpeg_info_struct(f) for f in files]
    bufs = [np.empty(i.stream_bytes // 4, np.uint32) for i in infos]
    jobs = [(f, b.ctypes.data, b.nbytes) for f, b in zip(files, bufs)]
    one, pool_t = [], []
    threads = min(len(os.sched_getaffinity(0)), 16)
    pool = concurrent.futures.ThreadPoolExecutor(threads)
    for r in range(args.host_reps + 1):
        t0 = time.perf_counter()
        for j in jobs:
            pipeline.jpeg_parse_into(*j)
        t1 = time.perf_counter()
        list(pool.map(lambda j: pipeline.jpeg_parse_into(*j), jobs))
        t2 = time.perf_counter()
        if r:
            one.append((t1 - t0) * 1e3 / len(files))
            pool_t.append((t2 - t1) * 1e3 / len(files))
    res = {"parse_ms_per_page_one_core": spread(one), "parse_ms_per_page_pool": spread(pool_t), "pool_threads": threads,
           "pil_decode_ms_per_page": None}
    try:
        from PIL import Image
    except ImportError:
        return res
    pil = []
    for r in range(args.host_reps + 1):
        t0 = time.perf_counter()
        for f in files:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        if r:
            pil.append((time.perf_counter() - t0) * 1e3 / len(files))
    res["pil_decode_ms_per_page"] = spread(pil)
    return res


def bench_engine(files, args):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    eng = Engine(det, rec, DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6), det_size=960, det_chunk=16)
    files = [files[i % len(files)] for i in range(args.engine_pages)]
    arrays = pipeline.imdecode(files)
    host_arrays = [a.cpu().numpy() for a in arrays]
    t = {"jpeg": [], "device_arrays": [], "host_arrays": []}
    parse = []
    for r in range(args.engine_warmup + args.engine_reps):
        for name, pages in (("jpeg", files), ("device_arrays", arrays), ("host_arrays", host_arrays)):
            t0 = time.perf_counter()
            eng.run(pages)
            if r >= args.engine_warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
                if name == "jpeg":
                    parse.append(eng.stats["jpeg_parse_s"] * 1e3)
    res = {"pages": len(files), "det_size": 960, "det_chunk": 16, "dtype": "f16x2", "crops": eng.stats["crops"]}
    for k, v in t.items():
        res["run_" + k] = spread(v)
    res["jpeg_parse_ms_in_run"] = spread(parse)
    res["jpeg_minus_device_arrays_ms_per_page"] = (res["run_jpeg"]["ms"] - res["run_device_arrays"]["ms"]) / len(files)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--engine-pages", type=int, default=64)
    ap.add_argument("--engine-warmup", type=int, default=2)
    ap.add_argument("--engine-reps", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--dir", default=None, help="a folder of baseline .jpg files to time instead of the synthetic pages")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a GPU")
    lib = _lib.load()
    if args.dir:
        sets = {"dir": [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.dir, "*.jpg")))[:args.pages]]}
    else:
        sets = {"420": encode_pages(args.pages, 2), "444": encode_pages(args.pages, 0)}
    out = {"page": [H, W], "quality": 85}
    for name, files in sets.items():
        out[name] = bench_kernels(lib, files, args)
        out[name]["host"] = bench_host(files, args)
    if not args.no_engine:
        out["engine"] = bench_engine(next(iter(sets.values())), args)
    out["timing"] = (f"kernels: device events of the library profiler around each launch, median of {args.reps} after {args.warmup}; host: wall "
                     f"clock, median of {args.host_reps} passes after one; engine: host clock around run(), median of {args.engine_reps} after "
                     f"{args.engine_warmup}, settings alternating run by run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
