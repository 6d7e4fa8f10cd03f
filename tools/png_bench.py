#!/usr/bin/env python3
"""Times the PNG decoder (include/ocrvi.h, "PNG decode") on ``--pages`` synthetic 960 x 1280 invoices written as RGB8, grey8, 8-bit palette
and bilevel files.  Prints one JSON line.

Kernel: the library's per-launch profiler brackets ``png_unfilter_kernel`` with device events; ``--warmup`` batched launches first, then
the median, minimum and maximum of ``--reps``.  Host: ``ocrvi_png_parse`` (CRC, inflate, Adler-32) per page on one core and on 16
threads; PIL's whole decode of the same files on one core beside it where PIL is importable (``null`` otherwise).  PCIe: stream bytes
against 3 H W.  End to end: ``Engine.run`` on ``--engine-pages`` pages as PNG bytes against the same pages as pre-decoded device arrays
(no decode at all) and as host arrays (3 H W over the bus), the three settings alternating run by run, median and spread of each, for
each kind of file.
The files are written here (zlib level 6, every row Paeth-filtered: the filter that costs the device most); ``--dir`` takes a folder of
.png files instead.  Needs a GPU: there is no fallback."""
import argparse
import concurrent.futures
import glob
import io
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocr_vi_invoice_amd import _lib, pipeline, synth  # noqa: E402

H, W = 960, 1280


def chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)


def write_png(rows, bpp, colour, depth, width, palette=None):
    """rows: uint8 [H, row_bytes], unfiltered -> a PNG file, every row Paeth-filtered (the forward filter reads original bytes only)."""
    h, n = rows.shape
    r = np.zeros((h + 1, n + bpp), np.int16)
    r[1:, bpp:] = rows
    x, a, b, c = r[1:, bpp:], r[1:, :n], r[:-1, bpp:], r[:-1, :n]
    q = a + b - c
    pa, pb, pc = np.abs(q - a), np.abs(q - b), np.abs(q - c)
    p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((h, 1 + n), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = (x - p) & 255
    plte = chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()) if palette is not None else b""
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, h, depth, colour, 0, 0, 0)) + plte
            + chunk(b"IDAT", zlib.compress(out.tobytes(), 6)) + chunk(b"IEND"))


def make_pages(n, kind):
    out = []
    for i in range(n):
        img = synth.make_invoice(100 + i, H, W, lines=30)[0]
        if kind == "rgb8":
            out.append(write_png(img.reshape(H, 3 * W), 3, 2, 8, W))
        elif kind == "grey8":
            out.append(write_png(img[:, :, 0], 1, 0, 8, W))
        elif kind == "palette8":
            levels = np.arange(16, dtype=np.uint8) * 17
            out.append(write_png(img[:, :, 0] // 16, 1, 3, 8, W, np.stack([levels] * 3, axis=1)))
        else:
            out.append(write_png(np.packbits(img[:, :, 0] > 128, axis=1), 1, 0, 1, W))
    return out


def spread(v):
    return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}


def bench_kernel(lib, files, args):
    infos = [pipeline.png_info_struct(f) for f in files]
    n = len(files)
    s_off, w_off, d_off = [0], [0], [0]
    for info in infos:
        s_off.append(s_off[-1] + (info.stream_bytes + 255) // 256 * 256)
        w_off.append(w_off[-1] + info.workspace_bytes)
        d_off.append(d_off[-1] + (info.out_height * info.out_width * 3 + 255) // 256 * 256)
    h_rec = torch.empty(s_off[-1], dtype=torch.uint8).pin_memory()
    used = [pipeline.png_parse_into(f, h_rec.data_ptr() + s_off[i], infos[i].stream_bytes) for i, f in enumerate(files)]
    table = np.zeros((n, _lib.PNG_ENTRY), np.int64)
    for i, info in enumerate(infos):
        pipeline.png_table_entry(info, used[i], s_off[i], d_off[i], 3 * info.out_width, w_off[i], table[i])
    d_rec = h_rec.cuda()
    d_tab = torch.from_numpy(table).cuda()
    ws = torch.empty(max(w_off[-1], 256), dtype=torch.uint8, device="cuda")
    out = torch.empty(d_off[-1], dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.ocrvi_png_decode_pages(0, d_rec.data_ptr(), d_tab.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), st))

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    t = []
    lib.ocrvi_prof_enable(1)
    for _ in range(args.reps):
        lib.ocrvi_prof_reset()
        launch()
        torch.cuda.synchronize()
        t.append(_lib.prof_report()["png_unfilter"]["ms"])
    lib.ocrvi_prof_enable(0)
    lib.ocrvi_prof_reset()
    rgb = sum(3 * i.out_height * i.out_width for i in infos)
    streams = sum(used)
    plans = [pipeline.png_plan(i) for i in infos]
    res = {"pages": n, "stream_bytes": streams, "rgb_bytes": rgb, "file_bytes": sum(len(f) for f in files), "steps_per_page": plans[0]["steps"],
           "bands_per_page": plans[0]["bands"], "png_unfilter": spread(t)}
    res["png_unfilter"]["ms_per_page"] = res["png_unfilter"]["ms"] / n
    res["pcie_bytes_per_page"] = {"stream": streams / n, "raw_rgb": rgb / n, "ratio": streams / rgb}
    return res


def bench_host(files, args):
    infos = [pipeline.png_info_struct(f) for f in files]
    bufs = [np.empty(i.stream_bytes, np.uint8) for i in infos]
    jobs = [(f, b.ctypes.data, b.nbytes) for f, b in zip(files, bufs)]
    one, pool_t = [], []
    pool = concurrent.futures.ThreadPoolExecutor(16)
    for r in range(args.host_reps + 1):
        t0 = time.perf_counter()
        for j in jobs:
            pipeline.png_parse_into(*j)
        t1 = time.perf_counter()
        list(pool.map(lambda j: pipeline.png_parse_into(*j), jobs))
        t2 = time.perf_counter()
        if r:
            one.append((t1 - t0) * 1e3 / len(files))
            pool_t.append((t2 - t1) * 1e3 / len(files))
    res = {"parse_ms_per_page_one_core": spread(one), "parse_ms_per_page_16_threads": spread(pool_t), "pil_decode_ms_per_page": None}
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


def bench_engine(sets, args):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    eng = Engine(det, rec, DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6), det_size=960, det_chunk=16)
    res = {"pages": args.engine_pages, "det_size": 960, "det_chunk": 16, "dtype": "f16x2"}
    for kind, files in sets.items():
        files = [files[i % len(files)] for i in range(args.engine_pages)]
        arrays = pipeline.imdecode(files)
        host_arrays = [a.cpu().numpy() for a in arrays]
        t = {"png": [], "device_arrays": [], "host_arrays": []}
        parse = []
        for r in range(args.engine_warmup + args.engine_reps):
            for name, pages in (("png", files), ("device_arrays", arrays), ("host_arrays", host_arrays)):
                t0 = time.perf_counter()
                eng.run(pages)
                if r >= args.engine_warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
                    if name == "png":
                        parse.append(eng.stats["png_parse_s"] * 1e3)
        one = {"run_" + k: spread(v) for k, v in t.items()}
        one["png_parse_ms_in_run"] = spread(parse)
        one["png_minus_device_arrays_ms_per_page"] = (one["run_png"]["ms"] - one["run_device_arrays"]["ms"]) / len(files)
        one["png_minus_host_arrays_ms_per_page"] = (one["run_png"]["ms"] - one["run_host_arrays"]["ms"]) / len(files)
        res[kind] = one
        del arrays, host_arrays
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--engine-pages", type=int, default=64)
    ap.add_argument("--engine-warmup", type=int, default=1)
    ap.add_argument("--engine-reps", type=int, default=3)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--dir", default=None, help="a folder of .png files to time instead of the synthetic pages")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a GPU")
    lib = _lib.load()
    if args.dir:
        sets = {"dir": [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(args.dir, "*.png")))[:args.pages]]}
    else:
        sets = {k: make_pages(args.pages, k) for k in ("rgb8", "grey8", "palette8", "bilevel")}
    out = {"page": [H, W], "filter": "Paeth on every row", "zlib_level": 6}
    for name, files in sets.items():
        out[name] = bench_kernel(lib, files, args)
        out[name]["host"] = bench_host(files, args)
    if not args.no_engine:
        out["engine"] = bench_engine(sets, args)
    out["timing"] = (f"kernel: device events of the library profiler around each launch, median of {args.reps} after {args.warmup}; host: wall "
                     f"clock, median of {args.host_reps} passes after one; engine: host clock around run(), median of {args.engine_reps} after "
                     f"{args.engine_warmup}, settings alternating run by run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
