#!/usr/bin/env python3
"""Times the detector's four configurations -- ResNet-50 / ResNet-18, with / without DCN in layers 2-4 -- on one chunk of pages, and the
residual epilogue of the pipelined deformable convolution against the kernel without it.  Prints one JSON line.

Models: ``DBNetPP.forward_binary`` (what the page loop runs) on ``--n`` pages of ``--height`` x ``--width``, seeded random weights, in
the ``--dtypes`` modes.  Device events around ``--inner`` back-to-back calls on one stream, ``--warmup`` such groups first, then the median
of ``--reps`` groups divided by ``--inner``, with the groups' minimum and maximum.  The configurations are measured one after another
in one process, each with its own warm-up.

Epilogue: ``ocrvi_test_deform_conv_res`` against ``ocrvi_test_deform_conv`` at the detector's three stride-1 deformable shapes (16 pages
960 x 1280: 128 channels at 120 x 160, 256 at 60 x 80, 512 at 30 x 40), the hooks' own ``iters`` / ``avg_ms`` (events around ``--dcn-iters``
launches after one warm-up launch), the two hooks alternating ``--dcn-reps`` times, the median of each.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocr_vi_invoice_amd import DBNetPP, _lib, weights  # noqa: E402

CONFIGS = [("resnet50", True), ("resnet50", False), ("resnet18", True), ("resnet18", False)]
DCN_SHAPES = [(128, 120, 160), (256, 60, 80), (512, 30, 40)]      # (channels, H, W) of the stride-1 deformable layers, 16 pages 960 x 1280


def timed(fn, warmup, reps, inner):
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


def bench_models(args):
    x = torch.randn(args.n, 3, args.height, args.width, generator=torch.Generator().manual_seed(1)).cuda()
    out = {}
    for dt in args.dtypes.split(","):
        for backbone, dcn in CONFIGS:
            sd = weights.make_det_state_dict(seed=1234, backbone=backbone, dcn=dcn)
            m = DBNetPP(backbone=backbone, pretrained=False, dcn=dcn, state_dict=sd, dtype=dt)
            r = timed(lambda: m.forward_binary(x), args.warmup, args.reps, args.inner)
            m.check_range()
            r["pages_per_s"] = args.n / (r["ms"] * 1e-3)
            out[f"{dt} {backbone} dcn={dcn}"] = r
            del m
            torch.cuda.empty_cache()
    return out


def bench_epilogue(args):
    lib = _lib.load()
    out = {}
    for dt in args.dtypes.split(","):
        code = _lib.dtype_code(dt)
        for ch, h, w in DCN_SHAPES:
            g = torch.Generator().manual_seed(ch)
            n = args.dcn_n
            x = torch.randn(n, ch, h, w, generator=g).cuda()
            off = (torch.randn(n, 18, h, w, generator=g) * 1.5).cuda()
            mask = torch.rand(n, 9, h, w, generator=g).cuda()
            res = torch.randn(n, ch, h, w, generator=g).cuda()
            wt = np.ascontiguousarray((torch.randn(ch, ch, 3, 3, generator=g) / np.sqrt(9 * ch)).numpy())
            b = np.ascontiguousarray((torch.randn(ch, generator=g) * 0.1).numpy())
            y = torch.empty(n, ch, h, w, device="cuda")
            t = {"plain": [], "res": []}
            for _ in range(args.dcn_reps):
                ms = C.c_float(0)
                _lib.check(lib.ocrvi_test_deform_conv(0, code, x.data_ptr(), off.data_ptr(), mask.data_ptr(), wt.ctypes.data, b.ctypes.data,
                                                      n, ch, h, w, ch, 1, 1, y.data_ptr(), args.dcn_iters, C.byref(ms)))
                t["plain"].append(ms.value)
                _lib.check(lib.ocrvi_test_deform_conv_res(0, code, x.data_ptr(), off.data_ptr(), mask.data_ptr(), wt.ctypes.data, b.ctypes.data,
                                                          res.data_ptr(), n, ch, h, w, ch, 1, 1, y.data_ptr(), args.dcn_iters, C.byref(ms)))
                t["res"].append(ms.value)
            p, r = statistics.median(t["plain"]), statistics.median(t["res"])
            out[f"{dt} {n}x{ch}x{h}x{w}"] = {"plain_ms": p, "plain_min_max": [min(t["plain"]), max(t["plain"])], "res_ms": r,
                                            "res_min_max": [min(t["res"]), max(t["res"])], "res_over_plain": r / p}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--dtypes", default="f16x2,f16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--dcn-n", type=int, default=16)
    ap.add_argument("--dcn-iters", type=int, default=20)
    ap.add_argument("--dcn-reps", type=int, default=5)
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--no-epilogue", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_backbone_bench needs a GPU")
    out = {"tool": "det_backbone_bench", "shape": [args.n, 3, args.height, args.width]}
    if not args.no_models:
        out["forward_binary"] = bench_models(args)
    if not args.no_epilogue:
        out["dcn_residual_epilogue"] = bench_epilogue(args)
    out["timing"] = (f"models: device events around {args.inner} calls, median of {args.reps} groups after {args.warmup} warm-up groups; epilogue: "
                     f"the hooks' events around {args.dcn_iters} launches, median of {args.dcn_reps} alternating repeats")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
