#!/usr/bin/env python3
"""Times the ASF kernels inside one detector forward (16 pages 960x1280) through the library's profiler.

    tools/asf_bench.py [--reps N] [dtype ...]        (default: 3 forwards, f16)

Per dtype one line: the `asf_fused` tag (three score launches + the blend) in us per launch and GB/s of its algorithmic traffic, and
beside it the bandwidth two streaming kernels of the same forward reach (`db_maps`, `nchw_to_nhwc4`): the roof to set the tag against.
OCRVI_LIB selects another build of the library, e.g. the parent commit's, for an A/B in alternated processes."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocr_vi_invoice_amd import DBNetPP, _lib
args = sys.argv[1:]
reps = 3
if "--reps" in args:
    i = args.index("--reps")
    reps = int(args[i + 1])
    del args[i:i + 2]
lib = _lib.load()
x = torch.randn(16, 3, 960, 1280, device="cuda")


def rate(v):
    return v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else 0.0


for dt in args or ["f16"]:
    det = DBNetPP(pretrained=False, dtype=dt)
    det(x); torch.cuda.synchronize()
    lib.ocrvi_prof_reset(); lib.ocrvi_prof_enable(1)
    for _ in range(reps): det(x)
    torch.cuda.synchronize(); lib.ocrvi_prof_enable(0)
    rep = _lib.prof_report()
    v = rep["asf_fused"]
    roof = "  ".join(f"{t} {rate(rep[t]):6.0f} GB/s" for t in ("db_maps", "nchw_to_nhwc4") if t in rep)
    print(f"{dt}: asf_fused {v['ms']/v['launches']*1e3:8.1f} us/launch {rate(v):6.0f} GB/s  ({roof})  "
          f"(det forward {sum(u['ms'] for u in rep.values())/reps:.2f} ms)", flush=True)
    del det
