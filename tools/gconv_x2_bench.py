#!/usr/bin/env python3
"""Times LocalMixing's grouped 3x3 convolutions in f16x2 through ocrvi_test_gconv_x2 on conv_gemm (OCRVI_GCONV32=0 in the process'
environment) and on gconv_x2: both epilogues (conv1: GELU -> f16x2; conv2: GELU + fp32 residual -> fp32), 20 launches by device events,
three repeats per process, processes alternating old / new / old / new.
usage  gconv_x2_bench.py [n,C,H,W ...]             the parent: starts the child processes and prints the table
       gconv_x2_bench.py --one conv1|conv2 n,C,H,W   one process (the arm is its OCRVI_GCONV32): three repeats, one line of microseconds"""
import ctypes as C, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 128, 12, 80), (256, 256, 6, 80)]
HBM = 5.5e12          # what the streaming kernels reach on the MI355X: the floor the table's last column is a fraction of


def one(epi, n, Cc, H, W):
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    from ocr_vi_invoice_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, Cc, H, W, generator=g).cuda()
    w = np.ascontiguousarray((torch.randn(Cc, 32, 3, 3, generator=g) / 288 ** 0.5).numpy())
    b = np.ascontiguousarray(torch.randn(Cc, generator=g).numpy())
    res = torch.randn(n, Cc, H, W, generator=g).cuda() if epi == "conv2" else None
    raw = torch.empty(n * H * W * Cc, device="cuda")
    out = torch.empty(n, Cc, H, W, device="cuda")
    us = []
    for _ in range(3):
        ms = C.c_float(0)
        L.check(lib.ocrvi_test_gconv_x2(0, x.data_ptr(), w.ctypes.data, b.ctypes.data, None if res is None else res.data_ptr(), n, Cc, H, W, 2,
                                        int(epi == "conv2"), int(epi == "conv2"), 0, 0, raw.data_ptr(), out.data_ptr(), 20, C.byref(ms)))
        us.append(ms.value * 1e3)
    print("US " + " ".join(f"{v:.2f}" for v in us), flush=True)


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in sys.argv[1:]] or SHAPES
    print("| n,C,H,W | epilogue | arm | us per repeat (two processes x three) | fastest | slowest | GB/s (algorithmic) | floor us at 5.5 TB/s | floor / median | routed |\n"
          "|---|---|---|---|---|---|---|---|---|---|")
    for n, Cc, H, W in shapes:
        for epi in ("conv1", "conv2"):
            runs = {"old": [], "new": []}
            for arm in ("old", "new", "old", "new"):
                env = dict(os.environ)
                env.pop("OCRVI_GCONV32", None)
                if arm == "old":
                    env["OCRVI_GCONV32"] = "0"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", epi, f"{n},{Cc},{H},{W}"], capture_output=True, text=True,
                                   timeout=300, env=env)
                if r.returncode != 0:
                    print(r.stderr[-2000:])
                    sys.exit(r.returncode)      # (nothing more is started after a failed process)
                runs[arm] += [float(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("US ")][-1].split()[1:]]
            px = n * H * W * Cc
            by = 4.0 * px * (3 if epi == "conv2" else 2) + 4.0 * Cc * 288
            floor = by / HBM * 1e6
            wins = max(runs["new"]) < min(runs["old"])
            for arm in ("old", "new"):
                v = runs[arm]
                med = sorted(v)[len(v) // 2]
                print(f"| {n},{Cc},{H},{W} | {epi} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {min(v):.1f} | {max(v):.1f} | {by / med / 1e3:.0f} | {floor:.1f} | "
                      f"{floor / med:.2f} | {('yes' if wins else 'no') if arm == 'new' else ''} |", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], *[int(v) for v in sys.argv[3].split(",")])
    else:
        main()
