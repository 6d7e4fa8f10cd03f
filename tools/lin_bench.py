#!/usr/bin/env python3
"""Times the recogniser's qkv-type Linears (f16x2, T output) on the ring GEMM (ocrvi_test_gemm) and on lin_x2 (ocrvi_test_lin_x2):
20 launches by device events, three repeats per process, processes alternating ring / new / ring / new.
usage  lin_bench.py [M,K,N ...]          the parent: starts the child processes and prints the table
       lin_bench.py --one ring|new M,K,N   one process: three repeats, one line of microseconds"""
import ctypes as C, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(61440, 384, 1152), (122880, 256, 768), (61440, 384, 768)]


def one(arm, M, K, N):
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    from ocr_vi_invoice_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(1)
    a = torch.randn(M, K, generator=g).cuda()
    w = np.ascontiguousarray((torch.randn(N, K, generator=g) / K ** 0.5).numpy())
    b = np.ascontiguousarray(torch.randn(N, generator=g).numpy())
    out = torch.empty(M, N, device="cuda")
    us = []
    for _ in range(3):
        ms = C.c_float(0)
        if arm == "ring":
            L.check(lib.ocrvi_test_gemm(0, 3, a.data_ptr(), w.ctypes.data, b.ctypes.data, None, M, K, N, 0, 0, 0, out.data_ptr(), 20, C.byref(ms)))
        else:
            L.check(lib.ocrvi_test_lin_x2(0, a.data_ptr(), w.ctypes.data, b.ctypes.data, M, K, N, 0, None, out.data_ptr(), 20, C.byref(ms)))
        us.append(ms.value * 1e3)
    print("US " + " ".join(f"{v:.2f}" for v in us), flush=True)


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in sys.argv[1:]] or SHAPES
    print("| M | K | N | arm | us per repeat (two processes x three) | fastest | slowest | TFLOP/s (of 833) | GB/s (A + W + out) | routed |\n|---|---|---|---|---|---|---|---|---|---|")
    for M, K, N in shapes:
        runs = {"ring": [], "new": []}
        for arm in ("ring", "new", "ring", "new"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arm, f"{M},{K},{N}"], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(r.stderr[-2000:])
                sys.exit(r.returncode)      # (nothing more is started after a failed process)
            runs[arm] += [float(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("US ")][-1].split()[1:]]
        fl, by = 2.0 * M * K * N, 4.0 * (M * K + N * K + M * N)
        wins = max(runs["new"]) < min(runs["ring"])
        for arm in ("ring", "new"):
            v = runs[arm]
            med = sorted(v)[len(v) // 2]
            print(f"| {M} | {K} | {N} | {arm} | {' '.join(f'{x:.1f}' for x in v)} | {min(v):.1f} | {max(v):.1f} | {fl / med / 1e6:.0f} ({fl / med / 1e6 / 833 * 100:.0f} %) | "
                  f"{by / med / 1e3:.0f} | {('yes' if wins else 'no') if arm == 'new' else ''} |", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], *[int(v) for v in sys.argv[3].split(",")])
    else:
        main()
