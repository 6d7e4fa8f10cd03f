"""ResNet-50 layer1 chain at the bench's shape (16 pages: M = 1 228 800 pixels), alone on the chip: the fused launch (csrc/bneck_tail.h)
or the three launches it replaces (conv3_halo NC = 64, the ring GEMM with RES_SAME, conv_gemm 128 x 64), through the test hooks.
Device events over 20 launches, 3 repeats per process.  usage: python tools/bneck_bench.py fused|three   (OCRVI_LIB picks the library)"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from ocr_vi_invoice_amd import _lib
lib = _lib.load()
mode = sys.argv[1]
N, H, W = 16, 240, 320
M = N * H * W
g = np.random.default_rng(0)
w2 = (g.standard_normal((64, 64, 3, 3)) / np.sqrt(576)).astype(np.float32)
w3 = (g.standard_normal((256, 64, 1, 1)) / 8).astype(np.float32)
w1 = (g.standard_normal((64, 256, 1, 1)) / 16).astype(np.float32)
b2, b3, b1 = (np.zeros(n, np.float32) for n in (64, 256, 64))
t1 = torch.relu(torch.randn(N, 64, H, W, device="cuda"))
idn = torch.relu(torch.randn(N, 256, H, W, device="cuda"))
y = torch.empty(N, 256, H, W, device="cuda")
t2 = torch.empty(N, 64, H, W, device="cuda")
tn = torch.empty(N, 64, H, W, device="cuda")
ms = C.c_float(0)
MB = M * 4 * (64 + 256 + 256 + 64) / 1e6
FL = 2.0 * M * (64 * 576 + 256 * 64 + 64 * 256)
for rep in range(3):
    if mode == "fused":
        for yo in (0, 1):
            _lib.check(lib.ocrvi_test_bneck_tail(0, t1.data_ptr(), idn.data_ptr(), w2.ctypes.data, b2.ctypes.data, w3.ctypes.data, b3.ctypes.data,
                                                 w1.ctypes.data, b1.ctypes.data, N, H, W, yo, y.data_ptr(), tn.data_ptr(), 20, C.byref(ms)))
            mb = MB - (M * 4 * 64 / 1e6 if yo else 0)
            fl = FL - (2.0 * M * 64 * 256 if yo else 0)
            print(f"rep {rep} fused {'y-only' if yo else 'y+t1n'}: {ms.value * 1e3:8.1f} us  {mb / ms.value / 1e3:6.2f} TB/s over {mb:.0f} MB  "
                  f"{fl / ms.value / 1e9:6.1f} TF/s = {fl / ms.value / 1e9 / 833:.3f} of 833", flush=True)
    else:
        us = []
        _lib.check(lib.ocrvi_test_conv(0, 3, t1.data_ptr(), w2.ctypes.data, b2.ctypes.data, N, 64, H, W, 64, 3, 1, 1, 1, 1, t2.data_ptr(), 20, C.byref(ms)))
        us.append(ms.value * 1e3)
        _lib.check(lib.ocrvi_test_conv_res(0, 3, t2.data_ptr(), w3.ctypes.data, b3.ctypes.data, idn.data_ptr(), N, 64, H, W, 256, 1, 1, 1, y.data_ptr(),
                                           20, C.byref(ms)))
        us.append(ms.value * 1e3)
        _lib.check(lib.ocrvi_test_conv(0, 3, y.data_ptr(), w1.ctypes.data, b1.ctypes.data, N, 256, H, W, 64, 1, 1, 1, 1, 1, tn.data_ptr(), 20, C.byref(ms)))
        us.append(ms.value * 1e3)
        print(f"rep {rep} three launches: conv2 {us[0]:7.1f} + conv3 {us[1]:7.1f} + conv1' {us[2]:7.1f} = {sum(us):8.1f} us   (y-only chain: {us[0] + us[1]:8.1f} us)",
              flush=True)
