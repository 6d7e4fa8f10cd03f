"""The direct halo-tile 3x3 convolution of the f16x2 mode (csrc/conv3_halo.h): dense 3x3 / stride 1 / pad 1 layers with 64, 128 or 256
output channels.  Checked against a float64 torch reference, for batch invariance (a page alone and inside a batch give the same bits),
and against the implicit GEMM it replaces (OCRVI_CONV3_HALO=0, read once per process: a fresh child process per setting)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import TOL, run_conv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HALO_CASES = [
    # N, Cin, H, W, Co, act -- the detector's dense 3x3 layers at reduced map sizes, then ragged and small cases
    (2, 256, 48, 64, 256, 1),    # neck.fpn[0] (240x320 map at 16 pages)
    (2, 256, 40, 48, 128, 1),    # head_conv, both branches (256 -> 128)
    (2, 256, 24, 32, 256, 1),    # neck.fpn[1]
    (3, 256, 12, 16, 256, 1),    # neck.fpn[2]
    (3, 256, 6, 8, 256, 1),      # neck.fpn[3]: smaller than one tile
    (2, 64, 48, 64, 64, 1),      # layer1 conv2 (64 -> 64)
    (1, 64, 37, 45, 256, 0),     # ragged: H, W not multiples of 16; no activation
    (2, 256, 19, 33, 128, 0),
    (3, 64, 17, 23, 64, 0),
    (1, 128, 5, 70, 256, 1),     # one tile row, a ragged last column tile
    (2, 96, 21, 18, 120, 1),     # Cin = 3 channel blocks, N_g 120 of 128 columns
]


def _ref(x, w, b, act):
    r = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    return F.relu(r) if act == 1 else r


def _case_tensors(case):
    N, Cin, H, W, Co, act = case
    g = torch.Generator().manual_seed(sum(case) * 7 + 1)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / np.sqrt(9 * Cin)
    b = torch.randn(Co, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("case", HALO_CASES)
def test_conv3_halo_matches_float64(case):
    x, w, b, act = *_case_tensors(case), case[5]
    out = run_conv(x, w, b, 3, 1, 1, 1, act, "f16x2")
    ref = _ref(x, w, b, act)
    err = float((out.double() - ref).abs().max() / (ref.pow(2).mean().sqrt() + 1e-12))
    assert err < TOL["f16x2"], err
    # every border row and column of every image (where the patch's zero halo is read)
    H, W = x.shape[2:]
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    e2 = float((out[:, :, edge].double() - ref[:, :, edge]).abs().max() / (ref.pow(2).mean().sqrt() + 1e-12))
    assert e2 < TOL["f16x2"], e2
    assert torch.equal(out, run_conv(x, w, b, 3, 1, 1, 1, act, "f16x2"))   # no race: a second launch gives the same bits


@pytest.mark.parametrize("case", [(3, 256, 40, 56, 256, 1), (3, 64, 33, 47, 64, 0), (3, 256, 20, 24, 128, 1)])
def test_conv3_halo_batch_invariant(case):
    """n_img = 3 gives the same bits as three single-image calls (neither the kernel nor the K order depends on n_img or M)."""
    x, w, b, act = *_case_tensors(case), case[5]
    whole = run_conv(x, w, b, 3, 1, 1, 1, act, "f16x2")
    for i in range(x.shape[0]):
        assert torch.equal(whole[i:i + 1], run_conv(x[i:i + 1], w, b, 3, 1, 1, 1, act, "f16x2")), i


_CHILD = r"""
import sys, torch, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_kernels import run_conv
d = torch.load(sys.argv[2])
out = run_conv(d["x"], d["w"], d["b"], 3, 1, 1, 1, d["act"], "f16x2")
torch.save(out, sys.argv[3])
"""


@pytest.mark.parametrize("case", [(2, 256, 37, 45, 256, 1), (2, 64, 24, 40, 64, 1), (1, 256, 30, 20, 128, 0)])
def test_conv3_halo_agrees_with_conv_gemm(case, tmp_path):
    """The halo kernel and OCRVI_CONV3_HALO=0 (conv_gemm, K order (tap, channel)) agree within the f16x2 tolerance."""
    x, w, b, act = *_case_tensors(case), case[5]
    inp = tmp_path / "in.pt"
    torch.save({"x": x, "w": w, "b": b, "act": act}, inp)
    outs = {}
    for flag in ("1", "0"):
        env = dict(os.environ, OCRVI_CONV3_HALO=flag)
        dst = tmp_path / f"out{flag}.pt"
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(inp), str(dst)], env=env, check=True, timeout=600)
        outs[flag] = torch.load(dst)
    ref = _ref(x, w, b, act)
    scale = float(ref.pow(2).mean().sqrt())
    assert float((outs["1"] - outs["0"]).abs().max()) / scale < TOL["f16x2"]
