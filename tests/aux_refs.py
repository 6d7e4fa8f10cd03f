"""Plain float64 statements of the memory-bound operations of csrc/kernels.hip: what tests/test_gpu_aux_kernels.py holds the HIP kernels
to, one short function each.  tests/test_aux_refs_cpu.py pins them to torch.nn.functional, to the oracle and to a reference-generated
golden, so that they are not a third opinion.  No GPU, no library: torch and numpy only."""
import numpy as np
import torch
import torch.nn.functional as F


def f16x2_round(x: torch.Tensor) -> torch.Tensor:
    """The value an f16x2 element holds for the fp32 value x: hi = fp16(x), lo = fp16(x - hi), hi + lo in float32 (include/ocrvi.h)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.float() + lo.float()


def round_to(x: torch.Tensor, dt: str) -> torch.Tensor:
    """x rounded to something the element type `dt` holds exactly (float32 result)."""
    if dt == "bf16":
        return x.to(torch.bfloat16).float()
    if dt == "f16":
        return x.half().float()
    if dt == "f16x2":
        return f16x2_round(x)
    return x.float()


def layernorm_ref(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the last dim (svtrv2.py:93,95,446): two-pass mean / biased variance.  Returns (y, sigma) in float64."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double(), var.sqrt().squeeze(-1)


def log_softmax_ref(x):
    """log_softmax over the last dim in float64.  A row holding NaN or +inf, or nothing but -inf, is NaN throughout (as torch's is)."""
    x = x.double()
    mx = x.max(-1, keepdim=True).values
    return (x - mx) - torch.log(torch.exp(x - mx).sum(-1, keepdim=True))


def maxpool_ref(x):
    """MaxPool2d(3, stride 2, padding 1) (backbone.py:34): the padding never wins, i.e. it is -inf."""
    N, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(x.double(), (1, 2, 1, 2), value=float("-inf"))
    taps = [p[:, :, r:r + 2 * OH:2, q:q + 2 * OW:2] for r in range(3) for q in range(3)]
    return torch.stack(taps).max(0).values


def frm_vertical_ref(kv, vq, B, H, W, D):
    """FRM vertical cross-attention with the precomputed query (svtrv2.py:236-243): kv [B*H*W][2D] (token = h*W + w; k | v), vq [D],
    heads of 32 -> out [B*W][D] in float64: softmax over the H keys of a column of q.k / sqrt(32), times v."""
    h = D // 32
    kv = kv.double().reshape(B, H, W, 2, h, 32)
    s = (kv[:, :, :, 0] * vq.double().reshape(h, 32)).sum(-1) * 32 ** -0.5      # [B, H, W, h]
    p = torch.softmax(s, 1)
    return (p.unsqueeze(-1) * kv[:, :, :, 1]).sum(1).reshape(B * W, D)


def _taps_align_corners(n_in, n_out):
    """Tap indices and the weight of the second tap of F.interpolate(mode="bilinear", align_corners=True) along one axis.  The source
    coordinate is float32((in - 1) / (out - 1)) * dst in float32, as ATen's fp32 kernel (and asf_blend_kernel) computes it; the rest is exact."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = src.astype(np.float64) - i0
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam)


def bilinear_up_ref(p, H, W):
    """F.interpolate(p, (H, W), mode="bilinear", align_corners=True) in float64 with the fp32 tap coordinates (neck.py:65)."""
    p = p.double()
    y0, y1, ly = _taps_align_corners(p.shape[2], H)
    x0, x1, lx = _taps_align_corners(p.shape[3], W)
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)
    rows = p[:, :, y0] * (1 - ly) + p[:, :, y1] * ly
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def asf_ref(p2, p3, p4, p5, w, b):
    """ScaleFeatureSelection.forward, the literal form of neck.py:57-79: upsample p3..p5 to p2's size, concatenate, 1x1 conv (w [4][1024],
    b [4]), softmax over the 4 scores, weighted sum.  Returns (fused, attention [N,4,H,W]) in float64."""
    H, W = p2.shape[-2:]
    ups = [p2.double()] + [bilinear_up_ref(p, H, W) for p in (p3, p4, p5)]
    score = torch.einsum("oc,nchw->nohw", w.double().reshape(4, 1024), torch.cat(ups, 1)) + b.double().view(1, 4, 1, 1)
    att = torch.softmax(score, 1)
    return sum(u * att[:, i:i + 1] for i, u in enumerate(ups)), att


def db_maps_ref(bin_logits, thresh_logits):
    """binary, thresh = sigmoid of the two logit maps (head.py:34,38) in float64."""
    return torch.sigmoid(bin_logits.double()), torch.sigmoid(thresh_logits.double())


def db_step_ref(binary, thresh, k):
    """The DB step function 1 / (1 + exp(-k (binary - thresh))) (head.py:28-30) in float64."""
    return torch.reciprocal(1 + torch.exp(-float(k) * (binary.double() - thresh.double())))


def ctc_collapse_ref(argmax_ids, blank=0):
    """Greedy CTC path of argmax ids [B][T] (svtrv2.py:559-566): collapse repeats, drop the blank -> (ids [B][T] padded with -1, lens [B])."""
    a = np.asarray(argmax_ids)
    ids = np.full(a.shape, -1, np.int32)
    lens = np.zeros(a.shape[0], np.int32)
    for b, row in enumerate(a):
        keep = [int(c) for t, c in enumerate(row) if c != blank and (t == 0 or c != row[t - 1])]
        ids[b, :len(keep)] = keep
        lens[b] = len(keep)
    return ids, lens
