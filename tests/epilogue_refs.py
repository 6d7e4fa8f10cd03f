"""Plain float64 statements of the convolution epilogues the detector's neck and head depend on (csrc/conv_gemm.h, csrc/gemm_ring.h): what
tests/test_gpu_conv_epilogues.py holds the HIP kernels to.  tests/test_epilogue_refs_cpu.py pins them to torch.nn.functional and to the head
of oracle/dbnet_cpu.py, so that they are not a third opinion.  No GPU, no library: torch only.

* conv_res_ref: act(conv(x) + b + res), the residual either of the output's shape (RES_SAME: Bottleneck conv3, BasicBlock conv2) or of half
  its resolution and read at (oh // 2, ow // 2) (RES_UP2: the FPN top-down path, neck.py:36-38);
* db_tail_ref: one branch of the DB head behind its 3x3 conv (head.py:13-16): ConvTranspose2d(64, 64, 2, 2) + folded BN + ReLU, then
  ConvTranspose2d(64, 1, 2, 2); with non-overlapping 2x2 / stride-2 kernels every output pixel has exactly one term per channel.
"""
import torch

RES_NONE, RES_SAME, RES_UP2 = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1


def conv_ref(x, w):
    """Stride-1 cross-correlation with zero padding k // 2 (nn.Conv2d, square odd kernel), tap by tap: [N, Ci, H, W] x [Co, Ci, k, k] ->
    [N, Co, H, W] in float64."""
    x, w = x.double(), w.double()
    N, Ci, H, W = x.shape
    k = w.shape[-1]
    p = k // 2
    xp = torch.zeros(N, Ci, H + 2 * p, W + 2 * p, dtype=torch.float64)
    xp[:, :, p:p + H, p:p + W] = x
    y = torch.zeros(N, w.shape[0], H, W, dtype=torch.float64)
    for r in range(k):
        for s in range(k):
            y += torch.einsum("nchw,oc->nohw", xp[:, :, r:r + H, s:s + W], w[:, :, r, s])
    return y


def up2(res, H, W):
    """Nearest 2x upsample from the definition: out[.., oh, ow] = res[.., oh // 2, ow // 2]."""
    oh = torch.arange(H) // 2
    ow = torch.arange(W) // 2
    return res[:, :, oh][:, :, :, ow]


def conv_res_ref(x, w, b, res, res_mode, act):
    """act(conv(x) + b + res) in float64.  res_mode RES_UP2: res is [N, Co, H / 2, W / 2]."""
    y = conv_ref(x, w)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if res_mode == RES_SAME:
        y = y + res.double()
    elif res_mode == RES_UP2:
        y = y + up2(res.double(), y.shape[2], y.shape[3])
    return torch.relu(y) if act == ACT_RELU else y


def up2_add(x, w, b, res, act=ACT_NONE):
    """The FPN lateral: act(conv1x1(x) + b + res[:, :, oh // 2, ow // 2])."""
    return conv_res_ref(x, w, b, res, RES_UP2, act)


def db_tail_stage1(x, w1, b1):
    """v[n, co, 2 oh + a, 2 ow + b] = relu(sum_ci x[n, ci, oh, ow] W1[ci, co, a, b] + b1[co])   (float64)"""
    x, w1, b1 = x.double(), w1.double(), b1.double()
    N, _, OH, OW = x.shape
    v = torch.einsum("nihw,ioab->nohawb", x, w1) + b1.view(1, -1, 1, 1, 1, 1)
    return torch.relu(v).reshape(N, w1.shape[1], 2 * OH, 2 * OW)


def db_tail_ref(x, w1, b1, w2, b2):
    """One branch: x [N, 64, OH, OW], W1 [64, 64, 2, 2] (c_in, c_out, a, b; BN folded), b1 [64], W2 [64, 1, 2, 2], b2 [1] -> logits
    [N, 1, 4 OH, 4 OW] in float64:
        out[n, 0, 4 oh + 2 a + a', 4 ow + 2 b + b'] = b2 + sum_co relu(sum_ci x[n, ci, oh, ow] W1[ci, co, a, b] + b1[co]) W2[co, 0, a', b']"""
    v = db_tail_stage1(x, w1, b1)
    N, _, H2, W2_ = v.shape
    y = torch.einsum("ncyx,cab->nyaxb", v, w2.double()[:, 0]) + b2.double().reshape(())
    return y.reshape(N, 1, 2 * H2, 2 * W2_)


def db_tail_partial_sum_bound(x, w1, b1, w2, b2):
    """An upper bound on |every partial sum|, in any summation order, of db_tail_ref's two dots: max over outputs of the sum of the terms'
    magnitudes.  Below 2^24 with integer operands, every partial sum is an integer float32 holds exactly."""
    a1 = torch.einsum("nihw,ioab->nohawb", x.double().abs(), w1.double().abs()) + b1.double().abs().view(1, -1, 1, 1, 1, 1)
    v = db_tail_stage1(x, w1, b1)
    a2 = torch.einsum("ncyx,cab->nyaxb", v, w2.double()[:, 0].abs()) + b2.double().abs().reshape(())
    return max(float(a1.max()), float(a2.max()))


# ---- the input families of tests/test_gpu_conv_epilogues.py (tests/test_epilogue_refs_cpu.py checks the claims made about them)
DB_TAIL_CASES = [
    # (N, OH, OW) of the 64-channel map in front of the deconvolutions; the GEMM has M = N OH OW rows in 128-row tiles
    (1, 2, 3),       # M = 6: one partial tile
    (3, 5, 9),       # M = 135: the tile boundary at row 128 falls mid-row inside image 2, then a 7-row tail
    (2, 16, 24),     # the head of a 64 x 96 page
    (2, 24, 40),     # M = 1920: 15 full tiles
]


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def db_tail_int_case(N, OH, OW, seed, groups=2):
    """Routing data: x in {0..3}, W1 in {-2..2}, b1 in {-8..8}, W2 in {-3..3}, b2 in {-5..5}, per branch.  Every operand is exact in bf16;
    relu(sum + b1) <= 64 * 6 + 8 = 392 and |b2| + the second dot <= 5 + 64 * 392 * 3 = 75269 < 2^24, so fp32 accumulation is exact in
    any order.  Returns x [N, 64 groups, OH, OW] and per branch (W1, b1, W2, b2)."""
    g = torch.Generator().manual_seed(seed)
    x = _randint(g, 0, 3, (N, 64 * groups, OH, OW))
    br = [(_randint(g, -2, 2, (64, 64, 2, 2)), _randint(g, -8, 8, (64,)), _randint(g, -3, 3, (64, 1, 2, 2)), _randint(g, -5, 5, (1,)))
          for _ in range(2)]
    return x, br


def db_tail_gauss_case(N, OH, OW, seed, groups=2):
    """Value data at the head's own scales (weights.make_det_state_dict: He-initialised deconvolutions, post-ReLU input)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, 64 * groups, OH, OW, generator=g))
    br = [(torch.randn(64, 64, 2, 2, generator=g) * (2.0 / 64) ** 0.5, torch.randn(64, generator=g) * 0.1,
           torch.randn(64, 1, 2, 2, generator=g) * (4.0 / 64) ** 0.5, torch.randn(1, generator=g) * 0.1) for _ in range(2)]
    return x, br


def up2_int_case(N, Cin, OH, OW, Co, seed):
    """Routing data for RES_UP2: x = 0, Gaussian weights, integer bias in [-20, 20], integer residual in [-100, 100] at half resolution:
    the output is bias + res[:, :, oh // 2, ow // 2], |.| <= 120, exact in every element type (bf16 holds integers up to 256)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, Cin, OH, OW)
    w = torch.randn(Co, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = _randint(g, -20, 20, (Co,))
    res = _randint(g, -100, 100, (N, Co, OH // 2, OW // 2))
    return x, w, b, res


def conv_res_gauss_case(N, Cin, H, W, Co, ksize, res_mode, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, ksize, ksize, generator=g) / (Cin * ksize * ksize) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    rs = (N, Co, H // 2, W // 2) if res_mode == RES_UP2 else (N, Co, H, W)
    res = torch.randn(*rs, generator=g)
    return x, w, b, res


def db_tail_branches_from_folded(folded):
    """The DB head's deconvolutions out of weights.fold_det's tensors, in the order ocrvi_test_db_tail takes them and det_model.hip packs
    them: branch 0 = head.bin (binarise), branch 1 = head.thr (threshold); per branch (W1, b1, W2, b2)."""
    return [tuple(torch.from_numpy(folded[f"head.{s}.{k}"].copy()) for k in ("dc1.w", "dc1.b", "dc2.w", "dc2.b")) for s in ("bin", "thr")]
