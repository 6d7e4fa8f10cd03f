"""REFERENCE for the detector's other backbone configurations (test infrastructure only -- never imported by the product path).

The oracle (oracle/dbnet_cpu.py) restates the reference's DBNet++ forward for ResNet-50 and already runs it without DCN
(``backbone(sd, x, dcn=False)``).  This file adds the ResNet-18 the reference's constructor also offers
(model/det/backbone.py:12-15), in the same plain functional torch fp32 on a reference-schema ``state_dict``:

* ``basic_block``: ``torchvision.models.resnet.BasicBlock`` -- conv1 3x3 (carries the stride) + BN + ReLU, conv2 3x3 stride 1 + BN,
  add the identity (``downsample`` = 1x1 strided conv + BN where the shape changes), ReLU.
* with ``dcn`` the reference replaces ``conv2`` of EVERY block of layers 2-4 by its DeformableConv2d (backbone.py:39-53: the loop
  does not look at the block type), so a BasicBlock's deformable conv runs at stride 1 on conv1's output; ``conv1`` is never
  deformable.

Parity is UNPINNED, like the oracle's Bottleneck: the reference delegates the blocks to torchvision, which is not importable here,
so nothing in this file is checked against a reference-run output.  It is self-checked instead (tests/test_backbones_cpu.py): with
the reference's own DCN initialisation (offset / mask conv all zero, dcn.py:28-29: offsets 0, mask sigmoid(0) = 0.5) the DCN backbone
equals the plain one on the same weights with every layer-2..4 ``conv2.weight`` halved.  ``_bn``, ``dcn_module``, ``neck`` and ``head``
are the oracle's, imported unchanged.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F

from oracle.dbnet_cpu import _bn, dcn_module, head, neck

R18_BLOCKS = [2, 2, 2, 2]


def basic_block(sd, p, x, stride, has_down, dcn):
    idn = x
    y = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"], None, stride, 1)))
    if dcn:
        y = dcn_module(sd, p + ".conv2", y, 1)
    else:
        y = F.conv2d(y, sd[p + ".conv2.weight"], None, 1, 1)
    y = _bn(sd, p + ".bn2", y)
    if has_down:
        idn = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride))
    return F.relu(y + idn)


def backbone18(sd, x, dcn=True) -> List[torch.Tensor]:
    """ResNet.forward (backbone.py:55-60) on torchvision's resnet18 -> [c2, c3, c4, c5] with 64 / 128 / 256 / 512 channels."""
    bb = "backbone.model."
    y = F.relu(_bn(sd, bb + "bn1", F.conv2d(x, sd[bb + "conv1.weight"], None, 2, 3)))
    y = F.max_pool2d(y, 3, 2, 1)
    feats = []
    for li, nblk in enumerate(R18_BLOCKS, start=1):
        for b in range(nblk):
            first = b == 0 and li > 1
            y = basic_block(sd, f"{bb}layer{li}.{b}", y, 2 if first else 1, first, dcn and li >= 2)
        feats.append(y)
    return feats


@torch.no_grad()
def forward18(sd, x, dcn=True, return_feats=False):
    """DBNetPP(backbone='resnet18', dcn=dcn).forward (dbnet.py:13-17): (N,3,H,W) fp32, H,W % 32 == 0 -> the five (N,1,H,W) maps."""
    feats = backbone18(sd, x.float(), dcn)
    fused = neck(sd, feats)
    out = head(sd, fused)
    if return_feats:
        out = dict(out, c2=feats[0], c3=feats[1], c4=feats[2], c5=feats[3], fused=fused)
    return out


@torch.no_grad()
def forward50(sd, x, dcn=True, return_feats=False):
    """The oracle's forward with the DCN choice exposed (its own ``forward`` fixes dcn=True)."""
    from oracle.dbnet_cpu import backbone
    feats = backbone(sd, x.float(), dcn)
    fused = neck(sd, feats)
    out = head(sd, fused)
    if return_feats:
        out = dict(out, c2=feats[0], c3=feats[1], c4=feats[2], c5=feats[3], fused=fused)
    return out


def as_reference_checkpoint(sd):
    """`sd` as a trainer of the reference saves it: the backbone under the aliases backbone.layerN.* only (layer1 = Sequential(conv1, bn1,
    relu, maxpool, layer1), so the stem sits at backbone.layer1.{0,1} and layer1's blocks at backbone.layer1.4.B), every key behind a
    'module.' prefix, the whole dict under 'model_state_dict'."""
    alias = {}
    for k, v in sd.items():
        if k.startswith("backbone.model.layer"):
            li = int(k[len("backbone.model.layer")])
            rest = k[len("backbone.model.layerN."):]
            alias[f"backbone.layer{li}.{'4.' if li == 1 else ''}{rest}"] = v
        elif k.startswith("backbone.model.conv1."):
            alias["backbone.layer1.0." + k[len("backbone.model.conv1."):]] = v
        elif k.startswith("backbone.model.bn1."):
            alias["backbone.layer1.1." + k[len("backbone.model.bn1."):]] = v
        else:
            alias[k] = v
    assert not any(k.startswith("backbone.model.") for k in alias)
    return {"model_state_dict": {"module." + k: v for k, v in alias.items()}, "epoch": 3}


# ------------------------------------------------------------------ 16-bit emulation (for the error budgets of the bf16 / f16 modes)
def _q(t, dtype):
    return t.to(dtype).float()


@torch.no_grad()
def forward_lowp_emulation(sd, x, dtype, return_feats=False):
    """The fp32 reference with the storage of a 16-bit mode: the BN-folded conv weights (what the library packs) and every activation that
    is written to memory -- each layer's output after its fused bias / residual / ReLU epilogue -- rounded to `dtype` (torch.bfloat16 /
    torch.float16); arithmetic, biases, the deformable offsets and masks, the ASF attention and the head's fused deconvolution tail stay
    fp32, as in the library.  Either backbone, with or without DCN (read off the keys).  It says how far 16-bit STORAGE alone moves the
    maps on given weights and input; the library's reduction order and fused epilogues differ from it.
    It takes the folded weights and the architecture from the product's own ``weights.fold_det`` / ``det_arch``, so it is NOT independent of
    the folding: a folding error would move this bound and the library's output together.  What pins the folding is the fp32 / f16x2 tests,
    which compare the library against the unfolded references above (and test_backbones_cpu.py's conv2 + bn2 check)."""
    from ocr_vi_invoice_amd import weights
    from oracle.dbnet_cpu import deform_conv2d_gather
    backbone, dcn = weights.det_arch(sd)
    basic = backbone == "resnet18"
    f = {k: torch.from_numpy(v) for k, v in weights.fold_det(sd).items()}

    def q(t):
        return _q(t, dtype)

    def conv(name, t, stride=1, pad=0, relu=False, res=None):
        y = F.conv2d(t, q(f[name + ".w"]), f[name + ".b"], stride, pad)
        if res is not None:
            y = y + res
        return q(F.relu(y) if relu else y)

    def deform(name, t, stride, relu, res=None):
        om = F.conv2d(t, q(f[name + ".off.w"]), f[name + ".off.b"], stride, 1)                 # fp32 offsets / masks
        y = deform_conv2d_gather(t, om[:, :18], torch.sigmoid(om[:, 18:]), q(f[name + ".w"]), stride) + f[name + ".b"].view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return q(F.relu(y) if relu else y)

    y = conv("stem", q(x.float()), 2, 3, relu=True)
    y = F.max_pool2d(y, 3, 2, 1)
    feats = []
    for li, nblk in enumerate(R18_BLOCKS if basic else [3, 4, 6, 3], start=1):
        for b in range(nblk):
            p = f"layer{li}.{b}"
            stride = 2 if (b == 0 and li > 1) else 1
            use_dcn = dcn and li >= 2
            idn = conv(p + ".down", y, stride) if (p + ".down.w") in f else y
            if basic:
                t = conv(p + ".conv1", y, stride, 1, relu=True)
                y = deform(p + ".conv2", t, 1, True, idn) if use_dcn else conv(p + ".conv2", t, 1, 1, relu=True, res=idn)
            else:
                t = conv(p + ".conv1", y, relu=True)
                t = deform(p + ".conv2", t, stride, True) if use_dcn else conv(p + ".conv2", t, stride, 1, relu=True)
                y = conv(p + ".conv3", t, relu=True, res=idn)
        feats.append(y)
    # FPN (neck.py:26-41): lateral + nearest-2x of the level above in the lateral's epilogue, then 3x3 + BN + ReLU
    inner, ps = None, [None] * 4
    for i in (3, 2, 1, 0):
        inner = conv(f"neck.lat{i}", feats[i], res=None if inner is None else F.interpolate(inner, size=feats[i].shape[-2:], mode="nearest"))
        ps[i] = conv(f"neck.fpn{i}", inner, 1, 1, relu=True)
    size = ps[0].shape[-2:]
    ups = [ps[0]] + [F.interpolate(p, size=size, mode="bilinear", align_corners=True) for p in ps[1:]]
    score = F.softmax(F.conv2d(torch.cat(ups, 1), f["neck.asf.w"].view(4, 1024, 1, 1), f["neck.asf.b"]), 1)
    fused = q(sum(u * score[:, i:i + 1] for i, u in enumerate(ups)))
    hc = conv("head.conv", fused, 1, 1, relu=True)                                             # both branches' 3x3: binarise = channels 0..63
    out = {}
    for j, (short, name) in enumerate((("bin", "bin_logits"), ("thr", "thresh_logits"))):
        t = F.relu(F.conv_transpose2d(hc[:, 64 * j:64 * j + 64], q(f[f"head.{short}.dc1.w"]), f[f"head.{short}.dc1.b"], 2))   # not stored
        out[name] = F.conv_transpose2d(t, f[f"head.{short}.dc2.w"], f[f"head.{short}.dc2.b"], 2)
    out["binary"], out["thresh"] = torch.sigmoid(out["bin_logits"]), torch.sigmoid(out["thresh_logits"])
    if return_feats:
        out = dict(out, c2=feats[0], c3=feats[1], c4=feats[2], c5=feats[3], fused=fused)
    return out
