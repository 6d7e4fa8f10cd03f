"""CPU checks of the detector's backbone configurations (ResNet-50 / ResNet-18, with / without DCN): the reference functions of
tests/backbone_refs.py against themselves, the synthetic state_dict schema, fold_det's inference from the keys, the blob round trip,
the unchanged default weights, and what of the facade and the C ABI needs no GPU."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_refs as R  # noqa: E402

from ocr_vi_invoice_amd import weights  # noqa: E402
from oracle import dbnet_cpu  # noqa: E402

WIDTH = [64, 128, 256, 512]


def _digest(t) -> str:
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]


# ------------------------------------------------------------------ the references against themselves
def _zero_dcn_init(sd):
    """dcn.py:28-29: the offset / mask conv starts all zero -> offsets 0, mask sigmoid(0) = 0.5."""
    sd = dict(sd)
    for k in sd:
        if ".offset_mask_conv." in k:
            sd[k] = torch.zeros_like(sd[k])
    return sd


def _halved_plain(sd):
    """The same weights without the offset convs and with conv2 of every block of layers 2-4 halved."""
    out = {}
    for k, v in sd.items():
        if ".offset_mask_conv." in k:
            continue
        deform = k.endswith(".conv2.weight") and any(f"layer{li}." in k for li in (2, 3, 4))
        out[k] = v * 0.5 if deform else v
    return out


@pytest.mark.parametrize("backbone", ["resnet18", "resnet50"])
def test_dcn_backbone_at_the_reference_init_is_the_plain_backbone_with_halved_conv2(backbone):
    """Zero offsets sample the regular 3x3 grid and a mask of 0.5 halves every tap, so DeformableConv2d(x) == conv2d(x, w / 2): ties the
    DCN wiring of each block type (which conv is replaced, at which stride) to the plain path."""
    sd = _zero_dcn_init(weights.make_det_state_dict(seed=5, backbone=backbone, dcn=True))
    plain = _halved_plain(sd)
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    bb = R.backbone18 if backbone == "resnet18" else dbnet_cpu.backbone
    with torch.no_grad():
        a, b = bb(sd, x, dcn=True), bb(plain, x, dcn=False)
    for li, (fa, fb) in enumerate(zip(a, b)):
        scale = float(fb.abs().max())
        assert scale > 0.1
        # fp32 round-off of two summation orders (gather + matmul vs conv2d) through <= 16 blocks
        assert float((fa - fb).abs().max()) < 2e-5 * max(scale, 1.0), li


def test_resnet18_reference_shapes_and_block_wiring():
    sd = weights.make_det_state_dict(seed=6, backbone="resnet18", dcn=True)
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    out = R.forward18(sd, x, dcn=True, return_feats=True)
    for i, k in enumerate(("c2", "c3", "c4", "c5")):
        assert out[k].shape == (2, WIDTH[i], 64 >> (i + 2), 96 >> (i + 2))
    assert out["fused"].shape == (2, 256, 16, 24) and out["binary"].shape == (2, 1, 64, 96)
    # one block by hand: layer2.0 = relu(bn2(dcn(relu(bn1(conv1 s2)))) + bn(down s2))
    import torch.nn.functional as F
    p = "backbone.model.layer2.0"
    t = torch.randn(1, 64, 10, 12, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y = F.relu(dbnet_cpu._bn(sd, p + ".bn1", F.conv2d(t, sd[p + ".conv1.weight"], None, 2, 1)))
        y = dbnet_cpu._bn(sd, p + ".bn2", dbnet_cpu.dcn_module(sd, p + ".conv2", y, 1))
        idn = dbnet_cpu._bn(sd, p + ".downsample.1", F.conv2d(t, sd[p + ".downsample.0.weight"], None, 2))
        want = F.relu(y + idn)
        got = R.basic_block(sd, p, t, 2, True, True)
    assert got.shape == (1, 128, 5, 6) and torch.equal(got, want)


# ------------------------------------------------------------------ synthetic weights
def test_default_det_weights_are_the_ones_the_parent_commit_drew():
    """Digests taken from make_det_state_dict as it stood before it learnt `backbone=` / `dcn=`: every existing test and the benchmark see
    the same tensors."""
    want = {
        1234: {"backbone.model.conv1.weight": "7e1b1a5a7594c106",
               "backbone.model.layer2.0.conv2.offset_mask_conv.weight": "1b3308492e57509d",
               "backbone.model.layer4.2.bn3.running_var": "0d61e35f839b3ef9",
               "neck.lateral_convs.3.weight": "b3a6bf4ec7fedb8b",
               "head.thresh_conv.4.bias": "dd25ea8c95601a13"},
        21: {"backbone.model.conv1.weight": "4c62157fbce297a6",
             "backbone.model.layer2.0.conv2.offset_mask_conv.weight": "a3089988b1faa0ea",
             "backbone.model.layer4.2.bn3.running_var": "a509c35331027e27",
             "neck.lateral_convs.3.weight": "92cf75f0f9165adf",
             "head.thresh_conv.4.bias": "f6e54f04997cb416"},
    }
    whole = {1234: "401718cc2502136b", 21: "73fed1a4a092af83"}
    for seed, tensors in want.items():
        sd = weights.make_det_state_dict(seed)
        assert len(sd) == 408
        for k, d in tensors.items():
            assert _digest(sd[k]) == d, (seed, k)
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode())
            h.update(v.numpy().tobytes())
        assert h.hexdigest()[:16] == whole[seed]
        explicit = weights.make_det_state_dict(seed, 1.5, "resnet50", True)
        assert list(explicit) == list(sd) and all(torch.equal(explicit[k], sd[k]) for k in sd)


@pytest.mark.parametrize("dcn", [True, False])
def test_resnet18_state_dict_schema(dcn):
    sd = weights.make_det_state_dict(seed=7, backbone="resnet18", dcn=dcn)
    bb = "backbone.model."
    assert sd[bb + "conv1.weight"].shape == (64, 3, 7, 7)
    inpl = 64
    expected = {bb + "conv1.weight"} | {bb + "bn1." + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    for li, w in enumerate(WIDTH, start=1):
        for b in range(2):
            p = f"{bb}layer{li}.{b}"
            assert sd[p + ".conv1.weight"].shape == (w, inpl, 3, 3)
            assert sd[p + ".conv2.weight"].shape == (w, w, 3, 3)
            assert sd[p + ".bn1.weight"].shape == sd[p + ".bn2.running_var"].shape == (w,)
            names = [".conv1.weight", ".conv2.weight"]
            bns = [".bn1", ".bn2"]
            if b == 0 and li >= 2:
                assert sd[p + ".downsample.0.weight"].shape == (w, inpl, 1, 1)
                names.append(".downsample.0.weight")
                bns.append(".downsample.1")
            else:
                assert p + ".downsample.0.weight" not in sd
            if dcn and li >= 2:
                assert sd[p + ".conv2.offset_mask_conv.weight"].shape == (27, w, 3, 3)
                assert sd[p + ".conv2.offset_mask_conv.bias"].shape == (27,)
                names += [".conv2.offset_mask_conv.weight", ".conv2.offset_mask_conv.bias"]
            else:
                assert p + ".conv2.offset_mask_conv.weight" not in sd
            assert p + ".conv3.weight" not in sd and p + ".bn3.weight" not in sd
            expected |= {p + n for n in names}
            expected |= {p + q + "." + s for q in bns for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
            inpl = w
    assert {k for k in sd if k.startswith(bb)} == expected
    for i, w in enumerate(WIDTH):
        assert sd[f"neck.lateral_convs.{i}.weight"].shape == (256, w, 1, 1)
    # neck (beyond the laterals' inputs) and head have the ResNet-50 model's keys and shapes
    r50 = weights.make_det_state_dict(seed=7)
    rest = [k for k in r50 if not k.startswith(bb)]
    assert [k for k in sd if not k.startswith(bb)] == rest
    assert all(sd[k].shape == r50[k].shape for k in rest if "lateral_convs" not in k or k.endswith(".bias"))
    with pytest.raises(NotImplementedError):
        weights.make_det_state_dict(backbone="resnet101")


def test_resnet50_without_dcn_drops_only_the_offset_convs():
    a, b = weights.make_det_state_dict(seed=8), weights.make_det_state_dict(seed=8, dcn=False)
    assert [k for k in a if ".offset_mask_conv." not in k] == list(b)
    assert sum(".offset_mask_conv." in k for k in a) == 2 * 13


# ------------------------------------------------------------------ folding
CONFIGS = [("resnet50", True), ("resnet50", False), ("resnet18", True), ("resnet18", False)]


@pytest.mark.parametrize("backbone,dcn", CONFIGS)
def test_fold_det_infers_the_architecture_from_the_keys(backbone, dcn):
    sd = weights.make_det_state_dict(seed=9, backbone=backbone, dcn=dcn)
    assert weights.det_arch(sd) == (backbone, dcn)
    f = weights.fold_det(sd)
    basic = backbone == "resnet18"
    blocks = [2, 2, 2, 2] if basic else [3, 4, 6, 3]
    ex = 1 if basic else 4
    inpl = 64
    for li, (n, w) in enumerate(zip(blocks, WIDTH), start=1):
        for b in range(n):
            p = f"layer{li}.{b}"
            assert f[p + ".conv1.w"].shape == ((w, inpl, 3, 3) if basic else (w, inpl, 1, 1))
            assert f[p + ".conv2.w"].shape == (w, w, 3, 3) and f[p + ".conv2.b"].shape == (w,)
            assert ((p + ".conv3.w") in f) == (not basic)
            assert ((p + ".conv2.off.w") in f) == (dcn and li >= 2)
            assert ((p + ".down.w") in f) == (b == 0 and (not basic or li >= 2))
            if (p + ".down.w") in f:
                assert f[p + ".down.w"].shape == (ex * w, inpl, 1, 1)
            inpl = ex * w
    for i, w in enumerate(WIDTH):
        assert f[f"neck.lat{i}.w"].shape == (256, ex * w, 1, 1)
    # the same with the expectation stated
    g = weights.fold_det(sd, backbone=backbone, dcn=dcn)
    assert list(g) == list(f) and all(np.array_equal(g[k], f[k]) for k in f)
    # and stated wrongly: a KeyError that names the deciding key
    other = "resnet18" if backbone == "resnet50" else "resnet50"
    with pytest.raises(KeyError, match=r"layer1\.0\.conv3\.weight"):
        weights.fold_det(sd, backbone=other)
    with pytest.raises(KeyError, match=r"layer2\.0\.conv2\.offset_mask_conv\.weight"):
        weights.fold_det(sd, dcn=not dcn)
    with pytest.raises(NotImplementedError):
        weights.fold_det(sd, backbone="resnet101")


def test_fold_det_folds_bn2_into_a_basic_blocks_conv2():
    import torch.nn.functional as F
    sd = weights.make_det_state_dict(seed=10, backbone="resnet18", dcn=False)
    f = weights.fold_det(sd)
    p = "backbone.model.layer3.1"
    x = torch.randn(1, 256, 6, 7, generator=torch.Generator().manual_seed(1))
    want = dbnet_cpu._bn(sd, p + ".bn2", F.conv2d(x, sd[p + ".conv2.weight"], None, 1, 1))
    got = F.conv2d(x, torch.from_numpy(f["layer3.1.conv2.w"]), torch.from_numpy(f["layer3.1.conv2.b"]), 1, 1)
    assert float((got - want).abs().max()) < 1e-5 * float(want.abs().max())


def test_fold_det_takes_resnet18_checkpoint_wrappers_and_aliases():
    """The reference's state_dict() carries the backbone under backbone.layerN.* too (layer1 = Sequential(conv1, bn1, relu, maxpool,
    layer1), so its blocks sit at backbone.layer1.4.B); trainers wrap it in {'model_state_dict': ...} with a 'module.' prefix."""
    sd = weights.make_det_state_dict(seed=11, backbone="resnet18", dcn=True)
    want = weights.fold_det(sd)
    wrapped = R.as_reference_checkpoint(sd)
    assert weights.det_arch(wrapped) == ("resnet18", True)
    got = weights.fold_det(wrapped)
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("backbone,dcn", CONFIGS[1:])
def test_blob_round_trip_of_the_new_configurations(backbone, dcn):
    f = weights.fold_det(weights.make_det_state_dict(seed=12, backbone=backbone, dcn=dcn))
    back = weights.unpack_blob(weights.pack_blob(f))
    assert list(back) == list(f)
    assert all(np.array_equal(back[k], f[k]) and back[k].dtype == np.float32 for k in f)


# ------------------------------------------------------------------ facade and C ABI, as far as they need no GPU
def test_facade_constructor_errors_need_no_gpu():
    from ocr_vi_invoice_amd import DBNetPP
    for bad in ("resnet101", "resnet34", ""):
        with pytest.raises(NotImplementedError, match="not implemented"):
            DBNetPP(backbone=bad)
    for bb in ("resnet18", "resnet50"):
        with pytest.raises(ValueError, match="in_channels"):
            DBNetPP(backbone=bb, in_channels=1)
        with pytest.raises(ValueError, match="inner_channels"):
            DBNetPP(backbone=bb, inner_channels=128, dcn=False)
        with pytest.raises(RuntimeError, match="pretrained"):
            DBNetPP(backbone=bb, pretrained=True)


def test_det_cfg_keeps_its_layout_and_the_new_hook_is_exported():
    from ocr_vi_invoice_amd import _lib
    assert C.sizeof(_lib.DetCfg) == 32
    assert (_lib.DetCfg.backbone.offset, _lib.DetCfg.no_dcn.offset, _lib.DetCfg.reserved.offset) == (12, 16, 20)
    z = _lib.DetCfg()
    assert (z.backbone, z.no_dcn) == (0, 0)          # a zeroed struct is ResNet-50 with DCN
    assert "ocrvi_test_deform_conv_res" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "ocrvi_test_deform_conv_res")
    assert lib.ocrvi_abi_version() == 5
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "ocrvi.h")).read()
    assert "int32_t backbone;" in header and "int32_t no_dcn;" in header and "int32_t reserved[3];" in header


def test_det_create_refuses_a_bad_cfg_before_it_touches_the_blob():
    """cfg validation runs before blob parsing and before any device call."""
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    for field, val in (("backbone", 2), ("backbone", -1), ("no_dcn", 2), ("no_dcn", -1)):
        cfg = _lib.DetCfg()
        setattr(cfg, field, val)
        h = C.c_void_p()
        rc = lib.ocrvi_det_create(0, b"", 0, C.byref(cfg), C.byref(h))
        assert rc == -1 and field in _lib.last_error(), (field, val, rc, _lib.last_error())
        assert not h.value
