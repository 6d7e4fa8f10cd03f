"""DBNet++ detector on libocrvi -- host-side mirror of the reference module's inference API
(model/det/dbnet.py:6-17): same constructor arguments and the same five-map output dict (head.py:42-48)."""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, weights
from ._model import HandleModel

MAPS = ("binary", "thresh", "thresh_binary", "bin_logits", "thresh_logits")


class DBNetPP(HandleModel):
    _NAME = "DBNetPP"
    _CREATE, _DESTROY, _STATUS = "ocrvi_det_create", "ocrvi_det_destroy", "ocrvi_det_status"
    _WS_BYTES = {"forward": "ocrvi_det_workspace_bytes", "binary": "ocrvi_det_binary_workspace_bytes"}

    def __init__(self, backbone: str = "resnet50", pretrained: bool = False, in_channels: int = 3, inner_channels: int = 256,
                 k: float = 50, dcn: bool = True, *, state_dict=None, blob: bytes = None, seed: int = 1234, dtype="f32",
                 device="cuda:0"):
        if backbone not in weights.DET_BACKBONES:
            # backbone.py:12-15 offers resnet50 and resnet18 and raises the same for anything else
            raise NotImplementedError(f"Backbone {backbone} not implemented")
        if pretrained:
            raise RuntimeError("pretrained=True downloads torchvision ImageNet weights (backbone.py:17); there is no network -- "
                               "pass state_dict= (inference callers use pretrained=False, pipeline2.py:45)")
        if in_channels != 3 or inner_channels != 256:
            raise ValueError("only in_channels=3 and inner_channels=256 (the reference's defaults, dbnet.py:7) are built")
        self.backbone = backbone
        self.dcn = bool(dcn)
        self.k = float(k)
        self._init_handle(dtype, device, seed, state_dict, blob, lambda: weights.make_det_state_dict(seed, backbone=self.backbone, dcn=self.dcn))

    def _fold(self, state_dict):
        try:
            return weights.fold_det(state_dict, backbone=self.backbone, dcn=self.dcn)
        except weights.UnexpectedKeyError as e:
            raise RuntimeError(f"Error(s) in loading state_dict for DBNetPP(backbone={self.backbone!r}, dcn={self.dcn}): unexpected key {e} "
                               "(the state_dict is of another architecture)") from None

    def _cfg(self):
        cfg = _lib.DetCfg()
        cfg.dtype = self.dtype
        cfg.k = self.k
        cfg.max_batch = 0
        cfg.backbone = weights.DET_BACKBONES.index(self.backbone)
        cfg.no_dcn = 0 if self.dcn else 1
        return cfg

    # ---- the two C forwards, enqueue-only: raw device pointers, sizes and a stream; nothing is allocated or synchronised
    def enqueue_forward(self, x, N, H, W, maps, ws, ws_bytes, stream) -> None:
        """``ocrvi_det_forward``.  ``maps``: the five output pointers in ``MAPS`` order; all but the first may be None."""
        _lib.check(_lib.load().ocrvi_det_forward(self._handle, x, N, H, W, *maps, ws, ws_bytes, stream))

    def enqueue_forward_binary(self, x, N, H, W, binary, ws, ws_bytes, stream) -> None:
        """``ocrvi_det_forward_binary``; its workspace is sized by ``workspace_bytes(N, H, W, "binary")``."""
        _lib.check(_lib.load().ocrvi_det_forward_binary(self._handle, x, N, H, W, binary, ws, ws_bytes, stream))

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected (N,3,H,W) input, got {tuple(x.shape)}")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def forward(self, x: torch.Tensor, binary_only: bool = False) -> Dict[str, torch.Tensor]:
        """(N,3,H,W), H,W % 32 == 0 -> {'binary','thresh','thresh_binary','bin_logits','thresh_logits'}, each (N,1,H,W) float32
        on the device (dbnet.py:13-17, head.py:42-48).  ``binary_only`` skips writing the four maps the pipeline never reads
        (pipeline2.py:318)."""
        x = self._input(x)
        N, _, H, W = x.shape
        ws = self._workspace(N, H, W)
        out = {n: torch.empty((N, 1, H, W), dtype=torch.float32, device=self.device) for n in (MAPS[:1] if binary_only else MAPS)}
        self.enqueue_forward(x.data_ptr(), N, H, W, [_lib.ptr(out.get(n)) for n in MAPS], ws.data_ptr(), ws.numel(),
                             torch.cuda.current_stream(self.device).cuda_stream)
        return out

    __call__ = forward

    def forward_binary(self, x: torch.Tensor) -> torch.Tensor:
        """(N,3,H,W), H,W % 32 == 0 -> the ``binary`` map (N,1,H,W) float32 alone: what the page loop reads of the reference's dict
        (``preds['binary']``, pipeline2.py:318).  Unlike ``forward(x, binary_only=True)``, which computes the whole two-branch head and skips
        four stores, this runs the binarise branch only (head.py:34): the threshold branch (head.py:38) is not computed and no logit map is
        written.  Same bits as ``forward(x)['binary']`` in the f32 and f16x2 modes.  Its workspace is cached apart from ``forward``'s."""
        x = self._input(x)
        N, _, H, W = x.shape
        ws = self._workspace(N, H, W, "binary")
        out = torch.empty((N, 1, H, W), dtype=torch.float32, device=self.device)
        self.enqueue_forward_binary(x.data_ptr(), N, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def debug_features(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Test hook: c2..c5 and the fused neck feature as float32 NCHW, after a forward on x."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        N, _, H, W = x.shape
        self.forward(x, binary_only=True)
        ex = 1 if self.backbone == "resnet18" else 4     # BasicBlocks do not expand
        shapes = {"c2": (64 * ex, 4), "c3": (128 * ex, 8), "c4": (256 * ex, 16), "c5": (512 * ex, 32), "fused": (256, 4)}
        out = {k: torch.empty((N, c, H // s, W // s), dtype=torch.float32, device=self.device) for k, (c, s) in shapes.items()}
        ws = self._workspace(N, H, W)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.load().ocrvi_det_debug_features(self._handle, N, H, W, *[out[k].data_ptr() for k in ("c2", "c3", "c4", "c5", "fused")],
                                                        ws.data_ptr(), ws.numel(), stream))
        return out
