"""What DBNetPP and SVTRv2 share: one libocrvi handle built from a state_dict or a packed blob, the nn.Module-like surface around it
(``load_state_dict`` / ``state_dict`` / ``to`` / ``eval``), the per-forward workspace cache and the f16x2 range flag.  A subclass names its
C entries, fills its cfg struct, folds its state_dict and adds its forwards."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, weights


class HandleModel:
    _NAME = ""              # the class name messages use
    _CREATE = _DESTROY = _STATUS = ""               # C symbols
    _WS_BYTES = {}          # forward kind -> the C symbol that sizes its workspace

    def _cfg(self):
        """The filled ``ocrvi_*_cfg`` struct of this model."""
        raise NotImplementedError

    def _fold(self, state_dict):
        """``weights.fold_*`` of this model (KeyError names a missing tensor)."""
        raise NotImplementedError

    def _init_handle(self, dtype, device, seed, state_dict, blob, make_state_dict):
        """The end of a constructor, once the architecture attributes ``_cfg`` and ``_fold`` read are set."""
        self.device = torch.device(device)
        self.dtype = _lib.dtype_code(dtype)
        self._handle = None
        self._ws = {}
        self.training = False
        self._seed = seed
        if blob is not None:        # already folded + packed (weights.pack_blob): what rank 0 broadcasts to the other ranks
            self.load_blob(blob)
        else:
            self.load_state_dict(state_dict if state_dict is not None else make_state_dict())

    # ---- nn.Module-like surface used by the pipeline (pipeline2.py:45-53, 72-82)
    def load_state_dict(self, state_dict, strict: bool = True):
        """nn.Module.load_state_dict semantics for the keys the inference graph uses: with ``strict`` (default) a missing tensor
        raises KeyError-as-RuntimeError like torch does; keys the graph does not read (the detector's duplicate ``backbone.layerN``
        aliases and unused ``fc``, the recogniser's training-only ``sgm.*``, svtrv2.py:252-385, optimizer state in a wrapped checkpoint)
        are ignored, as the reference's loader effectively does."""
        if not strict:
            # nn.Module semantics: tensors the given dict lacks keep their current values.  A model built from a packed blob (the
            # ranks behind the weight broadcast, bench.py) retains no unfolded state_dict to merge into: refuse rather than fill the
            # missing tensors with seeded random values
            if getattr(self, "_state", None) is None:
                raise RuntimeError("load_state_dict(strict=False) on a model built from a packed blob: no state_dict is retained to "
                                   "keep the missing tensors from; build the model from a state_dict, or load a complete one")
            base = dict(self._state)
            base.update(weights.unwrap_checkpoint(state_dict))
            state_dict = base
        try:
            folded = self._fold(state_dict)
        except KeyError as e:
            raise RuntimeError(f"Error(s) in loading state_dict for {self._NAME}: missing key {e}") from None
        self._state = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in weights.unwrap_checkpoint(state_dict).items()}
        return self.load_blob(weights.pack_blob(folded), _from_state=True)

    def state_dict(self):
        """The state_dict this model was loaded from (reference key schema); None-safe copy."""
        if getattr(self, "_state", None) is None:
            raise RuntimeError("model was built from a packed blob; no state_dict is retained")
        return dict(self._state)

    def load_blob(self, blob: bytes, _from_state: bool = False):
        if not _from_state:
            self._state = None      # a packed blob carries no unfolded state_dict (state_dict() / strict=False then raise)
        cfg = self._cfg()
        h = C.c_void_p()
        _lib.check(getattr(_lib.load(), self._CREATE)(self._dev_index(), blob, len(blob), C.byref(cfg), C.byref(h)))
        self._free()
        self._handle = h
        self._blob = blob
        return self

    def to(self, device):
        """Moves the model like nn.Module.to: a different device re-creates the handle there from the retained weights."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("libocrvi has no CPU path: the product runs on an MI355X (use the reference module for CPU)")
        if dev.index is None:     # model.to('cuda') (the reference's pattern, pipeline2.py:53) = the current device
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev != torch.device("cuda", self._dev_index()):
            if getattr(self, "_blob", None) is None:
                raise RuntimeError("no weights retained to move")
            self.device = dev
            self._ws = {}
            self.load_blob(self._blob)
        return self

    def eval(self):
        return self

    def _dev_index(self) -> int:
        return self.device.index if self.device.index is not None else torch.cuda.current_device()

    def _free(self):
        if getattr(self, "_handle", None):
            getattr(_lib.load(), self._DESTROY)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    # ---- workspaces
    def workspace_bytes(self, N, H, W, kind: str = "forward") -> int:
        """The workspace one ``kind`` forward of (N,3,H,W) needs; ValueError for a shape the graph does not take."""
        n = C.c_size_t()
        _lib.check(getattr(_lib.load(), self._WS_BYTES[kind])(self._handle, N, H, W, C.byref(n)))
        return n.value

    def _workspace(self, N, H, W, kind: str = "forward") -> torch.Tensor:
        """The cached workspace of the model's own forwards.  Each forward kind keeps one shape's buffer resident, apart from the other
        kinds': a captured graph of one forward holds its buffer's address, and running another forward must not free it."""
        key = (N, H, W)
        hit = self._ws.get(kind)
        if hit is not None and hit[0] == key:
            return hit[1]
        n = self.workspace_bytes(N, H, W, kind)
        self._ws.pop(kind, None)            # the previous shape's buffer goes before the new one is allocated
        ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._ws[kind] = (key, ws)
        return ws

    # ---- f16x2 range flag
    def range_status(self) -> int:
        """The C status of the last forward's range snapshot (0, or -5 with the message in ``_lib.last_error()``); the caller has
        synchronised the forward's stream."""
        return getattr(_lib.load(), self._STATUS)(self._handle)

    def check_range(self) -> None:
        """f16x2 mode only (a no-op otherwise): synchronise the current stream and raise OverflowError if an activation left fp16's
        exponent range (|x| >= 65520) during a forward -- the one way this mode can fail to stand in for the reference's fp32 path
        (pipeline2.py:312-318).  A forward itself never synchronises; the pipeline helpers and the decode paths call this where they
        already wait for the result (``.cpu()``, pipeline2.py:320; ``.tolist()``, svtrv2.py:562)."""
        if self.dtype == _lib.OCRVI_F16X2:
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self.range_status())

    def reset_range(self) -> None:
        """Clear the device's (sticky) f16x2 range flag, e.g. after handling an OverflowError."""
        _lib.check(_lib.load().ocrvi_range_reset(self._dev_index(), torch.cuda.current_stream(self.device).cuda_stream))
