"""SVTRv2 recogniser on libocrvi -- host-side mirror of the reference module's inference API
(model/rec2/svtrv2.py:410-569): same constructor arguments, ``forward`` / ``decode_probs`` /
``decode_greedy`` semantics and attributes (``tokenizer``, ``blank_id``, ``dims``)."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, weights
from ._model import HandleModel
from .vocab import VOCAB, Tokenizer


class Recognition(NamedTuple):
    """One recognised line with the greedy CTC path's confidences (``return_confidence=True``).  ``char_scores[i]`` is exp of the largest
    log-probability the path gave character i over the steps of its run, ``spans[i] = (t0, t1)`` that run (inclusive steps of T = W / 4;
    include/ocrvi.h, ``ocrvi_ctc_greedy_conf``); both cover exactly the characters of ``text``.  ``score`` is their mean (0.0 for an empty
    string): the path's own per-character maximum, not a calibrated probability.  ``log_prob`` is the log-probability of the collapsed id
    sequence over all alignments (``-ocrvi_ctc_loss``), or ``None`` where no log-probabilities were kept."""
    text: str
    score: float
    char_scores: Tuple[float, ...]
    spans: Tuple[Tuple[int, int], ...]
    log_prob: Optional[float]


def make_recognitions(tokenizer: Tokenizer, ids, lens, char_lp, char_span, log_probs: Optional[Sequence[float]] = None) -> List[Recognition]:
    """Host half of the confidences: the device's exact ``ids`` [n,T] / ``lens`` [n] / ``char_lp`` [n,T] / ``char_span`` [n,T,2] on the
    host (numpy arrays or anything ``np.asarray`` takes) -> one ``Recognition`` per row, in float64.  An id outside
    ``tokenizer.id_to_token`` (pad id 1) is dropped from text, scores and spans alike, as ``Tokenizer.decode`` drops it from the text.
    Only the ``lens[b]`` valid entries of a row become Python objects."""
    ids, lens, char_lp, char_span = np.asarray(ids), np.asarray(lens), np.asarray(char_lp), np.asarray(char_span)
    tokens = tokenizer.id_to_token
    out = []
    for b in range(len(lens)):
        n = int(lens[b])
        row = ids[b, :n].tolist()
        keep = [k for k, i in enumerate(row) if i in tokens]
        if len(keep) == n:
            lp, sp = char_lp[b, :n].tolist(), char_span[b, :n].tolist()
        else:
            lp, sp = char_lp[b, keep].tolist(), char_span[b, keep].tolist()
            row = [row[k] for k in keep]
        scores = tuple([math.exp(v) for v in lp])
        out.append(Recognition("".join([tokens[i] for i in row]), math.fsum(scores) / len(scores) if scores else 0.0, scores,
                               tuple([(t0, t1) for t0, t1 in sp]), None if log_probs is None else float(log_probs[b])))
    return out


class SVTRv2(HandleModel):
    _NAME = "SVTRv2"
    _CREATE, _DESTROY, _STATUS = "ocrvi_rec_create", "ocrvi_rec_destroy", "ocrvi_rec_status"
    _WS_BYTES = {"forward": "ocrvi_rec_workspace_bytes"}

    def __init__(self, variant: str = "small", in_channels: int = 3, charset=VOCAB, dropout: float = 0.0,
                 context_window: int = 3, *, state_dict=None, blob: bytes = None, seed: int = 1234, dtype="f32", device="cuda:0"):
        assert variant in weights.REC_VARIANTS, \
            f"Unknown variant: {variant}. Choose from {list(weights.REC_VARIANTS.keys())}"  # svtrv2.py:425
        if in_channels != 3:
            raise ValueError("only 3-channel input is supported (pipeline2.py:74 uses in_channels=3)")
        self.variant = variant
        self.tokenizer = Tokenizer(charset)
        if self.tokenizer.num_classes != weights.NUM_CLASSES:
            raise ValueError(f"charset gives {self.tokenizer.num_classes} classes; kernels are built for {weights.NUM_CLASSES}")
        self.blank_id = self.tokenizer.blank_id
        self.dims = list(weights.REC_VARIANTS[variant]["dims"])
        self._init_handle(dtype, device, seed, state_dict, blob, lambda: weights.make_rec_state_dict(variant, seed))

    def _fold(self, state_dict):
        return weights.fold_rec(state_dict, self.variant)

    def _cfg(self):
        cfg = _lib.RecCfg()
        v = weights.REC_VARIANTS[self.variant]
        cfg.dtype = self.dtype
        cfg.dims[:] = v["dims"]
        cfg.num_blocks[:] = v["num_blocks"]
        cfg.num_local[:] = v["num_local"]
        cfg.num_classes = self.tokenizer.num_classes
        cfg.blank_id = self.blank_id
        return cfg

    def enqueue_forward(self, x, B, H, W, log_probs, argmax, ids, lens, ws, ws_bytes, stream) -> None:
        """``ocrvi_rec_forward``, enqueue-only: raw device pointers (any output may be None), sizes and a stream; nothing is allocated
        or synchronised."""
        _lib.check(_lib.load().ocrvi_rec_forward(self._handle, x, B, H, W, log_probs, argmax, ids, lens, ws, ws_bytes, stream))

    def enqueue_forward_conf(self, x, B, H, W, log_probs, argmax, ids, lens, best_lp, char_lp, char_span, ws, ws_bytes, stream) -> None:
        """``ocrvi_rec_forward_conf``, enqueue-only like ``enqueue_forward``: the same four outputs plus best_lp / char_lp [B,T] float32 and
        char_span [B,T,2] int32 (any may be None)."""
        _lib.check(_lib.load().ocrvi_rec_forward_conf(self._handle, x, B, H, W, log_probs, argmax, ids, lens, best_lp, char_lp, char_span, ws,
                                                      ws_bytes, stream))

    def _run(self, x: torch.Tensor, want_log_probs: bool, want_ids: bool):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected (B,3,H,W) input, got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        T = W // 4
        ws = self._workspace(B, H, W)
        lp = torch.empty((T, B, self.tokenizer.num_classes), dtype=torch.float32, device=self.device) if want_log_probs else None
        am = ids = lens = None
        if want_ids:
            am = torch.empty((B, T), dtype=torch.int32, device=self.device)
            ids = torch.empty((B, T), dtype=torch.int32, device=self.device)
            lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        self.enqueue_forward(x.data_ptr(), B, H, W, _lib.ptr(lp), _lib.ptr(am), _lib.ptr(ids), _lib.ptr(lens), ws.data_ptr(), ws.numel(),
                             torch.cuda.current_stream(self.device).cuda_stream)
        return lp, am, ids, lens

    def forward(self, x: torch.Tensor, targets=None) -> torch.Tensor:
        """(B,3,H,W) -> log_probs (T=W/4, B, num_classes) float32 on the device (svtrv2.py:503-536)."""
        if targets is not None:
            raise NotImplementedError("the SGM training branch (svtrv2.py:519-522) is out of scope of the inference engine")
        return self._run(x, True, False)[0]

    __call__ = forward

    def debug_features(self, x: torch.Tensor):
        """Test hook: (backbone_norm [B,N,D], frm [B,T,D]) after a forward on x."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        self._run(x, False, False)
        d = self.dims[2]
        bn = torch.empty((B, (H // 16) * (W // 4), d), dtype=torch.float32, device=self.device)
        frm = torch.empty((B, W // 4, d), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, H, W)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.load().ocrvi_rec_debug_features(self._handle, B, H, W, bn.data_ptr(), frm.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return bn, frm

    def _ids_to_text(self, ids: torch.Tensor, lens: torch.Tensor) -> List[str]:
        ids_h, lens_h = ids.cpu().tolist(), lens.cpu().tolist()
        self.check_range()      # (the copies above synchronised the stream already)
        return self.tokenizer.decode([row[:n] for row, n in zip(ids_h, lens_h)])

    def _conf_buffers(self, B: int, T: int):
        d = dict(device=self.device)
        return (torch.empty((B, T), dtype=torch.int32, **d), torch.empty((B, T), dtype=torch.int32, **d), torch.empty((B,), dtype=torch.int32, **d),
                torch.empty((B, T), dtype=torch.float32, **d), torch.empty((B, T), dtype=torch.float32, **d),
                torch.empty((B, T, 2), dtype=torch.int32, **d))

    def _recognitions(self, lp: torch.Tensor, ids, lens, char_lp, char_span) -> List[Recognition]:
        """Device outputs -> ``Recognition`` rows; ``log_prob = -ocrvi_ctc_loss`` of ``lp`` with the device ids / lens as targets."""
        T, B, Cn = lp.shape
        logp = None
        if T <= _lib.CTC_LOSS_MAX_TARGET:
            nll = torch.empty(B, dtype=torch.float64, device=self.device)
            _lib.check(_lib.load().ocrvi_ctc_loss(self._dev_index(), lp.data_ptr(), T, B, Cn, ids.data_ptr(), T, lens.data_ptr(), None,
                                                  self.blank_id, nll.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
            logp = (-nll).cpu().tolist()
        rows = [t.cpu().numpy() for t in (ids, lens, char_lp, char_span)]
        self.check_range()      # (the copies above synchronised the stream already)
        return make_recognitions(self.tokenizer, *rows, logp)

    def decode_probs(self, log_probs: torch.Tensor, return_confidence: bool = False):
        """Greedy CTC decode of (T,B,C) log-probs (svtrv2.py:545-569): argmax, collapse repeats, drop blank on the
        device; id -> text (dropping pad id 1, tokenizer.py:73) on the host.  ``return_confidence=True``: a list of ``Recognition``
        (``ocrvi_ctc_greedy_conf``) whose ``text`` are the strings returned otherwise."""
        lp = log_probs.to(device=self.device, dtype=torch.float32).contiguous()
        T, B, Cn = lp.shape
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if return_confidence:
            am, ids, lens, blp, clp, span = self._conf_buffers(B, T)
            _lib.check(_lib.load().ocrvi_ctc_greedy_conf(self._dev_index(), lp.data_ptr(), T, B, Cn, self.blank_id, am.data_ptr(), ids.data_ptr(),
                                                         lens.data_ptr(), blp.data_ptr(), clp.data_ptr(), span.data_ptr(), stream))
            return self._recognitions(lp, ids, lens, clp, span)
        am = torch.empty((B, T), dtype=torch.int32, device=self.device)
        ids = torch.empty((B, T), dtype=torch.int32, device=self.device)
        lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.load().ocrvi_ctc_greedy(self._dev_index(), lp.data_ptr(), T, B, Cn, self.blank_id, am.data_ptr(), ids.data_ptr(),
                                                lens.data_ptr(), stream))
        return self._ids_to_text(ids, lens)

    def decode_greedy(self, images: torch.Tensor, return_confidence: bool = False):
        """forward + decode in one device pass (svtrv2.py:538-543).  ``return_confidence=True``: a list of ``Recognition``; the pass then
        also stores the log-probabilities, which ``log_prob`` needs."""
        if return_confidence:
            if images.dim() != 4 or images.shape[1] != 3:
                raise ValueError(f"expected (B,3,H,W) input, got {tuple(images.shape)}")
            x = images.to(device=self.device, dtype=torch.float32).contiguous()
            B, _, H, W = x.shape
            T = W // 4
            ws = self._workspace(B, H, W)
            lp = torch.empty((T, B, self.tokenizer.num_classes), dtype=torch.float32, device=self.device)
            am, ids, lens, blp, clp, span = self._conf_buffers(B, T)
            self.enqueue_forward_conf(x.data_ptr(), B, H, W, lp.data_ptr(), am.data_ptr(), ids.data_ptr(), lens.data_ptr(), blp.data_ptr(),
                                      clp.data_ptr(), span.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(self.device).cuda_stream)
            return self._recognitions(lp, ids, lens, clp, span)
        _, _, ids, lens = self._run(images, False, True)
        return self._ids_to_text(ids, lens)
