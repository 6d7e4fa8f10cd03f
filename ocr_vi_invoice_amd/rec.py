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


class Hypothesis(NamedTuple):
    """One reading of a line from the CTC prefix beam search (``beam=W``; include/ocrvi.h, ``ocrvi_ctc_beam``).  ``log_prob`` is the device's
    ``score``: the log-probability of the id string ``ids`` over the alignments the beam kept, a lower bound of its full probability
    (``-ocrvi_ctc_loss``) and equal to it when nothing that leads to the string was ever pruned.  ``text`` is ``Tokenizer.decode`` of
    ``ids``."""
    text: str
    log_prob: float
    ids: Tuple[int, ...]


def make_hypotheses(tokenizer: Tokenizer, ids, lens, score) -> List[List[Hypothesis]]:
    """Host half of the beam search: the device's ``ids`` [B,nbest,T] / ``lens`` [B,nbest] / ``score`` [B,nbest] on the host -> one list
    of ``Hypothesis`` per row, best first.  A missing hypothesis (``lens`` -1) is dropped, so a list may be shorter than nbest or empty.
    Two id strings that ``Tokenizer.decode`` maps to one text (they differ in pad id 1 only, which decode drops) stay two hypotheses:
    their probabilities are not added."""
    ids, lens, score = np.asarray(ids), np.asarray(lens), np.asarray(score)
    # only the valid ids become Python objects: one flat list, cut by the lengths
    flat = ids[np.arange(ids.shape[2]) < lens[..., None]].tolist()
    tokens = tokenizer.id_to_token
    out, at = [], 0
    for row_lens, row_score in zip(lens.tolist(), score.tolist()):
        hyps = []
        for n, s in zip(row_lens, row_score):
            if n >= 0:
                r = flat[at:at + n]
                at += n
                hyps.append(Hypothesis("".join([tokens[i] for i in r if i in tokens]), s, tuple(r)))
        out.append(hyps)
    return out


class LMHypothesis(NamedTuple):
    """One reading of a line from the beam search with a language model fused in (``beam=W, lm=...``; include/ocrvi.h,
    ``ocrvi_ctc_beam_lm``).  ``score`` is the rank total the search ordered by, ``(log_prob + lm_weight * lm_log_prob) + len_bonus *
    len(ids)``; ``log_prob`` is the acoustic part, what ``Hypothesis.log_prob`` is (a lower bound of ``-ocrvi_ctc_loss``); ``lm_log_prob``
    is the model's score of ``ids`` (``CharLM.score``)."""
    text: str
    score: float
    ids: Tuple[int, ...]
    log_prob: float
    lm_log_prob: float


def make_lm_hypotheses(tokenizer: Tokenizer, ids, lens, score, ctc_score, lm_score) -> List[List[LMHypothesis]]:
    """``make_hypotheses`` for the five outputs of ``ocrvi_ctc_beam_lm``."""
    ctc, lms = np.asarray(ctc_score).tolist(), np.asarray(lm_score).tolist()
    out = []
    for b, row in enumerate(make_hypotheses(tokenizer, ids, lens, score)):
        out.append([LMHypothesis(h.text, h.log_prob, h.ids, ctc[b][k], lms[b][k]) for k, h in enumerate(row)])
    return out


def check_lm(lm, lm_weight, len_bonus, beam, num_classes: Optional[int] = None, blank_id: Optional[int] = None) -> None:
    """The ``ValueError`` cases of ``lm=...`` (a no-op for ``lm=None`` with the default weights), raised before any device work."""
    if lm is None:
        if lm_weight != 1.0 or len_bonus != 0.0:
            raise ValueError("lm_weight / len_bonus without lm")
        return
    if beam is None:
        raise ValueError("lm without beam: the language model is fused into the beam search (beam=W)")
    from .lm import CharLM
    if not isinstance(lm, CharLM):
        raise ValueError(f"lm must be a CharLM, got {type(lm).__name__}")
    ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in (lm_weight, len_bonus))
    if not ok or lm_weight < 0:
        raise ValueError(f"lm_weight {lm_weight!r}, len_bonus {len_bonus!r}: need finite numbers, lm_weight >= 0")
    if num_classes is not None and lm.num_classes != num_classes:
        raise ValueError(f"the language model has {lm.num_classes} classes, the recogniser {num_classes}")
    if blank_id is not None and lm.blank_id != blank_id:
        raise ValueError(f"the language model's begin-of-line id {lm.blank_id} is not the recogniser's blank {blank_id}")


def first_matching(hyps: Sequence[Hypothesis], accept) -> Optional[Hypothesis]:
    """The first hypothesis whose text ``accept`` takes (a callable, or a compiled pattern: its ``fullmatch``), else ``hyps[0]``, else
    ``None``.  The invoice use: ``first_matching(hyps, re.compile(r"\\d{10}(-\\d{3})?"))`` for a tax code, or a checksum function."""
    ok = accept.fullmatch if hasattr(accept, "fullmatch") else accept
    return next((h for h in hyps if ok(h.text)), hyps[0] if hyps else None)


def check_beam(beam, nbest, T: Optional[int] = None, return_confidence: bool = False) -> None:
    """The ``ValueError`` cases of ``beam=W`` (a no-op for ``beam=None``), raised before any device work."""
    if beam is None:
        return
    if return_confidence:
        raise ValueError("beam together with return_confidence=True: the confidences are defined on the greedy path")
    if not (isinstance(beam, int) and isinstance(nbest, int)) or not 1 <= beam <= _lib.CTC_BEAM_MAX or not 1 <= nbest <= beam:
        raise ValueError(f"beam {beam!r}, nbest {nbest!r}: need integers with 1 <= nbest <= beam <= {_lib.CTC_BEAM_MAX}")
    if T is not None and T > _lib.CTC_BEAM_MAX_T:
        raise ValueError(f"beam search takes at most T = {_lib.CTC_BEAM_MAX_T} steps, got {T}")


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

    def beam_workspace_bytes(self, T: int, B: int, beam: int, num_classes: Optional[int] = None) -> int:
        n = _lib.C.c_size_t(0)
        _lib.check(_lib.load().ocrvi_ctc_beam_workspace_bytes(T, B, num_classes or self.tokenizer.num_classes, beam, _lib.C.byref(n)))
        return int(n.value)

    def enqueue_beam(self, log_probs, T, B, beam, nbest, ids, lens, score, ws, ws_bytes, stream, num_classes: Optional[int] = None) -> None:
        """``ocrvi_ctc_beam`` on log_probs [T,B,C], enqueue-only: raw device pointers, sizes and a stream.  C is the model's class count
        unless ``num_classes`` says otherwise (``decode_probs`` takes it from the tensor, as the greedy decode does)."""
        _lib.check(_lib.load().ocrvi_ctc_beam(self._dev_index(), log_probs, T, B, num_classes or self.tokenizer.num_classes, self.blank_id,
                                              beam, nbest, ids, lens, score, ws, ws_bytes, stream))

    def beam_lm_workspace_bytes(self, T: int, B: int, beam: int, num_classes: Optional[int] = None) -> int:
        n = _lib.C.c_size_t(0)
        _lib.check(_lib.load().ocrvi_ctc_beam_lm_workspace_bytes(T, B, num_classes or self.tokenizer.num_classes, beam, _lib.C.byref(n)))
        return int(n.value)

    def enqueue_beam_lm(self, log_probs, T, B, beam, nbest, lm, lm_weight, len_bonus, ids, lens, score, ctc_score, lm_score, ws, ws_bytes, stream,
                        num_classes: Optional[int] = None) -> None:
        """``ocrvi_ctc_beam_lm``, enqueue-only like ``enqueue_beam``; ``lm`` a ``CharLM`` (its handle on this device is made on first use,
        which uploads the table: do that before a graph capture with ``lm.to(device)``)."""
        _lib.check(_lib.load().ocrvi_ctc_beam_lm(self._dev_index(), log_probs, T, B, num_classes or self.tokenizer.num_classes, self.blank_id,
                                                 beam, nbest, lm.handle(self.device), float(lm_weight), float(len_bonus), ids, lens, score,
                                                 ctc_score, lm_score, ws, ws_bytes, stream))

    def _beam_search(self, T: int, B: int, beam: int, nbest: int, lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0,
                     num_classes: Optional[int] = None):
        """What tells the two searches apart, for ``_beam_hypotheses`` and the engine: (the workspace bytes, the outputs' (shape, dtype),
        ``enqueue(log_probs, outputs, ws, ws_bytes, stream)``, the ``make_*hypotheses`` that reads the outputs).  ``enqueue`` takes raw
        device pointers, ``outputs`` a list of them in the order of the shapes: ids, lens, score (with ``lm``: ctc_score, lm_score)."""
        row = ((B, nbest), torch.float64)
        outputs = (((B, nbest, T), torch.int32), ((B, nbest), torch.int32), row)                     # ids, lens, score
        if lm is None:
            return (self.beam_workspace_bytes(T, B, beam, num_classes), outputs,
                    lambda lp, outs, *ws: self.enqueue_beam(lp, T, B, beam, nbest, *outs, *ws, num_classes), make_hypotheses)
        return (self.beam_lm_workspace_bytes(T, B, beam, num_classes), outputs + (row, row),         # ctc_score, lm_score
                lambda lp, outs, *ws: self.enqueue_beam_lm(lp, T, B, beam, nbest, lm, lm_weight, len_bonus, *outs, *ws, num_classes),
                make_lm_hypotheses)

    def _beam_hypotheses(self, lp: torch.Tensor, beam: int, nbest: int, lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
        T, B, Cn = lp.shape
        ws_bytes, outputs, enqueue, make = self._beam_search(T, B, beam, nbest, lm, lm_weight, len_bonus, Cn)
        outs = [torch.empty(sh, dtype=dt, device=self.device) for sh, dt in outputs]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        enqueue(lp.data_ptr(), [t.data_ptr() for t in outs], ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        rows = [t.cpu().numpy() for t in outs]
        self.check_range()      # (the copies above synchronised the stream already)
        return make(self.tokenizer, *rows)

    def decode_probs(self, log_probs: torch.Tensor, return_confidence: bool = False, beam: Optional[int] = None, nbest: int = 1,
                     lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
        """Greedy CTC decode of (T,B,C) log-probs (svtrv2.py:545-569): argmax, collapse repeats, drop blank on the
        device; id -> text (dropping pad id 1, tokenizer.py:73) on the host.  ``return_confidence=True``: a list of ``Recognition``
        (``ocrvi_ctc_greedy_conf``) whose ``text`` are the strings returned otherwise.
        ``beam=W``: the prefix beam search instead (``ocrvi_ctc_beam``): one list of ``Hypothesis`` per row, best first, at most ``nbest``
        long, possibly empty.  ValueError, before any device work, for ``beam`` outside 1..64, ``nbest`` outside 1..beam, T > 1024 and
        ``beam`` together with ``return_confidence=True``.
        ``lm=CharLM`` (with ``beam``): the search ranks by ``(log_prob + lm_weight * lm(ids)) + len_bonus * len(ids)``
        (``ocrvi_ctc_beam_lm``) and the lists hold ``LMHypothesis``.  ValueError, before any device work, for ``lm`` without ``beam``, a
        model whose class count or blank is not this tensor's / this recogniser's, and weights that are not finite or ``lm_weight < 0``."""
        check_beam(beam, nbest, log_probs.shape[0], return_confidence)
        check_lm(lm, lm_weight, len_bonus, beam, log_probs.shape[2], self.blank_id)
        lp = log_probs.to(device=self.device, dtype=torch.float32).contiguous()
        T, B, Cn = lp.shape
        if beam is not None:
            return self._beam_hypotheses(lp, beam, nbest, lm, lm_weight, len_bonus)
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

    def _run_conf(self, images: torch.Tensor):
        """``ocrvi_rec_forward_conf`` with the log-probabilities stored -> (lp, ids, lens, char_lp, char_span) on the device."""
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
        return lp, ids, lens, clp, span

    def decode_greedy_and_beam(self, images: torch.Tensor, beam: int, nbest: int = 1, return_confidence: bool = False,
                               lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
        """One forward, both decodes: (what ``decode_greedy(images, return_confidence)`` returns, what ``decode_greedy(images, beam=beam,
        nbest=nbest)`` returns).  The greedy half comes from the same entry as without ``beam``; the pass also stores the
        log-probabilities, which the beam search reads.  ``lm``, ``lm_weight``, ``len_bonus`` as ``decode_probs`` takes them."""
        check_beam(beam, nbest, images.shape[-1] // 4 if images.dim() == 4 else None)
        check_lm(lm, lm_weight, len_bonus, beam, self.tokenizer.num_classes, self.blank_id)
        if return_confidence:
            lp, ids, lens, clp, span = self._run_conf(images)
            greedy = self._recognitions(lp, ids, lens, clp, span)
        else:
            lp, _, ids, lens = self._run(images, True, True)
            greedy = self._ids_to_text(ids, lens)
        return greedy, self._beam_hypotheses(lp, beam, nbest, lm, lm_weight, len_bonus)

    def decode_greedy(self, images: torch.Tensor, return_confidence: bool = False, beam: Optional[int] = None, nbest: int = 1,
                      lm=None, lm_weight: float = 1.0, len_bonus: float = 0.0):
        """forward + decode in one device pass (svtrv2.py:538-543).  ``return_confidence=True``: a list of ``Recognition``; the pass then
        also stores the log-probabilities, which ``log_prob`` needs.  ``beam=W``: the forward, then the prefix beam search on its
        log-probabilities: lists of ``Hypothesis`` as ``decode_probs(..., beam=W, nbest=nbest)`` returns them (of ``LMHypothesis`` with
        ``lm``)."""
        check_beam(beam, nbest, images.shape[-1] // 4 if images.dim() == 4 else None, return_confidence)
        check_lm(lm, lm_weight, len_bonus, beam, self.tokenizer.num_classes, self.blank_id)
        if beam is not None:
            return self._beam_hypotheses(self._run(images, True, False)[0], beam, nbest, lm, lm_weight, len_bonus)
        if return_confidence:
            return self._recognitions(*self._run_conf(images))
        _, _, ids, lens = self._run(images, False, True)
        return self._ids_to_text(ids, lens)
