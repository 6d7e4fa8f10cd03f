"""Character n-gram language model for the CTC prefix beam search (include/ocrvi.h, "Character n-gram language model"): ``CharLM`` holds the
backoff table as the library's blob, scores strings on the host (``ocrvi_lm_score``) and hands ``ocrvi_ctc_beam_lm`` a per-device handle
(``ocrvi_lm_create``).  ``train_ngrams`` is the trainer, plain Python in float64; the table itself, its validation and its scoring are the
library's."""
from __future__ import annotations

import ctypes as C
import math
from collections import defaultdict
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .vocab import Tokenizer

Gram = Tuple[int, ...]


def cond_log_prob(grams: Dict[Gram, Tuple[float, float]], ctx: Sequence[int], c: int, unk_lp: float) -> float:
    """lm(c | ctx) over a dict {gram: (lp, bo)}: the header's backoff chain in float64 (what the trainer calls for the lower orders)."""
    ctx = tuple(ctx)
    acc = 0.0
    for k in range(len(ctx), -1, -1):
        h = ctx[len(ctx) - k:]
        hit = grams.get(h + (c,))
        if hit is not None:
            return acc + hit[0]
        if k >= 1 and h in grams:
            acc = acc + grams[h][1]
    return acc + unk_lp


def train_ngrams(lines: Iterable[Sequence[int]], order: int, num_classes: int, blank_id: int = 0, discount: float = 0.75):
    """Normalised absolute-discounting backoff model over id strings -> ({gram: (lp, bo)}, unk_lp), natural logs, float64.

    Every line l is read as BOS + l, BOS = ``blank_id``.  Position q of l predicts c = l[q] from the q + 1 symbols before it; for every
    k in 1..min(order - 1, q + 1) the context h = the last k of those symbols gets count(h, c) += 1.  count(h.) = sum_c count(h, c),
    S(h) = {c: count(h, c) > 0}, D = ``discount`` in (0, 1).

    * unigrams: p(c) = (count(c) + 1) / (n + num_classes - 1) for EVERY class c != blank (n = all predicted symbols), so none is missing
      (unk_lp = -log(num_classes - 1) is never used by a trained table);
    * a context h, |h| >= 1: p(c | h) = (count(h, c) - D) / count(h.) for c in S(h), stored as the lp of the gram h + c;
      bo(h) = log(D |S(h)| / count(h.)) - log(1 - sum_{c in S(h)} p_lower(c | h[1:])), stored as the bo of the gram h, where p_lower is
      exp of this model's own score with the shorter context (the orders are built bottom up).  The sum is ``math.fsum`` over S(h).  When
      S(h) is every class but the blank the last logarithm's argument is 0 and nothing ever backs off from h: bo = 0;
    * the gram (BOS) has lp 0 (it predicts nothing), a gram that never was a context has bo 0.

    Then sum_{c != blank} exp(lm(c | h)) = 1 for every context, seen or not: c in S(h) takes 1 - D |S(h)| / count(h.) in all, and exp(bo(h))
    spreads the rest over the others in proportion to p_lower."""
    if not (isinstance(order, int) and 1 <= order <= _lib.LM_MAX_ORDER):
        raise ValueError(f"order {order!r} outside 1..{_lib.LM_MAX_ORDER}")
    if not 0.0 < discount < 1.0:
        raise ValueError(f"discount {discount!r} outside (0, 1)")
    if not (2 <= num_classes <= 1024 and 0 <= blank_id < num_classes):
        raise ValueError(f"num_classes {num_classes!r} outside 2..1024 or blank {blank_id!r} outside it")
    counts: List[Dict[Gram, Dict[int, int]]] = [defaultdict(lambda: defaultdict(int)) for _ in range(order)]   # [k][h][c]
    uni = defaultdict(int)
    n = 0
    for line in lines:
        seq = (blank_id,) + tuple(int(i) for i in line)
        if any(i == blank_id or not 0 <= i < num_classes for i in seq[1:]):
            raise ValueError("a training line holds the blank or an id outside [0, num_classes)")
        for q in range(1, len(seq)):
            c = seq[q]
            uni[c] += 1
            n += 1
            for k in range(1, min(order - 1, q) + 1):
                counts[k][seq[q - k:q]][c] += 1
    unk_lp = -math.log(num_classes - 1)
    grams: Dict[Gram, Tuple[float, float]] = {}
    for c in range(num_classes):
        if c != blank_id:
            grams[(c,)] = (math.log((uni[c] + 1) / (n + num_classes - 1)), 0.0)
    for k in range(1, order):
        level = {}
        for h in sorted(counts[k]):
            foll = counts[k][h]
            tot = sum(foll.values())
            for c in sorted(foll):
                level[h + (c,)] = math.log((foll[c] - discount) / tot)
            if len(foll) == num_classes - 1:
                bo = 0.0
            else:
                seen = math.fsum(math.exp(cond_log_prob(grams, h[1:], c, unk_lp)) for c in sorted(foll))
                bo = math.log(discount * len(foll) / tot) - math.log(1.0 - seen)
            grams[h] = (grams[h][0] if h in grams else 0.0, bo)
        for g, lp in level.items():
            grams[g] = (lp, 0.0)
    return grams, unk_lp


class CharLM:
    """A backoff character n-gram table over a recogniser's class ids.  ``from_ngrams`` is the seam for tables made elsewhere, ``train``
    builds one from text lines.  Values are stored as float32 (the table's slots); ``score`` and the beam search widen them to float64."""

    def __init__(self, gram_ids: np.ndarray, gram_lens: np.ndarray, lp: np.ndarray, bo: np.ndarray, order: int, num_classes: int,
                 blank_id: int, unk_lp: float, tokenizer: Optional[Tokenizer] = None):
        self.gram_ids = np.ascontiguousarray(gram_ids, np.int32).reshape(-1, _lib.LM_MAX_ORDER)
        self.gram_lens = np.ascontiguousarray(gram_lens, np.int32)
        self.lp, self.bo = np.ascontiguousarray(lp, np.float32), np.ascontiguousarray(bo, np.float32)
        n = len(self.gram_lens)
        if not (len(self.gram_ids) == len(self.lp) == len(self.bo) == n):
            raise ValueError("gram arrays of different lengths")
        self.order, self.num_classes, self.blank_id, self.unk_lp = int(order), int(num_classes), int(blank_id), float(unk_lp)
        self.tokenizer = tokenizer
        lib = _lib.load()
        args = (_lib.C.c_void_p(self.gram_ids.ctypes.data), self.gram_lens.ctypes.data, self.lp.ctypes.data, self.bo.ctypes.data, n, self.order,
                self.num_classes, self.blank_id, self.unk_lp)
        size = C.c_size_t(0)
        _lib.check(lib.ocrvi_lm_build(*args, None, 0, C.byref(size)))                # every rejected input is a ValueError here
        buf = C.create_string_buffer(size.value)
        _lib.check(lib.ocrvi_lm_build(*args, buf, size.value, C.byref(size)))
        self.blob = buf.raw
        self._handles = {}

    # ---- construction
    @classmethod
    def from_ngrams(cls, grams, order: int, num_classes: int, blank_id: int = 0, unk_lp: Optional[float] = None,
                    tokenizer: Optional[Tokenizer] = None) -> "CharLM":
        """``grams``: {ids tuple: (lp, bo)} or an iterable of (ids, lp, bo), natural logs; ids[0] may be ``blank_id`` = begin of line.
        ``unk_lp`` (the score of a class without a unigram) defaults to -log(num_classes - 1).  ValueError for what ``ocrvi_lm_build``
        rejects."""
        items = [(k, v[0], v[1]) for k, v in grams.items()] if isinstance(grams, dict) else [tuple(g) for g in grams]
        ids = np.full((len(items), _lib.LM_MAX_ORDER), -1, np.int32)
        lens = np.zeros(len(items), np.int32)
        for i, (g, _, _) in enumerate(items):
            g = tuple(g)
            lens[i] = len(g)
            ids[i, :min(len(g), _lib.LM_MAX_ORDER)] = g[:_lib.LM_MAX_ORDER]
        if not isinstance(num_classes, int) or num_classes < 2:
            raise ValueError(f"num_classes {num_classes!r}")
        return cls(ids, lens, np.array([v[1] for v in items], np.float32), np.array([v[2] for v in items], np.float32), order, num_classes,
                   blank_id, -math.log(num_classes - 1) if unk_lp is None else unk_lp, tokenizer)

    @classmethod
    def train(cls, texts: Iterable[str], tokenizer: Optional[Tokenizer] = None, order: int = 4, discount: float = 0.75) -> "CharLM":
        """A model of ``texts`` (one line each), encoded with ``tokenizer`` (the recogniser's; characters outside it are dropped):
        ``train_ngrams`` has the definition."""
        tok = tokenizer or Tokenizer()
        grams, unk_lp = train_ngrams((tok.encode_one(t) for t in texts), order, tok.num_classes, tok.blank_id, discount)
        return cls.from_ngrams(grams, order, tok.num_classes, tok.blank_id, unk_lp, tok)

    def save(self, path) -> None:
        """A ``.npz`` of arrays only (no pickled object)."""
        np.savez(path, gram_ids=self.gram_ids, gram_lens=self.gram_lens, lp=self.lp, bo=self.bo,
                 meta=np.array([self.order, self.num_classes, self.blank_id], np.int64), unk_lp=np.array([self.unk_lp], np.float64))

    @classmethod
    def load(cls, path, tokenizer: Optional[Tokenizer] = None) -> "CharLM":
        with np.load(path, allow_pickle=False) as z:
            order, num_classes, blank_id = (int(v) for v in z["meta"])
            return cls(z["gram_ids"], z["gram_lens"], z["lp"], z["bo"], order, num_classes, blank_id, float(z["unk_lp"][0]), tokenizer)

    def __len__(self) -> int:
        return len(self.gram_lens)

    # ---- host scoring
    def _ids(self, text_or_ids) -> List[int]:
        if isinstance(text_or_ids, str):
            return (self.tokenizer or Tokenizer()).encode_one(text_or_ids)
        return [int(i) for i in text_or_ids]

    def score(self, text_or_ids, per_char: bool = False):
        """g(ids): the string's log-probability under the model, float64, through ``ocrvi_lm_score``.  A str is encoded with the model's
        tokenizer (the default alphabet if it has none).  ``per_char=True``: (g, [each character's term])."""
        ids = np.asarray(self._ids(text_or_ids), np.int32)
        total = C.c_double(0.0)
        terms = np.zeros(max(len(ids), 1), np.float64)
        _lib.check(_lib.load().ocrvi_lm_score(self.blob, len(self.blob), ids.ctypes.data, len(ids), C.byref(total),
                                              terms.ctypes.data if per_char else None))
        return (total.value, terms[:len(ids)].tolist()) if per_char else total.value

    # ---- the device
    def to(self, device) -> "CharLM":
        """Uploads the table to ``device`` (``ocrvi_lm_create``); cached per device."""
        self.handle(device)
        return self

    def handle(self, device) -> C.c_void_p:
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the beam search runs on the device: CharLM.to takes a cuda device (score() is the host path)")
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        if index not in self._handles:
            h = C.c_void_p()
            _lib.check(_lib.load().ocrvi_lm_create(index, self.blob, len(self.blob), C.byref(h)))
            self._handles[index] = h
        return self._handles[index]

    def __del__(self):
        try:
            for h in self._handles.values():
                _lib.load().ocrvi_lm_destroy(h)
            self._handles = {}
        except Exception:
            pass
