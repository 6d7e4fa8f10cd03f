"""Float64 restatement, in numpy / Python, of the character n-gram model and of the CTC prefix beam search with LM fusion as include/ocrvi.h
defines them ("Character n-gram language model", "CTC prefix beam search with LM fusion"): the table (``Table``: the blob byte for byte,
the probe, the backoff score, ``g``), the trainer (``train``), ``beam_lm`` with the mutants of ``MUTANTS`` (each one rule broken) and
``brute_lm``.  Nothing here touches the library; the acoustic half is tests/ctcbeam_ref.py's."""
import math
import struct

import numpy as np

import ctcbeam_ref as BR

NINF = -math.inf
MAX_ORDER = 6
HASH_MUL = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1

# name -> the rule it breaks
MUTANTS = {
    "no_backoff": "the backoff weight of an absent gram's context dropped",
    "ctx_not_truncated": "the context not truncated to order - 1 symbols (one more is kept)",
    "no_bos": "BOS left out of the context of a short prefix",
    "lm_on_stay": "the last character's LM term added again on every stay",
    "len_on_stay": "the length bonus counted on a stay",
    "repeat_wrong_ctx": "the repeat extension scored with the context of the prefix without its last character",
    "unk_ninf": "a missing unigram taken as -inf instead of unk_lp",
    "rank_by_s": "ranking by the acoustic total alone, the LM only in the outputs",
    "assoc": "R = s + (alpha g + beta len) instead of (s + alpha g) + beta len",
}


def f32(x) -> float:
    return float(np.float32(x))


def key(gram) -> int:
    k = len(gram)
    out = k << 60
    for j, g in enumerate(gram):
        out |= int(g) << (10 * j)
    return out


def home(k: int, log2cap: int) -> int:
    return ((k * HASH_MUL) & M64) >> (64 - log2cap)


class Table:
    """grams: a list of (ids tuple, lp, bo) in insertion order; lp / bo are rounded to float32, as the slots hold them."""

    def __init__(self, grams, order: int, num_classes: int, bos: int, unk_lp: float):
        self.order, self.C, self.bos, self.unk = order, num_classes, bos, float(unk_lp)
        self.list = [(tuple(int(i) for i in g), f32(lp), f32(bo)) for g, lp, bo in grams]
        self.grams = {g: (lp, bo) for g, lp, bo in self.list}
        assert len(self.grams) == len(self.list)
        self.log2cap = 1
        while (1 << self.log2cap) < 2 * len(self.list):
            self.log2cap += 1
        cap = 1 << self.log2cap
        self.keys, self.vals = [0] * cap, [(0.0, 0.0)] * cap
        for g, lp, bo in self.list:
            at = home(key(g), self.log2cap)
            while self.keys[at]:
                at = (at + 1) & (cap - 1)
            self.keys[at], self.vals[at] = key(g), (lp, bo)
        self.followers = {}                                              # context -> {c: lp}
        for g, lp, _ in self.list:
            self.followers.setdefault(g[:-1], {})[g[-1]] = lp
        self._rows = {}

    def blob(self) -> bytes:
        head = struct.pack("<IIiiiiQdQ", 0x4D4C434F, 1, self.order, self.C, self.bos, self.log2cap, len(self.list), self.unk, 0)
        return head + b"".join(struct.pack("<Qff", k, *v) for k, v in zip(self.keys, self.vals))

    def probe(self, k: int):
        """(lp, bo) of the slot a probe from the key's home finds, or None: the table as the device walks it."""
        at, cap = home(k, self.log2cap), 1 << self.log2cap
        while True:
            if self.keys[at] == k:
                return self.vals[at]
            if self.keys[at] == 0:
                return None
            at = (at + 1) & (cap - 1)

    def cond(self, h, c: int, mutant=None) -> float:
        """lm(c | h): the chain of the header, literally."""
        h = tuple(h)
        acc = 0.0
        for k in range(len(h), -1, -1):
            suf = h[len(h) - k:]
            hit = self.probe(key(suf + (c,))) if len(suf) < MAX_ORDER else None
            if hit is not None:
                return acc + hit[0]
            if k >= 1 and mutant != "no_backoff":
                ctx = self.probe(key(suf))
                if ctx is not None:
                    acc = acc + ctx[1]
        return acc + (NINF if mutant == "unk_ninf" else self.unk)

    def ctx(self, l, mutant=None):
        keep = self.order if mutant == "ctx_not_truncated" else self.order - 1
        full = (() if mutant == "no_bos" else (self.bos,)) + tuple(l)
        return full[len(full) - min(keep, len(full)):] if keep else ()

    def row(self, h, mutant=None):
        """lm(c | h) for every c (NaN at the blank), the same values as ``cond`` (tests/test_ctclm_cpu.py holds them together): the unigram
        level first, then each longer level's followers over it."""
        hit = self._rows.get((h, mutant))
        if hit is None:
            acc = [0.0] * (len(h) + 1)                                   # acc[k]: the weights added before level k is tried
            for k in range(len(h), 0, -1):
                ctx = self.grams.get(h[len(h) - k:]) if mutant != "no_backoff" else None
                acc[k - 1] = acc[k] + ctx[1] if ctx is not None else acc[k]
            hit = np.full(self.C, acc[0] + (NINF if mutant == "unk_ninf" else self.unk))
            for k in range(0, len(h) + 1):
                if k + 1 <= MAX_ORDER:
                    for c, lp in self.followers.get(h[len(h) - k:], {}).items():
                        hit[c] = acc[k] + lp
            hit[self.bos] = np.nan
            self._rows[(h, mutant)] = hit
        return hit

    def g(self, l, per_char=None) -> float:
        total = 0.0
        for q, c in enumerate(l):
            term = self.cond(self.ctx(l[:q]), c)
            if per_char is not None:
                per_char.append(term)
            total = total + term
        return total


def train(lines, order: int, num_classes: int, blank: int = 0, discount: float = 0.75):
    """The trainer of ``ocr_vi_invoice_amd.lm.train_ngrams``, restated from its docstring: -> ({gram: (lp, bo)} float64, unk_lp)."""
    cnt = {}
    uni = [0] * num_classes
    for line in lines:
        seq = [blank] + list(line)
        for q in range(1, len(seq)):
            uni[seq[q]] += 1
            for k in range(1, min(order - 1, q) + 1):
                d = cnt.setdefault(tuple(seq[q - k:q]), {})
                d[seq[q]] = d.get(seq[q], 0) + 1
    n = sum(uni)
    unk = -math.log(num_classes - 1)
    grams = {(c,): (math.log((uni[c] + 1) / (n + num_classes - 1)), 0.0) for c in range(num_classes) if c != blank}

    def lower(h, c):                                                    # the model so far, shorter context
        acc = 0.0
        for k in range(len(h), -1, -1):
            suf = h[len(h) - k:]
            if suf + (c,) in grams:
                return acc + grams[suf + (c,)][0]
            if k >= 1 and suf in grams:
                acc = acc + grams[suf][1]
        return acc + unk

    for k in range(1, order):
        new = {}
        for h in sorted(x for x in cnt if len(x) == k):
            tot = sum(cnt[h].values())
            for c, m in cnt[h].items():
                new[h + (c,)] = (math.log((m - discount) / tot), 0.0)
            if len(cnt[h]) == num_classes - 1:
                bo = 0.0
            else:
                bo = math.log(discount * len(cnt[h]) / tot) - math.log(1.0 - math.fsum(math.exp(lower(h[1:], c)) for c in cnt[h]))
            grams[h] = (grams.get(h, (0.0, 0.0))[0], bo)
        grams.update(new)
    return grams, unk


def beam_lm(y, blank: int, W: int, lm: Table, alpha: float, beta: float, gaps=None, mutant=None):
    """y [T,C] float32 -> [(prefix, R, s, g)] in rank order, at most W.  ``gaps`` as ``ctcbeam_ref.beam`` fills it, of the rank totals."""
    assert mutant is None or mutant in MUTANTS
    y = np.asarray(y)
    T, C = y.shape
    assert lm.C == C and lm.bos == blank
    alpha, beta = float(alpha), float(beta)

    def total(s, g, ln):
        with np.errstate(invalid="ignore"):
            if mutant == "assoc":
                return s + (alpha * g + beta * ln)
            return (s + alpha * g) + beta * ln

    entries = [[(), 0.0, NINF, 0.0, 0.0, 0]]                            # prefix, pb, pnb, s, g, len
    for t in range(T):
        v = y[t].astype(np.float64)
        v = np.where(np.isnan(v), NINF, v)
        n = len(entries)
        ext, gext = np.empty((n, C)), np.empty((n, C))
        for i, (l, pb, pnb, s, g, ln) in enumerate(entries):
            base = np.full(C, s)
            if l:
                base[l[-1]] = pb
            ext[i] = base + v
            gext[i] = g + lm.row(lm.ctx(l, mutant), mutant)
            if l and mutant == "repeat_wrong_ctx":
                gext[i, l[-1]] = g + lm.row(lm.ctx(l[:-1], mutant), mutant)[l[-1]]
        ext[:, blank] = NINF
        merged = [NINF] * n
        where = {e[0]: i for i, e in enumerate(entries)}
        for j, e in enumerate(entries):
            i = where.get(e[0][:-1]) if e[0] else None
            if i is not None:
                merged[j] = float(ext[i, e[0][-1]])
                ext[i, e[0][-1]] = NINF
        stay = []
        for j, (l, pb, pnb, s, g, ln) in enumerate(entries):
            pbn = s + float(v[blank])
            pnbn = BR.lse(pnb + float(v[l[-1]]) if l else NINF, merged[j])
            gs = g + float(lm.row(lm.ctx(l[:-1], mutant), mutant)[l[-1]]) if l and mutant == "lm_on_stay" else g
            stay.append((pbn, pnbn, BR.lse(pbn, pnbn), gs, ln + 1 if mutant == "len_on_stay" else ln))
        tot = ext.copy()
        tot[:, blank] = [s[2] for s in stay]
        gall = gext.copy()
        gall[:, blank] = [s[3] for s in stay]
        lens = np.repeat(np.array([e[5] + 1 for e in entries], np.float64)[:, None], C, 1)
        lens[:, blank] = [s[4] for s in stay]
        flat, gflat = tot.reshape(-1), gall.reshape(-1)
        idx = np.flatnonzero(flat > NINF)                               # the acoustic total decides what is a candidate
        R = total(flat[idx], gflat[idx], lens.reshape(-1)[idx])
        rank = flat[idx] if mutant == "rank_by_s" else R
        order = np.lexsort((idx, -rank))
        idx, R = idx[order], R[order]
        if gaps is not None:
            head = (flat[idx] if mutant == "rank_by_s" else R)[:W + 1]
            with np.errstate(invalid="ignore"):                       # (a mutant's -inf totals)
                gaps.append((head, head[:-1] - head[1:]))
        nxt = []
        for k in idx[:W].tolist():
            i, c = divmod(k, C)
            l = entries[i][0]
            if c == blank:
                nxt.append([l, stay[i][0], stay[i][1], stay[i][2], stay[i][3], stay[i][4]])
            else:
                nxt.append([l + (c,), NINF, float(flat[k]), float(flat[k]), float(gflat[k]), entries[i][5] + 1])
        entries = nxt
    return [(e[0], float(total(e[3], e[4], float(e[5]))), e[3], e[4]) for e in entries]


def brute_lm(y, blank: int, lm: Table, alpha: float, beta: float):
    """{labelling: (R, s, g)} over all C^T alignments: ``ctcbeam_ref.brute`` plus alpha g(l) + beta |l|."""
    out = {}
    for l, s in BR.brute(y, blank).items():
        g = lm.g(l)
        out[l] = ((s + alpha * g) + beta * len(l), s, g)
    return out


def outputs(rows, T: int, nbest: int):
    """[(prefix, R, s, g)] per row -> ids [B,nbest,T] int32, lens [B,nbest] int32 and score / ctc_score / lm_score [B,nbest] float64."""
    ids, lens, score = BR.outputs([[(h[0], h[1]) for h in r] for r in rows], T, nbest)
    ctc, lms = np.full(score.shape, NINF), np.full(score.shape, NINF)
    for b, hyps in enumerate(rows):
        for k, h in enumerate(hyps[:nbest]):
            ctc[b, k], lms[b, k] = h[2], h[3]
    return ids, lens, score, ctc, lms


# ---------------------------------------------------------------------------------------------------- tables and lines for the cases
def random_table(seed: int, order: int, C: int, blank: int, per_level: int = 0, keep: float = 0.7, unigrams: float = 1.0):
    """A table that is no probability model: lp in (-3, 0), bo in (-1, 0.5) on every level, the top one included.  ``per_level`` = 0: every
    possible gram with probability ``keep`` (small C); otherwise that many random grams per level above the unigrams."""
    rng = np.random.default_rng(seed)
    labels = [c for c in range(C) if c != blank]
    grams = {}
    for c in labels:
        if rng.random() < unigrams:
            grams[(c,)] = None
    if order > 1:
        grams[(blank,)] = None
    for k in range(2, order + 1):
        if per_level:
            for _ in range(per_level):
                g = tuple(int(x) for x in rng.choice(labels, k))
                grams[((blank,) + g[1:]) if rng.random() < 0.25 else g] = None
        else:
            firsts = labels + [blank]
            for first in firsts:
                for rest in np.ndindex(*([len(labels)] * (k - 1))):
                    if rng.random() < keep:
                        grams[(first,) + tuple(labels[r] for r in rest)] = None
    out = []
    for g in grams:
        lp = 0.0 if g == (blank,) else -3.0 * rng.random()
        out.append((g, lp, 1.5 * rng.random() - 1.0))
    return Table(out, order, C, blank, -4.0 - rng.random())


WORDS = ("hoá đơn giá trị gia tăng công ty cổ phần trách nhiệm hữu hạn địa chỉ số tài khoản mã thuế người mua bán hàng ngày tháng năm "
         "đơn vị tính lượng thành tiền tổng cộng chiết khấu thanh toán chuyển khoản ngân ký ghi rõ họ tên điện thoại quận phường thành phố "
         "Hà Nội Hồ Chí Minh Đà Nẵng VND 0 1 2 3 4 5 6 7 8 9 10 2024 % .").split()


def synthetic_lines(seed: int, n: int):
    rng = np.random.default_rng(seed)
    return [" ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), int(rng.integers(2, 8)))) for _ in range(n)]
