"""Float64 restatement of the CTC prefix beam search of include/ocrvi.h ("CTC prefix beam search"), in numpy / Python: ``beam`` (with the
mutants of ``MUTANTS``, each one rule of the definition broken), ``brute`` (every path collapsed and summed) and the input generators.
Nothing here touches the library."""
import itertools
import math

import numpy as np

NINF = -math.inf

# name -> the rule it breaks
MUTANTS = {
    "parent_node": "prefix identity by parent node instead of by string",
    "no_merge": "an extension that equals another entry's prefix stays a candidate of its own",
    "repeat_from_s": "the repeat extension taken from s instead of pb",
    "no_stay_pnb": "the stay candidate's own pnb' left out",
    "tie_larger": "equal totals ordered by the larger candidate index",
    "nan_kept": "a NaN input not mapped to -inf",
    "select_pnb": "selection by pnb' alone",
}


def lse(a: float, b: float) -> float:
    m = max(a, b)
    if not m > NINF:                                                    # -inf (and NaN)
        return m if m != m else NINF
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def beam(y, blank: int, W: int, gaps=None, mutant=None):
    """y [T,C] float32 -> [(prefix tuple, score)] in rank order, at most W.  ``gaps``: a list that receives, per step, the pair
    (totals of the first W+1 candidates in order, float64 array; their consecutive differences)."""
    assert mutant is None or mutant in MUTANTS
    y = np.asarray(y)
    T, C = y.shape
    cls = np.arange(C)
    # an entry: [prefix, pb, pnb, s, node, parent node]; the nodes only serve the parent_node mutant
    entries = [[(), 0.0, NINF, 0.0, 0, -1]]
    nodes = 1
    for t in range(T):
        v = y[t].astype(np.float64)
        if mutant != "nan_kept":
            v = np.where(np.isnan(v), NINF, v)
        n = len(entries)
        with np.errstate(invalid="ignore"):
            ext = np.empty((n, C))
            for i, (l, pb, pnb, s, _, _) in enumerate(entries):
                base = np.full(C, s)
                if l and mutant != "repeat_from_s":
                    base[l[-1]] = pb
                ext[i] = base + v
        ext[:, blank] = NINF
        # merge: entry i extended by last(l_j) is entry j
        merged = [NINF] * n
        if mutant != "no_merge":
            where = {e[0]: i for i, e in enumerate(entries)}
            node_at = {e[4]: i for i, e in enumerate(entries)}
            for j, e in enumerate(entries):
                if not e[0]:
                    continue
                i = node_at.get(e[5]) if mutant == "parent_node" else where.get(e[0][:-1])
                if i is not None:
                    merged[j] = float(ext[i, e[0][-1]])
                    ext[i, e[0][-1]] = NINF
        stay = []
        for j, (l, pb, pnb, s, _, _) in enumerate(entries):
            pbn = s + float(v[blank])
            own = pnb + float(v[l[-1]]) if l and mutant != "no_stay_pnb" else NINF
            pnbn = lse(own, merged[j])
            stay.append((pbn, pnbn, lse(pbn, pnbn)))
        tot = ext.copy()
        tot[:, blank] = [s[2] for s in stay]
        flat = tot.reshape(-1)
        idx = np.flatnonzero(flat > NINF)                               # (drops NaN too)
        key = flat[idx]
        if mutant == "select_pnb":
            rank = ext.copy()
            rank[:, blank] = [s[1] for s in stay]
            key = rank.reshape(-1)[idx]
        order = np.lexsort((-idx if mutant == "tie_larger" else idx, -key))
        idx = idx[order]
        if gaps is not None:
            head = flat[idx[:W + 1]]
            gaps.append((head, head[:-1] - head[1:]))
        nxt = []
        for k in idx[:W].tolist():
            i, c = divmod(k, C)
            l, _, _, _, node, _ = entries[i]
            if c == blank:
                nxt.append([l, stay[i][0], stay[i][1], stay[i][2], node, entries[i][5]])
            else:
                nxt.append([l + (c,), NINF, float(flat[k]), float(flat[k]), nodes, node])
                nodes += 1
        entries = nxt
    return [(e[0], e[3]) for e in entries]


def brute(y, blank: int):
    """{labelling tuple: log-probability over all C^T alignments}, float64."""
    y = np.asarray(y).astype(np.float64)
    T, C = y.shape
    acc = {}
    for path in itertools.product(range(C), repeat=T):
        lab = tuple(c for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1]))
        acc.setdefault(lab, []).append(float(sum(y[t, c] for t, c in enumerate(path))))
    out = {}
    for lab, xs in acc.items():
        m = max(xs)
        out[lab] = m + math.log(math.fsum(math.exp(x - m) for x in xs)) if m > NINF else NINF
    return out


def log_softmax32(x):
    x = np.asarray(x, np.float64)
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def make(seed: int, T: int, C: int, scale: float):
    return log_softmax32(np.random.default_rng(seed).normal(size=(T, C)) * scale)


def text_like(seed: int, T: int, C: int, scale: float, blank: int = 0, noise: float = 1.0):
    """A random id string laid out as a path with blank runs and repeats; scale * one-hot of the path plus noise, log-softmax."""
    rng = np.random.default_rng(seed)
    path = []
    while len(path) < T:
        path += [blank] * int(rng.integers(0, 4))
        c = int(rng.integers(0, C - 1))
        path += [c + (c >= blank)] * int(rng.integers(1, 4))
    x = rng.normal(size=(T, C)) * noise
    x[np.arange(T), path[:T]] += scale
    return log_softmax32(x)


def outputs(rows, T: int, nbest: int):
    """[(prefix, score)] per row -> the device's ids [B,nbest,T] int32, lens [B,nbest] int32, score [B,nbest] float64."""
    B = len(rows)
    ids = np.full((B, nbest, T), -1, np.int32)
    lens = np.full((B, nbest), -1, np.int32)
    score = np.full((B, nbest), NINF, np.float64)
    for b, hyps in enumerate(rows):
        for k, (l, s) in enumerate(hyps[:nbest]):
            ids[b, k, :len(l)] = l
            lens[b, k] = len(l)
            score[b, k] = s
    return ids, lens, score
