"""float64 / integer restatements of the validation arithmetic that include/ocrvi.h states for ``ocrvi_det_eval``, ``ocrvi_ctc_loss`` and
``ocrvi_edit_distance``, written from the header's text (numpy, no library code).  The GPU tests compare the kernels with these; the
CPU tests compare these with goldens the reference's own modules produced (tests/golden/make_eval_golden.py).

The ``*_torch`` functions at the end are the same arithmetic in torch ops on whatever device the inputs live on: the context column of
tools/eval_bench.py."""
from functools import lru_cache

import numpy as np

EPS = 1e-6


# ---------------------------------------------------------------------------------------------- detection
def det_eval(binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask, negative_ratio=3.0):
    """The record of ``ocrvi_det_eval``: counts from the float32 products and comparisons the header states, sums in float64 from the
    float32 inputs (every term evaluated in float64)."""
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1)   # noqa: E731
    b, t, tb, x, g, m, tm, tk = (f32(a) for a in (binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask))
    gm = g * m                                        # float32 products, as the counts need them
    ngm = (np.float32(1) - g) * m
    p = (np.trunc(gm).astype(np.int64) & 255)         # .byte()
    q = (np.trunc(ngm).astype(np.int64) & 255)
    P = (b > np.float32(0.5)).astype(np.float32) * m
    rec = {
        "tp": int(np.sum((P == 1) & (gm == 1))),
        "fp": int(np.sum((P == 1) & (gm == 0))),
        "fn": int(np.sum((P == 0) & (gm == 1))),
        "positive_count": int(p.sum()),
        "negatives": int(q.sum()),
    }
    want = np.trunc(float(rec["positive_count"]) * float(negative_ratio))
    k = int(min(rec["negatives"], int(want))) if want >= 1 else 0
    rec["negative_count"] = k
    d = lambda a: a.astype(np.float64)                # noqa: E731
    x64, g64, m64 = d(x), d(g), d(m)
    loss = np.maximum(x64, 0) - x64 * g64 + np.log1p(np.exp(-np.abs(x64)))
    rec["pos_bce"] = float(np.sum(loss * p))
    neg = np.sort(loss * q)[::-1]
    rec["topk_bce"] = float(np.sum(neg[:k])) if k else 0.0
    rec["dice_inter"] = float(np.sum(d(tb) * g64 * m64))
    rec["pred_mask"] = float(np.sum(d(tb) * m64))
    rec["gt_mask"] = float(np.sum(g64 * m64))
    rec["l1_num"] = float(np.sum(np.abs(d(t) - d(tm)) * d(tk)))
    rec["thresh_mask"] = float(np.sum(d(tk)))
    return rec


def db_loss(rec, alpha=5.0, beta=10.0):
    """loss, l_prob, l_binary, l_thresh from a record (the divisions the header lists under the record)."""
    l_prob = (rec["pos_bce"] + rec["topk_bce"]) / (rec["positive_count"] + rec["negative_count"] + EPS)
    l_binary = 1.0 - 2.0 * rec["dice_inter"] / (rec["pred_mask"] + rec["gt_mask"] + EPS)
    l_thresh = rec["l1_num"] / (rec["thresh_mask"] + EPS)
    return {"loss": l_prob + alpha * l_binary + beta * l_thresh, "l_prob": l_prob, "l_binary": l_binary, "l_thresh": l_thresh}


def metrics(tp, fp, fn):
    """Precision, recall, F1, IoU, dice from the three counts: float32 throughout, eps 1e-6."""
    f = np.float32
    tp, fp, fn, eps = f(tp), f(fp), f(fn), f(EPS)
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    return {"precision": float(precision), "recall": float(recall),
            "f1": float(f(2) * precision * recall / (precision + recall + eps)),
            "iou": float(tp / (tp + fp + fn + eps)),
            "dice": float(f(2) * tp / (f(2) * tp + fp + fn + eps))}


# ---------------------------------------------------------------------------------------------- CTC
def ctc_nll(log_probs, targets, target_lengths, input_lengths=None, blank=0):
    """Negative log-likelihood per sequence by the textbook alpha recursion (Graves et al. 2006, eq. 6-8) in float64 log space, one
    numpy row of states per step.  log_probs [T,B,C]; targets [B,Lmax]; +inf where no alignment exists."""
    y = np.asarray(log_probs, np.float64)
    T, B, _ = y.shape
    out = np.empty(B, np.float64)
    for b in range(B):
        L = int(target_lengths[b])
        Tb = T if input_lengths is None else int(input_lengths[b])
        ext = np.full(2 * L + 1, blank, np.int64)
        ext[1::2] = np.asarray(targets)[b, :L]
        S = len(ext)
        if Tb == 0:
            out[b] = 0.0 if L == 0 else np.inf
            continue
        skip = np.zeros(S, bool)                       # s - 2 -> s: only between two different labels
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        alpha = np.full(S, -np.inf)
        alpha[:2] = y[0, b, ext[:2]]
        with np.errstate(invalid="ignore"):
            for t in range(1, Tb):
                stay_or_step = np.logaddexp(alpha, np.concatenate(([-np.inf], alpha[:-1])))
                two = np.where(skip, np.concatenate(([-np.inf, -np.inf], alpha[:-2])), -np.inf)
                alpha = np.logaddexp(stay_or_step, two) + y[t, b, ext]
            out[b] = -np.logaddexp(alpha[S - 1], alpha[S - 2] if S > 1 else -np.inf)
    return out


def ctc_loss(nll, target_lengths, reduction="mean", zero_infinity=True):
    """nn.CTCLoss' treatment of the per-sequence values: zero_infinity, then 'mean' = mean over the batch of nll / max(L, 1)."""
    nll = np.array(nll, np.float64)
    if zero_infinity:
        nll[np.isinf(nll)] = 0.0
    if reduction == "mean":
        return float(np.mean(nll / np.maximum(np.asarray(target_lengths, np.float64), 1)))
    return float(nll.sum()) if reduction == "sum" else nll


# ---------------------------------------------------------------------------------------------- Levenshtein
def levenshtein(a, b):
    """Unit-cost edit distance of two sequences by the plain (len(a)+1) x (len(b)+1) table."""
    a, b = list(a), list(b)
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def levenshtein_recursive(a, b):
    """The definition itself, for tiny sequences: lev(a, b) = |a| if b is empty, |b| if a is empty, lev(tails) when the heads match, else
    1 + min(lev(tail a, b), lev(a, tail b), lev(tail a, tail b))."""
    a, b = tuple(a), tuple(b)

    @lru_cache(maxsize=None)
    def lev(i, j):
        if i == len(a):
            return len(b) - j
        if j == len(b):
            return len(a) - i
        if a[i] == b[j]:
            return lev(i + 1, j + 1)
        return 1 + min(lev(i + 1, j), lev(i, j + 1), lev(i + 1, j + 1))

    return lev(0, 0)


def edit_distance(pred_ids, pred_lens, gt_ids, gt_lens):
    """``ocrvi_edit_distance``: per row, the first pred_lens[b] prediction ids with ids < 2 dropped against the first gt_lens[b] ground-truth
    ids."""
    out = []
    for b in range(len(pred_lens)):
        p = [int(v) for v in np.asarray(pred_ids)[b, :int(pred_lens[b])] if v >= 2] if int(pred_lens[b]) else []
        g = [int(v) for v in np.asarray(gt_ids)[b, :int(gt_lens[b])]] if int(gt_lens[b]) else []
        out.append(levenshtein(p, g))
    return np.array(out, np.int32)


def encode_text(text, token_to_id):
    """A ground-truth string as ids: -2 for a character outside the alphabet."""
    return [token_to_id.get(c, -2) for c in text]


def cer(pred_strings, gt_strings):
    """compute_cer on strings: summed distances over summed ground-truth lengths (at least 1)."""
    errors = sum(levenshtein(p, g) for p, g in zip(pred_strings, gt_strings))
    return errors / max(sum(len(g) for _, g in zip(pred_strings, gt_strings)), 1)


def acc(pred_strings, gt_strings):
    return sum(1 for p, g in zip(pred_strings, gt_strings) if p == g) / max(len(pred_strings), 1)


# ---------------------------------------------------------------------------------------------- the same arithmetic in torch ops
def det_eval_torch(binary, thresh, thresh_binary, bin_logits, gt, mask, thresh_map, thresh_mask, negative_ratio=3.0):
    """``det_eval`` above in torch ops on the inputs' device (float32 terms, float64 sums, torch.topk for the k largest)."""
    import torch
    gm, ngm = gt * mask, (1 - gt) * mask
    p, q = gm.to(torch.uint8), ngm.to(torch.uint8)
    P = (binary > 0.5).float() * mask
    rec = {"tp": ((P == 1) & (gm == 1)).sum(), "fp": ((P == 1) & (gm == 0)).sum(), "fn": ((P == 0) & (gm == 1)).sum()}
    pos, neg = int(p.sum(dtype=torch.int64)), int(q.sum(dtype=torch.int64))
    k = min(neg, int(pos * negative_ratio))
    loss = torch.clamp_min(bin_logits, 0) - bin_logits * gt + torch.log1p(torch.exp(-bin_logits.abs()))
    top = torch.topk((loss * q.float()).view(-1), k).values
    rec.update(positive_count=pos, negatives=neg, negative_count=k,
               pos_bce=(loss * p.float()).sum(dtype=torch.float64), topk_bce=top.sum(dtype=torch.float64),
               dice_inter=(thresh_binary * gt * mask).sum(dtype=torch.float64), pred_mask=(thresh_binary * mask).sum(dtype=torch.float64),
               gt_mask=gm.sum(dtype=torch.float64), l1_num=((thresh - thresh_map).abs() * thresh_mask).sum(dtype=torch.float64),
               thresh_mask=thresh_mask.sum(dtype=torch.float64))
    return {k_: (float(v) if k_ in ("pos_bce", "topk_bce", "dice_inter", "pred_mask", "gt_mask", "l1_num", "thresh_mask") else int(v))
            for k_, v in rec.items()}


def ctc_nll_torch(log_probs, targets, target_lengths, input_lengths=None, blank=0):
    """``ctc_nll`` above in torch ops, all sequences at once: float64 alpha [B,S] stepped over t with torch.logsumexp."""
    import torch
    T, B, _ = log_probs.shape
    dev = log_probs.device
    tl = target_lengths.to(dev).long()
    il = torch.full((B,), T, device=dev, dtype=torch.long) if input_lengths is None else input_lengths.to(dev).long()
    Lmax = targets.shape[1]
    S = 2 * Lmax + 1
    ext = torch.full((B, S), blank, device=dev, dtype=torch.long)
    ext[:, 1::2] = targets.to(dev).long().clamp_min(0)
    valid = torch.arange(S, device=dev)[None, :] < (2 * tl + 1)[:, None]
    skip = torch.zeros((B, S), dtype=torch.bool, device=dev)
    skip[:, 2:] = (ext[:, 2:] != blank) & (ext[:, 2:] != ext[:, :-2])
    y = log_probs.double().permute(1, 0, 2)                       # [B,T,C]
    ninf = torch.full((B, S), -float("inf"), device=dev, dtype=torch.float64)
    alpha = ninf.clone()
    e0 = y[:, 0].gather(1, ext)
    alpha[:, :2] = e0[:, :2]
    alpha = torch.where(valid, alpha, ninf)
    for t in range(1, T):
        a1 = torch.cat([ninf[:, :1], alpha[:, :-1]], 1)
        a2 = torch.where(skip, torch.cat([ninf[:, :2], alpha[:, :-2]], 1), ninf)
        new = torch.logsumexp(torch.stack([alpha, a1, a2], 0), 0) + y[:, t].gather(1, ext)
        new = torch.where(valid, new, ninf)
        alpha = torch.where((t < il)[:, None], new, alpha)
    last = (2 * tl)[:, None]
    end = torch.logsumexp(torch.cat([alpha.gather(1, last), torch.where(tl[:, None] > 0, alpha.gather(1, (last - 1).clamp_min(0)), ninf[:, :1])], 1), 1)
    return -end


def edit_distance_torch(pred_ids, pred_lens, gt_ids, gt_lens):
    """``edit_distance`` above in torch ops, all pairs at once: one DP row [B,G+1] per prediction column, the insertion chain as a
    cumulative minimum.  A dropped prediction id (< 2, or beyond its row's length) leaves the row unchanged."""
    import torch
    B, T = pred_ids.shape
    G = gt_ids.shape[1]
    dev = pred_ids.device
    j = torch.arange(G + 1, device=dev)[None, :]
    row = j.expand(B, G + 1).clone()
    for i in range(T):
        p = pred_ids[:, i:i + 1]
        live = (p >= 2) & (i < pred_lens[:, None])
        t = torch.minimum(row[:, 1:] + 1, row[:, :-1] + (gt_ids != p).to(row.dtype))
        t = torch.cat([row[:, :1] + 1, t], 1)
        new = torch.cummin(t - j, 1).values + j
        row = torch.where(live, new, row)
    return row.gather(1, gt_lens[:, None].long()).squeeze(1).to(torch.int32)
