"""numpy restatement of the greedy CTC path with confidences (include/ocrvi.h, ``ocrvi_ctc_greedy_conf``), of the ``Recognition`` arithmetic
(``rec.make_recognitions``) and of ``pipeline.char_boxes``: one plain loop over the steps of a row, nothing shared with the library.

``MUTANTS`` are deliberate mis-statements of the per-character records; tests/test_ctcconf_cpu.py shows that each is caught by a named
case of ``cases()``, the constructed rows the GPU test feeds the kernels."""
import math

import numpy as np

MUTANTS = ("first_step", "span_end", "carry64")


def argmax_rows(lp):
    """[T,B,C] float32 -> (argmax int32 [B,T], best_lp float32 [B,T]).  Ties go to the first index; NaN entries never win; a row of
    nothing but NaN gives 0.  best_lp is the entry the argmax points at, bit for bit (the NaN itself for a NaN row)."""
    lp = np.asarray(lp, np.float32)
    T, B, C = lp.shape
    am = np.zeros((B, T), np.int32)
    best = np.empty((B, T), np.float32)
    for t in range(T):
        for b in range(B):
            row = lp[t, b]
            cand = np.flatnonzero(row > -np.inf)        # NaN compares false
            if len(cand):
                am[b, t] = cand[np.argmax(row[cand])]   # np.argmax: the first of equal maxima
            elif np.isnan(row).any() and not np.isnan(row).all():
                # nothing above -inf beside NaN entries: the kernel's lanes (entry c in lane c % 64) that saw no NaN offer their first entry
                clean = [l for l in range(min(C, 64)) if not np.isnan(row[l::64]).any()]
                am[b, t] = clean[0] if clean else 0
            best[b, t] = row[am[b, t]]
    return am, best


def _fmax(a, b):
    """fmaxf: a NaN operand is ignored unless both are."""
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a >= b else b


def collapse_conf(am, best_lp, blank, mutant=None):
    """argmax [B,T], best_lp [B,T] -> ids [B,T] (-1 padded), lens [B], char_lp float32 [B,T] (-inf padded), char_span int32 [B,T,2]
    ((-1, -1) padded)."""
    assert mutant is None or mutant in MUTANTS
    am = np.asarray(am)
    B, T = am.shape
    ids = np.full((B, T), -1, np.int32)
    lens = np.zeros(B, np.int32)
    char_lp = np.full((B, T), -np.inf, np.float32)
    span = np.full((B, T, 2), -1, np.int32)
    for b in range(B):
        k = 0
        t = 0
        while t < T:
            t1 = t
            while t1 + 1 < T and am[b, t1 + 1] == am[b, t]:
                t1 += 1
            if am[b, t] != blank:                       # t is the first step of its run: am[t] != am[t - 1]
                end = t1
                if mutant == "carry64":                 # the run forgets what it saw before a multiple of 64
                    end = min(t1, (t // 64) * 64 + 63)
                m = np.float32(best_lp[b, t])
                if mutant != "first_step":
                    for u in range(t + 1, end + 1):
                        m = _fmax(m, np.float32(best_lp[b, u]))
                ids[b, k] = am[b, t]
                char_lp[b, k] = m
                span[b, k] = (t, end - 1 if mutant == "span_end" and end > t else end)
                k += 1
            t = t1 + 1
        lens[b] = k
    return ids, lens, char_lp, span


def greedy_conf(lp, blank=0, mutant=None):
    """[T,B,C] log-probs -> dict(argmax, ids, lens, best_lp, char_lp, char_span)."""
    am, best = argmax_rows(lp)
    ids, lens, char_lp, span = collapse_conf(am, best, blank, mutant)
    return {"argmax": am, "ids": ids, "lens": lens, "best_lp": best, "char_lp": char_lp, "char_span": span}


def recognitions(id_to_token, ids, lens, char_lp, char_span, log_probs=None):
    """The ``Recognition`` arithmetic as plain tuples (text, score, char_scores, spans, log_prob), float64 on the host."""
    out = []
    for b in range(len(lens)):
        text, scores, spans = "", [], []
        for k in range(int(lens[b])):
            i = int(ids[b][k])
            if i not in id_to_token:                    # pad id 1 and anything unknown: gone from all three
                continue
            text += id_to_token[i]
            scores.append(math.exp(float(char_lp[b][k])))
            spans.append((int(char_span[b][k][0]), int(char_span[b][k][1])))
        score = math.fsum(scores) / len(scores) if scores else 0.0
        out.append((text, score, tuple(scores), tuple(spans), None if log_probs is None else float(log_probs[b])))
    return out


def char_boxes(rect, spans, rec_size=(32, 256)):
    """(x, y, w, h), [(t0, t1)] -> int32 [n, 4] page rectangles; exact rational arithmetic through Python integers."""
    x, y, w, h = (int(v) for v in rect)
    rw = max(min(int(w * (rec_size[0] / h)), rec_size[1]), 1)
    out = np.empty((len(spans), 4), np.int32)
    for i, (t0, t1) in enumerate(spans):
        c0, c1 = min(4 * t0, rw), min(4 * (t1 + 1), rw)
        x0 = min(x + c0 * w // rw, x + w - 1)
        x1 = min(x + (c1 * w + rw - 1) // rw, x + w)
        out[i] = (x0, y, max(x1 - x0, 1), h)
    return out


# ---------------------------------------------------------------------------------------------------- constructed rows
def peaked(path, C, hi=None, lo=-9.0):
    """A path of ids [T] -> [T, C] float32 rows whose argmax is the path: ``lo`` everywhere, ``hi[t]`` (default -0.25) at path[t]."""
    T = len(path)
    lp = np.full((T, C), lo, np.float32)
    hi = np.full(T, -0.25, np.float32) if hi is None else np.asarray(hi, np.float32)
    lp[np.arange(T), np.asarray(path)] = hi
    return lp


def cases(T, C, blank=0):
    """name -> [T, C] float32 rows, every constructed row the issue lists that fits T steps and C classes.  Values are plain numbers, not
    normalised: the decode reads them as they are."""
    a, b2 = (1, 2) if blank == 0 else (0, 2 if blank != 2 else 1)       # two characters; with blank != 0, id 0 is one of them
    nan = np.float32(np.nan)
    ramp = lambda n: (-0.5 - 0.01 * np.arange(n)).astype(np.float32)   # noqa: E731  distinct values, the maximum first
    out = {}
    out["all_blank"] = peaked([blank] * T, C)
    out["one_char_all_steps_max_first"] = peaked([a] * T, C, ramp(T))
    out["one_char_all_steps_max_last"] = peaked([a] * T, C, ramp(T)[::-1].copy())
    out["alternation"] = peaked([a if t % 2 == 0 else b2 for t in range(T)], C, ramp(T))      # lens = T
    out["pad_id_emitted"] = peaked([(1 if blank != 1 else a) if t % 3 == 0 else blank for t in range(T)], C)
    tie = peaked([blank] * T, C)
    tie[:, :] = -1.0                                                    # every class equal: the first index wins
    tie[::2, C - 1] = -0.5
    tie[::2, C // 2] = -0.5                                             # two equal maxima: the lower index
    out["argmax_ties"] = tie
    if T >= 3:
        out["a_blank_a"] = peaked(([a, blank, a] * T)[:T], C, ramp(T))
        mid = peaked([a] * T, C, ramp(T))
        mid[T // 2, a] = -0.125                                         # the maximum strictly inside the run
        out["one_char_max_inside"] = mid
        nr = peaked([a] * T, C, ramp(T))
        nr[1] = nan                                                     # a NaN row inside a run: argmax 0
        out["nan_inside_run"] = nr
        nb = peaked([a, blank, b2] + [blank] * (T - 3), C)
        nb[1] = nan                                                     # a NaN row between two runs
        out["nan_between_runs"] = nb
        only = peaked([blank] * T, C)
        only[:] = nan                                                   # a run of nothing but NaN (id 0: a character when blank != 0)
        out["all_nan"] = only
        part = peaked([b2] + [blank] * (T - 1), C)
        part[1:] = nan
        out["nan_run_after_char"] = part
    if T >= 65:
        path = [blank] * T
        hi = np.full(T, -0.25, np.float32)
        for t in range(60, 64):
            path[t] = a                                                 # a run ending at step 63
        path[64] = b2                                                   # one starting at 64
        hi[60:64] = [-0.4, -0.3, -0.2, -0.1]                            # maximum on the boundary step 63
        out["run_ends_63_next_starts_64"] = peaked(path, C, hi)
    if T >= 68:
        for name, peak in (("first", 62), ("boundary_63", 63), ("boundary_64", 64), ("last", 66)):
            path = [blank] * T
            hi = np.full(T, -0.25, np.float32)
            for t in range(62, 67):
                path[t] = a                                             # a run spanning 62..66
                hi[t] = -0.5 - 0.01 * (t - 62)
            hi[peak] = -0.0625
            out[f"run_62_66_max_{name}"] = peaked(path, C, hi)
    if T >= 130:
        path = [blank] * T
        hi = np.full(T, -0.25, np.float32)
        for t in range(60, 130):
            path[t] = a                                                 # crosses 64 and 128; maximum after the second boundary
            hi[t] = -0.5
        hi[129] = -0.0625
        out["run_crosses_two_boundaries"] = peaked(path, C, hi)
        nn = peaked(path, C, hi)
        nn[60:128] = nan                                                # with blank 0 and a = 1: NaN rows are id 0 = blank, a starts at 128
        out["nan_through_a_boundary"] = nn
    return out


def random_peaked(rng, T, B, C, blank=0):
    """Seeded [T,B,C] log-softmax rows whose paths hold runs of random lengths (so runs and blanks cross the pass boundaries)."""
    z = rng.normal(0, 1, (T, B, C)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, 9))
            c = blank if rng.random() < 0.4 else int(rng.integers(0, C))
            z[t:t + n, b, c] += rng.uniform(4, 9, (min(n, T - t),)).astype(np.float32)
            t += n
    m = z.max(-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)
