"""The shared case list of the LM-fused beam search tests: ``table(name)`` (a ``ctclm_ref.Table``, built once), ``CASES`` = [(name, y [T,B,C] float32,
blank, W, nbest, table name, alpha, beta)], the smallest shapes at which the kernel can go wrong, and ``reference(name)``, computed once
per process with tests/ctclm_ref.py and never changed.  ``EXACT`` names the cases the separation condition does not apply to (exact ties by
construction, or at most one finite candidate)."""
import functools

import numpy as np

import ctcbeam_cases as CC
import ctcbeam_ref as BR
import ctclm_ref as LR

from ocr_vi_invoice_amd.vocab import Tokenizer

NINF = -np.inf
TOK = Tokenizer()


def _colliding_table():
    """Eight bigrams and unigrams of C = 40 (blank 39) in 16 slots whose homes are all slot 14: the probe chain wraps round the end."""
    grams = []
    for a in range(39):
        for b in (None, *range(39)):
            g = (a,) if b is None else (a, b)
            if LR.home(LR.key(g), 4) == 14 and len(grams) < 8:
                grams.append((g, -0.25 * (len(grams) + 1), -0.125 * (len(grams) + 1)))
    assert len(grams) == 8
    return LR.Table(grams, 2, 40, 39, -5.0)


def _trained(order):
    grams, unk = LR.train([TOK.encode_one(t) for t in LR.synthetic_lines(7, 300)], order, TOK.num_classes, TOK.blank_id, 0.75)
    return LR.Table([(g, lp, bo) for g, (lp, bo) in grams.items()], order, TOK.num_classes, TOK.blank_id, unk)


def _order6_wide():
    """Order 6 over C = 1024 with the ids 0 (BOS), 1 and 1023 in every position of a 6-gram, beside random grams."""
    t = LR.random_table(61, 6, 1024, 0, per_level=400)
    grams = list(t.list)
    have = {g for g, _, _ in grams}
    rng = np.random.default_rng(62)
    for pos in range(6):
        for v in (1, 1023) + ((0,) if pos == 0 else ()):
            for k in range(pos + 1, 7):
                g = [int(x) for x in rng.integers(1, 1024, k)]
                g[pos] = v
                if tuple(g) not in have:
                    have.add(tuple(g))
                    grams.append((tuple(g), -3.0 * rng.random(), rng.random() - 1.0))
    return LR.Table(grams, 6, 1024, 0, -7.5)


def _tie_table():
    """Order 1 over C = 8, blank 3, dyadic lp: no logarithm and no rounding anywhere in R."""
    lp = {0: -1.0, 1: -0.5, 2: 0.5, 4: -2.0, 5: -0.5, 6: 1.0, 7: -0.5}
    return LR.Table([((c,), v, 0.0) for c, v in lp.items()], 1, 8, 3, -8.0)


@functools.lru_cache(maxsize=None)
def table(name: str) -> LR.Table:
    make = {
        "hand3_o1": lambda: LR.random_table(41, 1, 3, 0), "hand3_o2": lambda: LR.random_table(42, 2, 3, 0),
        "hand3_o3": lambda: LR.random_table(43, 3, 3, 0), "hand3_o2_blank2": lambda: LR.random_table(44, 2, 3, 2),
        "rand4_o3": lambda: LR.random_table(45, 3, 4, 0), "rand5_o3": lambda: LR.random_table(46, 3, 5, 0),
        "rand6_o3": lambda: LR.random_table(47, 3, 6, 0),
        "unk5_o2": lambda: LR.random_table(48, 2, 5, 0, unigrams=0.5),
        "rand2_o3": lambda: LR.random_table(49, 3, 2, 0, keep=1.0), "rand8_o4": lambda: LR.random_table(50, 4, 8, 0, per_level=300),
        "rand40_o3": lambda: LR.random_table(51, 3, 40, 0, per_level=1500),
        "rand40_o3_blank39": lambda: LR.random_table(52, 3, 40, 39, per_level=1500),
        "collide40": _colliding_table, "trained_o4": lambda: _trained(4), "trained_o2": lambda: _trained(2),
        "order6_C1024": _order6_wide, "tie8": _tie_table,
        "assoc8": lambda: LR.Table([((c,), 1.0 if c in (2, 6) else -1.0, 0.0) for c in range(8) if c != 3], 1, 8, 3, -8.0),
        # a bigram table that likes 2 at the line start and 2 after 2, and dislikes 1 there
        "decide": lambda: LR.Table([((c,), -1.5, 0.0) for c in (1, 2, 3)] + [((0,), 0.0, -0.5), ((0, 2), -0.25, 0.0), ((2, 2), -0.25, 0.0),
                                                                              ((0, 1), -3.0, 0.0), ((1, 1), -3.0, 0.0), ((1, 2), -3.0, 0.0),
                                                                              ((2, 1), -3.0, 0.0)], 2, 4, 0, -6.0),
    }
    return make[name]()


def _one(y):
    return np.ascontiguousarray(np.asarray(y, np.float32)[:, None, :])


def _decide_rows():
    """Classes 1 and 2 within 1e-3 at step 0 and at step 2 (1 a little ahead both times); blank at steps 1 and 3.  Acoustically (1, 1)
    leads (2, 2) by 1.8e-3; the table gives (2, 2) -0.5 and (1, 1) -6."""
    y = (-9.0 - 0.37 * np.arange(4)[None, :] - 0.11 * np.arange(4)[:, None]).astype(np.float32)
    y[0, 1], y[0, 2] = -0.6931, -0.6940
    y[1, 0] = -0.001
    y[2, 1], y[2, 2] = -0.6931, -0.6940
    y[3, 0] = -0.0013
    return y


def _build():
    cases = []
    add = lambda *c: cases.append(c)  # noqa: E731
    # 1. brute force: nothing is pruned
    k = 0
    for T, W, seed in ((5, 32, 11), (6, 64, 13)):
        for tname in ("hand3_o1", "hand3_o2", "hand3_o3"):
            for alpha in (0.5, 2.0):
                beta = (0.0, 0.7, -0.7)[k % 3]
                k += 1
                add(f"brute_T{T}_{tname[-2:]}_a{alpha}_b{beta}", _one(BR.make(seed + k, T, 3, 1.0)), 0, W, W, tname, alpha, beta)
    add("brute_T5_blank2", _one(BR.make(12, 5, 3, 1.0)), 2, 32, 32, "hand3_o2_blank2", 2.0, 0.7)
    # 2. the LM decides: the acoustically second class wins with alpha = 1
    add("decide_a0", _one(_decide_rows()), 0, 4, 4, "decide", 0.0, 0.0)
    add("decide_a1", _one(_decide_rows()), 0, 4, 4, "decide", 1.0, 0.0)
    # 3. exact ties in R: float32 inputs, dyadic lp, alpha, beta: ordered by candidate index
    tie = np.array([[-1.5, -2.0, -3.0, -1.0, -0.5, -2.0, -3.5, -2.0]], np.float32)   # R with alpha 1, beta 0.5: -2 -2 -2 (stay -1) -2 -2 -2 -2
    add("tie_R_equal", _one(tie), 3, 4, 4, "tie8", 1.0, 0.5)
    add("tie_R_equal_W8", _one(tie), 3, 8, 8, "tie8", 1.0, 0.5)
    # alpha = 2^53, beta = 1, lp = 1 for classes 2 and 6: class 2 has (-1 + 2^53) + 1 = 2^53 and class 6 (0 + 2^53) + 1 -> 2^53 (to even): a tie,
    # class 2 first.  s + (alpha g + beta len) gives class 2 only 2^53 - 1: class 6 first.
    big = np.array([[-4.0, -4.0, -1.0, -4.0, -4.0, -4.0, 0.0, -4.0]], np.float32)
    add("tie_assoc", _one(big), 3, 2, 2, "assoc8", 2.0 ** 53, 1.0)
    # 4. the hard rows of the acoustic case list under a random order-3 table
    for name, tname in (("one_hot", "rand5_o3"), ("dead_step", "rand5_o3"), ("nan_holes", "rand5_o3"), ("all_nan", "rand6_o3"),
                        ("identity_seed6_W3", "rand4_o3"), ("identity_seed35_W4", "rand4_o3"), ("identity_seed308_W3", "rand4_o3"),
                        ("identity_seed308_W4", "rand4_o3")):
        _, y, blank, W, nbest = CC.BY_NAME[name]
        add(name + "_lm", y, blank, W, nbest, tname, 0.8, 0.3)
    # 5. tables: ids to 1023 at order 6, a colliding and wrapping probe chain, missing unigrams
    add("order6_C1024_T16_W8", _one(BR.make(37, 16, 1024, 6.0)), 0, 8, 8, "order6_C1024", 1.0, 0.2)
    add("collide_T12_C40_W8", _one(BR.make(71, 12, 40, 2.0)), 39, 8, 8, "collide40", 1.5, -0.2)
    add("unk_T10_C5_W8", _one(BR.make(72, 10, 5, 1.5)), 0, 8, 8, "unk5_o2", 0.7, 0.1)
    # 6. real shapes
    lp = np.load(CC.GOLDEN)["log_probs"]
    add("golden_W8", np.ascontiguousarray(lp), 0, 8, 8, "trained_o4", 0.6, 0.4)
    add("golden_W64", np.ascontiguousarray(lp), 0, 64, 8, "trained_o4", 0.6, 0.4)
    add("text_like_W8", _one(BR.text_like(39, 80, 232, 8.0)), 0, 8, 4, "trained_o4", 0.5, 1.0)
    add("text_like_W64", _one(BR.text_like(73, 80, 232, 6.0, noise=2.0)), 0, 64, 16, "trained_o4", 0.5, 1.0)
    add("T300_C8_W64_workspace", _one(BR.make(40, 300, 8, 2.0)), 0, 64, 8, "rand8_o4", 0.4, 0.1)
    add("rows3_T140_C6_W64_workspace", CC.rows3_workspace(), 0, 64, 8, "rand6_o3", 0.4, 0.1)   # three rows' prefix tables and LM rows
    add("C2_T20_W8", _one(BR.make(38, 20, 2, 1.0)), 0, 8, 8, "rand2_o3", 1.0, 0.5)
    add("T64_C40_W16", _one(BR.make(34, 64, 40, 3.0)), 0, 16, 16, "rand40_o3", 0.9, -0.3)
    add("T65_C40_W16_blank39", _one(BR.make(35, 65, 40, 3.0)), 39, 16, 16, "rand40_o3_blank39", 0.9, 0.3)
    # 7. row independence
    add("rows5", np.ascontiguousarray(np.stack([BR.make(s, 12, 4, 1.5) for s in (6, 35, 308, 7, 8)], 1)), 0, 3, 3, "rand4_o3", 1.2, 0.25)
    return cases


CASES = _build()
BY_NAME = {c[0]: c for c in CASES}
EXACT = {"tie_R_equal", "tie_R_equal_W8", "tie_assoc", "one_hot_lm", "dead_step_lm", "all_nan_lm"}
assert len(BY_NAME) == len(CASES) and EXACT <= set(BY_NAME)


@functools.lru_cache(maxsize=None)
def reference(name: str, mutant=None):
    """(rows, gaps): rows[b] = [(prefix, R, s, g)] in rank order, at most W; gaps[b] = the per-step record of ``ctclm_ref.beam_lm``."""
    _, y, blank, W, _, tname, alpha, beta = BY_NAME[name]
    rows, gaps = [], []
    for b in range(y.shape[1]):
        g = []
        rows.append(LR.beam_lm(y[:, b], blank, W, table(tname), alpha, beta, g, mutant))
        gaps.append(g)
    return rows, gaps


def expected(name: str, mutant=None):
    """ids [B,nbest,T], lens [B,nbest], score, ctc_score, lm_score [B,nbest] as the device writes them."""
    _, y, _, _, nbest = BY_NAME[name][:5]
    return LR.outputs(reference(name, mutant)[0], y.shape[0], nbest)
