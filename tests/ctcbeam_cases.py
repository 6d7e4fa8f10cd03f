"""The shared case list of the CTC prefix beam search tests: ``CASES`` = [(name, y [T,B,C] float32, blank, W, nbest)], the smallest shapes
at which the kernel can go wrong, and ``reference(name)``, computed once per process with tests/ctcbeam_ref.py and never changed.
``EXACT`` names the cases the separation condition does not apply to (exact ties, or at most one finite candidate)."""
import functools
import os

import numpy as np

import ctcbeam_ref as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rec_base_48x320.npz")
NINF, NAN = -np.inf, np.nan


def _one(y):
    return np.ascontiguousarray(np.asarray(y, np.float32)[:, None, :])


def _path_rows(path, C, hit=0.0, miss=NINF):
    y = np.full((len(path), C), miss, np.float32)
    y[np.arange(len(path)), path] = hit
    return y


def rows3_workspace():
    return np.ascontiguousarray(np.stack([BR.make(s, 140, 6, 2.0) for s in (50, 52, 58)], 1))


def _build():
    cases = []
    add = lambda name, y, blank, W, nbest: cases.append((name, y, blank, W, nbest))  # noqa: E731
    # 1. brute force: nothing is pruned, every labelling comes back with its full probability
    add("brute_C3_T5_blank0", _one(BR.make(11, 5, 3, 1.0)), 0, 32, 32)
    add("brute_C3_T5_blank2", _one(BR.make(12, 5, 3, 1.0)), 2, 32, 32)
    add("brute_C3_T6_W64", _one(BR.make(13, 6, 3, 1.0)), 0, 64, 64)
    # 2. the tie rule: one step, several classes with the same float32 (no logarithm is taken: the ties are exact)
    tie = np.array([[-1.5, -1.5, -3.0, -1.5, -0.5, -1.5, -4.0, -1.5]], np.float32)
    add("tie_blank3", _one(tie), 3, 4, 4)          # (4), then -1.5 by class index: (0), (1), the stay candidate ()
    add("tie_blank0", _one(tie), 0, 4, 4)          # (4), the stay candidate () first among the -1.5, (1), (3)
    add("tie_all_equal", _one(np.full((1, 8), -2.0, np.float32)), 5, 4, 4)
    # 3. hard rows
    add("one_hot", _one(_path_rows([0, 2, 2, 0, 3, 3], 5)), 0, 4, 4)                 # exactly one hypothesis: (2, 3)
    dead = BR.make(21, 6, 5, 2.0)
    dead[3] = NINF
    add("dead_step", _one(dead), 0, 4, 4)                                            # a step of -inf: no hypothesis at all
    holes = BR.make(22, 8, 5, 2.0)
    holes[2, 0] = NAN                                                                # the blank
    holes[3, int(holes[2, 1:].argmax()) + 1] = NAN                                   # the class the best prefix ends in
    holes[5, 1:3] = NAN
    holes[6, 4] = NINF
    add("nan_holes", _one(holes), 0, 4, 4)
    add("all_nan", _one(np.full((4, 6), NAN, np.float32)), 0, 4, 4)
    # 4. string identity: a prefix that left the beam is created again while one of its children is still there
    for seed, W in ((6, 3), (35, 4), (308, 3), (308, 4)):
        add(f"identity_seed{seed}_W{W}", _one(BR.make(seed, 12, 4, 1.5)), 0, W, W)
    # 5. real shapes
    lp = np.load(GOLDEN)["log_probs"]
    for W in (1, 8, 64):
        add(f"golden_W{W}", np.ascontiguousarray(lp), 0, W, min(W, 8))
    add("T80_C232_s6_W8", _one(BR.make(31, 80, 232, 6.0)), 0, 8, 8)
    add("T80_C232_s6_W64", _one(BR.make(32, 80, 232, 6.0)), 0, 64, 16)
    add("T80_C232_s1_W8", _one(BR.make(33, 80, 232, 1.0)), 0, 8, 8)
    add("T64_C40_W16", _one(BR.make(34, 64, 40, 3.0)), 0, 16, 16)
    add("T65_C40_W16", _one(BR.make(35, 65, 40, 3.0)), 39, 16, 16)
    add("T200_C232_W8", _one(BR.make(36, 200, 232, 6.0)), 0, 8, 4)
    add("C1024_T16_W8", _one(BR.make(37, 16, 1024, 6.0)), 0, 8, 8)
    add("C2_T20_W8", _one(BR.make(38, 20, 2, 1.0)), 0, 8, 8)
    add("text_like", _one(BR.text_like(39, 80, 232, 8.0)), 0, 8, 4)
    # both prefix tables of (W = 64, T = 300) are past 32 KiB: they live in the workspace, not in LDS
    add("T300_C8_W64_workspace", _one(BR.make(40, 300, 8, 2.0)), 0, 64, 8)
    # the same path with three rows: each takes its own part of the workspace (2 * 64 * 140 * 2 = 35 840 bytes a row)
    add("rows3_T140_C6_W64_workspace", rows3_workspace(), 0, 64, 8)
    # 6. row independence: five different rows in one launch (the GPU test also launches each alone)
    add("rows5", np.ascontiguousarray(np.stack([BR.make(s, 12, 4, 1.5) for s in (6, 35, 308, 7, 8)], 1)), 0, 3, 3)
    return cases


CASES = _build()
BY_NAME = {c[0]: c for c in CASES}
EXACT = {"tie_blank3", "tie_blank0", "tie_all_equal", "one_hot", "dead_step", "all_nan"}
assert len(BY_NAME) == len(CASES) and EXACT <= set(BY_NAME)


@functools.lru_cache(maxsize=None)
def reference(name: str, mutant=None):
    """(rows, gaps): rows[b] = [(prefix, score)] in rank order, at most W; gaps[b] = the per-step record of ``ctcbeam_ref.beam``."""
    _, y, blank, W, _ = BY_NAME[name]
    rows, gaps = [], []
    for b in range(y.shape[1]):
        g = []
        rows.append(BR.beam(y[:, b], blank, W, g, mutant))
        gaps.append(g)
    return rows, gaps


def expected(name: str):
    """ids [B,nbest,T], lens [B,nbest], score [B,nbest] as the device writes them."""
    _, y, _, _, nbest = BY_NAME[name]
    return BR.outputs(reference(name)[0], y.shape[0], nbest)
