"""The numpy statement of the greedy CTC confidences (tests/ctcconf_ref.py) against what is already pinned -- the golden strings,
torch's log_softmax / gather, the float64 CTC forward of tests/eval_refs.py -- and against deliberate mis-statements of itself; the host
arithmetic of the library (``rec.make_recognitions``, ``pipeline.char_boxes``) against it; the C ABI's text.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctcconf_ref as CR  # noqa: E402
import eval_refs as ER  # noqa: E402

from ocr_vi_invoice_amd import _lib  # noqa: E402
from ocr_vi_invoice_amd.vocab import Tokenizer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_EXPORTS = ("ocrvi_rec_forward_conf", "ocrvi_ctc_greedy_conf", "ocrvi_test_ctc_logsoftmax_conf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- against what is pinned
def test_reference_decodes_the_known_answer_paths():
    g = np.load(os.path.join(GOLDEN, "ctc_kat.npz"))
    seqs = g["seqs"]
    B, T = seqs.shape
    lp = np.full((T, B, 232), -10.0, np.float32)
    for b in range(B):
        lp[np.arange(T), b, seqs[b]] = -0.1
    r = CR.greedy_conf(lp)
    assert np.array_equal(r["argmax"], seqs)
    tok = Tokenizer()
    assert tok.decode([row[:n] for row, n in zip(r["ids"].tolist(), r["lens"].tolist())]) == [str(s) for s in g["strings"]]
    recs = CR.recognitions(tok.id_to_token, r["ids"], r["lens"], r["char_lp"], r["char_span"])
    assert [x[0] for x in recs] == [str(s) for s in g["strings"]]
    for text, score, scores, spans, logp in recs:
        assert len(text) == len(scores) == len(spans) and logp is None
        assert all(s == math.exp(float(np.float32(-0.1))) for s in scores)
        assert score == (math.fsum(scores) / len(scores) if scores else 0.0)
        assert all(0 <= t0 <= t1 < T for t0, t1 in spans) and list(spans) == sorted(spans)


def test_reference_decodes_the_golden_recogniser_output():
    g = np.load(os.path.join(GOLDEN, "rec_tiny_32x256.npz"))
    r = CR.greedy_conf(g["log_probs"])
    assert np.array_equal(r["argmax"], g["argmax_ids"])
    recs = CR.recognitions(Tokenizer().id_to_token, r["ids"], r["lens"], r["char_lp"], r["char_span"])
    assert [x[0] for x in recs] == [str(s) for s in g["strings"]]


def test_best_lp_is_torch_gather_of_the_argmax():
    rng = np.random.default_rng(5)
    lp = torch.log_softmax(torch.from_numpy(rng.normal(0, 2, (37, 3, 65)).astype(np.float32)), -1)
    am = lp.argmax(-1)                                                   # [T,B]
    want = lp.gather(-1, am[..., None])[..., 0].T.contiguous().numpy()  # [B,T]
    got_am, got = CR.argmax_rows(lp.numpy())
    assert np.array_equal(got_am, am.T.numpy())
    assert np.array_equal(_bits(got), _bits(want))


def test_log_prob_bounds_on_seeded_rows():
    """log_prob = -nll of the collapsed ids over all alignments: a probability, so <= 0, and at least the probability of the greedy path,
    which is one alignment of its own string: log_prob >= sum_t best_lp.  Allowance: the float64 recursion does at most three logaddexp
    and one addition per step on numbers no larger than |sum_t best_lp| + 1, each within 2 ulp: 16 T 2^-53 (1 + |sum_t best_lp|)."""
    rng = np.random.default_rng(11)
    T, B, C = 70, 6, 40
    lp = CR.random_peaked(rng, T, B, C)
    r = CR.greedy_conf(lp)
    assert r["lens"].max() >= 3
    logp = -ER.ctc_nll(lp, r["ids"], r["lens"])
    path = r["best_lp"].astype(np.float64).sum(1)
    allow = 16 * T * 2.0 ** -53 * (1 + np.abs(path))
    print("log_prob", logp, "greedy path", path)
    assert (logp <= 0).all()
    assert (logp >= path - allow).all()


# ---------------------------------------------------------------------------------------------------- the host arithmetic
def test_make_recognitions_equals_the_reference_arithmetic():
    from ocr_vi_invoice_amd.rec import Recognition, make_recognitions
    tok = Tokenizer()
    rows = np.stack([CR.cases(12, 232)[k] for k in ("pad_id_emitted", "a_blank_a", "all_blank", "alternation")], 1)
    rows[:, 1, 1], rows[:, 1, 40] = -9.0, rows[:, 1, 1].copy()          # a real character (id 40) in place of id 1
    r = CR.greedy_conf(rows)
    want = CR.recognitions(tok.id_to_token, r["ids"], r["lens"], r["char_lp"], r["char_span"], [-1.5, -2.5, -0.0, -3.0])
    got = make_recognitions(tok, r["ids"], r["lens"], r["char_lp"], r["char_span"], [-1.5, -2.5, -0.0, -3.0])
    assert got == make_recognitions(tok, r["ids"].tolist(), r["lens"].tolist(), r["char_lp"].tolist(), r["char_span"].tolist(),
                                    [-1.5, -2.5, -0.0, -3.0])
    assert all(isinstance(g, Recognition) for g in got)
    assert [tuple(g) for g in got] == want
    assert got[0].text == "" and got[0].score == 0.0 and got[0].char_scores == () and got[0].spans == ()      # only pad ids: all dropped
    assert r["lens"][0] == 4 and got[2].text == "" and len(got[1].text) == 5
    assert got[1]._fields == ("text", "score", "char_scores", "spans", "log_prob")
    none = make_recognitions(tok, r["ids"], r["lens"], r["char_lp"], r["char_span"])
    assert all(g.log_prob is None for g in none)


CHAR_BOX_CASES = [
    # (rect, rec_size, spans, want), worked by hand from the definition in pipeline.char_boxes
    ("squeezed: new_w 1000 > 256", (10, 20, 1000, 32), (32, 256), [(0, 0), (10, 12), (63, 63)],
     [(10, 20, 16, 32), (166, 20, 48, 32), (994, 20, 16, 32)]),
    ("a span inside the padding", (5, 7, 64, 32), (32, 256), [(15, 16), (20, 21)], [(65, 7, 4, 32), (68, 7, 1, 32)]),
    ("w = 1", (3, 4, 1, 40), (32, 256), [(0, 0), (5, 9)], [(3, 4, 1, 40), (3, 4, 1, 40)]),
    ("new_w = int(98 * (32 / 49)) = 63 in floating point, as the device computes it", (0, 0, 98, 49), (32, 256), [(15, 15), (0, 1)],
     [(93, 0, 5, 49), (0, 0, 13, 49)]),
]


@pytest.mark.parametrize("name,rect,rec_size,spans,want", CHAR_BOX_CASES, ids=[c[0] for c in CHAR_BOX_CASES])
def test_char_boxes_hand_computed(name, rect, rec_size, spans, want):
    from ocr_vi_invoice_amd.pipeline import char_boxes
    from ocr_vi_invoice_amd.rec import Recognition
    assert CR.char_boxes(rect, spans, rec_size).tolist() == [list(w) for w in want]
    rec = Recognition("x" * len(spans), 0.5, (0.5,) * len(spans), tuple(spans), None)
    got = char_boxes(rect, rec, rec_size)
    assert got.dtype == np.int32 and got.shape == (len(spans), 4) and got.tolist() == [list(w) for w in want]


def test_char_boxes_stay_inside_the_crop_and_refuse_quads():
    from ocr_vi_invoice_amd.pipeline import char_boxes
    from ocr_vi_invoice_amd.rec import Recognition
    rng = np.random.default_rng(3)
    spans = tuple((t, min(t + int(rng.integers(0, 4)), 63)) for t in range(0, 64, 3))
    rec = Recognition("x" * len(spans), 0.5, (0.5,) * len(spans), spans, None)
    for rect in [(7, 9, int(w), int(h)) for w, h in rng.integers(1, 700, (40, 2))]:
        got = char_boxes(rect, rec)
        assert np.array_equal(got, CR.char_boxes(rect, spans))
        assert (got[:, 0] >= rect[0]).all() and (got[:, 2] >= 1).all() and (got[:, 0] + got[:, 2] <= rect[0] + rect[2]).all()
        assert (got[:, 1] == rect[1]).all() and (got[:, 3] == rect[3]).all()
    with pytest.raises(ValueError):
        char_boxes(np.zeros((4, 2), np.int32), rec)                       # four corners: an oriented crop
    with pytest.raises(ValueError):
        char_boxes(np.zeros((4, 2), np.float64), rec)
    with pytest.raises(ValueError):
        char_boxes((0, 0, 0, 5), rec)


# ---------------------------------------------------------------------------------------------------- mutants
MUTANT_CASES = {
    # mutant -> (T, the case of CR.cases that catches it, the output it corrupts)
    "first_step": (5, "one_char_all_steps_max_last", "char_lp"),
    "span_end": (5, "one_char_all_steps_max_first", "char_span"),
    "carry64": (70, "run_62_66_max_last", "char_lp"),
}


@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_each_mutant_is_caught_by_a_named_case(mutant):
    T, name, field = MUTANT_CASES[mutant]
    for blank in (0, 2):
        lp = CR.cases(T, 5, blank)[name][:, None, :]
        good, bad = CR.greedy_conf(lp, blank), CR.greedy_conf(lp, blank, mutant)
        assert good["lens"][0] == 1
        assert not np.array_equal(_bits(good[field]) if field == "char_lp" else good[field], _bits(bad[field]) if field == "char_lp" else bad[field])
        for k in ("argmax", "ids", "lens", "best_lp"):                   # what the mutants leave alone
            assert np.array_equal(good[k], bad[k])
        quiet = CR.cases(T, 5, blank)["all_blank"][:, None, :]           # and a row without characters tells them apart from nothing
        assert all(np.array_equal(CR.greedy_conf(quiet, blank)[k], CR.greedy_conf(quiet, blank, mutant)[k]) for k in ("char_lp", "char_span"))


def test_carry_case_values():
    """The run 62..66 with its maximum on step 66: one record, (62, 66), the value of step 66."""
    r = CR.greedy_conf(CR.cases(70, 5)["run_62_66_max_last"][:, None, :])
    assert r["lens"][0] == 1 and r["char_span"][0, 0].tolist() == [62, 66] and r["char_lp"][0, 0] == np.float32(-0.0625)
    assert r["char_span"][0, 1].tolist() == [-1, -1] and np.isneginf(r["char_lp"][0, 1])
    r = CR.greedy_conf(CR.cases(200, 5, 2)["nan_through_a_boundary"][:, None, :], 2)
    assert r["lens"][0] == 1 and r["char_span"][0, 0].tolist() == [60, 129] and r["char_lp"][0, 0] == np.float32(-0.0625)
    r = CR.greedy_conf(CR.cases(8, 5, 2)["all_nan"][:, None, :], 2)
    assert r["lens"][0] == 1 and r["char_span"][0, 0].tolist() == [0, 7] and np.isnan(r["char_lp"][0, 0])


# ---------------------------------------------------------------------------------------------------- the C ABI's text
def test_exports_header_and_abi():
    header = open(os.path.join(ROOT, "include", "ocrvi.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(" % name, header, re.M), name
    util = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "host_util.hip")).read()
    assert _lib.ABI_VERSION == 5 and "int ocrvi_abi_version(void) { return 5; }" in util
    for phrase in ("best_lp[b,t] is the float32 that log_probs[t,b,argmax_ids[b,t]] holds, bit for bit", "char_span [B,T,2] int32",
                   "(-1, -1) for k >= lens[b]", "under fmaxf", "-inf for k >= lens[b]"):
        assert phrase in header, phrase
    src = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "rec_model.hip")).read()
    for name in NEW_EXPORTS[:2]:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, n) for n in NEW_EXPORTS) and lib.ocrvi_abi_version() == 5
