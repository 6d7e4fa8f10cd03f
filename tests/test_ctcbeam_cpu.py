"""The float64 restatement of the CTC prefix beam search (tests/ctcbeam_ref.py) against brute force, its mutants against the shared case
list (tests/ctcbeam_cases.py), the separation condition that makes a reference ranking comparable, the C ABI's text and the host half
(``make_hypotheses``, ``first_matching``).  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctcbeam_cases as CC  # noqa: E402
import ctcbeam_ref as BR  # noqa: E402

from ocr_vi_invoice_amd import _lib  # noqa: E402
from ocr_vi_invoice_amd.vocab import Tokenizer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ocrvi_ctc_beam_workspace_bytes", "ocrvi_ctc_beam")
NAMES = [c[0] for c in CC.CASES]

# mutant -> the cases whose expected device output (ids, lens, score of the first nbest) it changes
MUTANT_CASES = {
    "parent_node": ("identity_seed6_W3", "identity_seed35_W4", "identity_seed308_W3", "identity_seed308_W4", "golden_W8"),
    "no_merge": ("brute_C3_T5_blank0", "T80_C232_s1_W8"),
    "repeat_from_s": ("one_hot", "golden_W1"),
    "no_stay_pnb": ("one_hot", "text_like"),
    "tie_larger": ("tie_blank3", "tie_blank0", "tie_all_equal"),
    "nan_kept": ("nan_holes",),
    "select_pnb": ("tie_blank0", "T80_C232_s6_W8"),
}


def _head(name, mutant=None):
    nbest = CC.BY_NAME[name][4]
    return [r[:nbest] for r in CC.reference(name, mutant)[0]]


# ---------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", ["brute_C3_T5_blank0", "brute_C3_T5_blank2", "brute_C3_T6_W64"])
def test_beam_equals_brute_force_when_nothing_is_pruned(name):
    _, y, blank, W, nbest = CC.BY_NAME[name]
    want = BR.brute(y[:, 0], blank)
    got = CC.reference(name)[0][0]
    assert len(want) == {5: 25, 6: 41}[y.shape[0]] and len(want) < W
    assert sorted(l for l, _ in got) == sorted(want)                    # every labelling, once
    for l, s in got:
        assert abs(s - want[l]) <= 1e-14 * abs(want[l]), (l, s, want[l])
    assert got[0][0] == max(want, key=want.get)
    ids, lens, score = CC.expected(name)
    assert (lens[0, len(want):] == -1).all() and np.isneginf(score[0, len(want):]).all() and (ids[0, len(want):] == -1).all()
    assert (lens[0, :len(want)] >= 0).all()


def test_tie_and_hard_rows_by_hand():
    assert [l for l, _ in CC.reference("tie_blank3")[0][0]] == [(4,), (0,), (1,), ()]
    assert [l for l, _ in CC.reference("tie_blank0")[0][0]] == [(4,), (), (1,), (3,)]
    assert [s for _, s in CC.reference("tie_blank3")[0][0]] == [-0.5, -1.5, -1.5, -1.5]
    assert [l for l, _ in CC.reference("tie_all_equal")[0][0]] == [(0,), (1,), (2,), (3,)]
    assert CC.reference("one_hot")[0][0] == [((2, 3), 0.0)]
    assert CC.reference("dead_step")[0][0] == [] and CC.reference("all_nan")[0][0] == []
    holes = CC.reference("nan_holes")[0][0]
    assert len(holes) == 4 and all(np.isfinite(s) for _, s in holes)
    y = CC.BY_NAME["nan_holes"][1][:, 0].copy()
    y[np.isnan(y)] = -np.inf
    assert BR.beam(y, 0, 4) == holes                                    # a NaN is -inf


@pytest.mark.parametrize("name", NAMES)
def test_reference_outputs_are_ordered_and_distinct(name):
    for row in _head(name):
        scores = [s for _, s in row]
        assert scores == sorted(scores, reverse=True) and len({l for l, _ in row}) == len(row)
        assert all(s <= 1e-12 for s in scores)                           # log-probabilities


@pytest.mark.parametrize("name", [n for n in NAMES if n not in CC.EXACT])
def test_separation_condition(name):
    """Where the kernel's ranking is compared with the reference's, the reference's own ranking must not hang on the last bits: the
    smallest gap between consecutive totals among the first W+1 candidates of any step, and between consecutive returned scores, is at
    least 1e-9 max(1, |total|).  Not a filter: a case that fails it fails here.  ``ctcbeam_cases.EXACT`` is exempt by construction: exact
    ties, or at most one finite candidate."""
    rows, gaps = CC.reference(name)
    nbest = CC.BY_NAME[name][4]
    smallest = np.inf
    for row, steps in zip(rows, gaps):
        for head, diff in steps:
            if len(diff):
                smallest = min(smallest, float((diff / np.maximum(1.0, np.abs(head[:-1]))).min()))
        sc = np.array([s for _, s in row[:nbest]])
        if len(sc) > 1:
            smallest = min(smallest, float(((sc[:-1] - sc[1:]) / np.maximum(1.0, np.abs(sc[:-1]))).min()))
    print(f"{name}: smallest relative gap {smallest:.2e}")
    assert smallest >= 1e-9, (name, smallest)


# ---------------------------------------------------------------------------------------------------- the mutants
def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(BR.MUTANTS) and all(n in CC.BY_NAME for v in MUTANT_CASES.values() for n in v)


@pytest.mark.parametrize("mutant,name", [(m, n) for m, v in MUTANT_CASES.items() for n in v])
def test_each_mutant_changes_a_named_case(mutant, name):
    """Each broken rule changes what a GPU case expects, so a kernel that breaks it fails there."""
    y, nbest = CC.BY_NAME[name][1], CC.BY_NAME[name][4]
    good = BR.outputs(_head(name), y.shape[0], nbest)
    bad = BR.outputs(_head(name, mutant), y.shape[0], nbest)
    ids_differ = not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    with np.errstate(invalid="ignore"):
        rel = np.abs(good[2] - bad[2]) / np.maximum(1.0, np.abs(good[2]))
    score_differs = bool((np.nan_to_num(rel, nan=0.0, posinf=1.0) > 1e-6).any())   # far outside the GPU test's 1e-9
    assert ids_differ or score_differs, (mutant, name)
    if mutant == "parent_node" and name.startswith("identity"):
        assert _head(name, mutant) != _head(name)


# ---------------------------------------------------------------------------------------------------- the C ABI's text
def test_exports_header_and_abi():
    header = open(os.path.join(ROOT, "include", "ocrvi.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert "CTC prefix beam search" in header and "#define OCRVI_CTC_BEAM_MAX 64" in header and "#define OCRVI_CTC_BEAM_MAX_T 1024" in header
    assert _lib.CTC_BEAM_MAX == 64 and _lib.CTC_BEAM_MAX_T == 1024
    util = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "host_util.hip")).read()
    assert _lib.ABI_VERSION == 5 and "int ocrvi_abi_version(void) { return 5; }" in util
    src = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "ctc_beam.hip")).read()
    for name in NEW_EXPORTS:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    mk = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "Makefile")).read()
    assert "ctc_beam.hip" in mk and "ctc_beam_core.h" in re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1)   # an edit rebuilds both objects
    lm_src = open(os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "ctc_beam_lm.hip")).read()
    assert all('#include "ctc_beam_core.h"' in t for t in (src, lm_src))
    lib = _lib.load()                                                   # the built library (there is no other way to have the symbols)
    assert all(hasattr(lib, n) for n in NEW_EXPORTS) and lib.ocrvi_abi_version() == 5


def test_workspace_bytes_and_argument_checks_on_the_host():
    import ctypes as C
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.ocrvi_ctc_beam_workspace_bytes(80, 256, 232, 8, C.byref(n)) == 0 and n.value == 256 * 2 * 8 * 80 * 2
    assert lib.ocrvi_ctc_beam_workspace_bytes(5, 1, 3, 32, C.byref(n)) == 0 and n.value == 768     # T rounded up to 6, 768 bytes
    for T, B, Cn, W in ((0, 1, 3, 4), (1025, 1, 3, 4), (5, 0, 3, 4), (5, 1, 1, 4), (5, 1, 1025, 4), (5, 1, 3, 0), (5, 1, 3, 65)):
        n.value = 7
        assert lib.ocrvi_ctc_beam_workspace_bytes(T, B, Cn, W, C.byref(n)) == -1 and n.value == 7, (T, B, Cn, W)
    assert lib.ocrvi_ctc_beam_workspace_bytes(5, 1, 3, 4, None) == -1


# ---------------------------------------------------------------------------------------------------- the host half
def test_make_hypotheses_on_hand_made_arrays():
    from ocr_vi_invoice_amd.rec import Hypothesis, make_hypotheses
    tok = Tokenizer()
    a, b, c = sorted(tok.id_to_token)[:3]
    ids = np.full((3, 3, 6), -1, np.int32)
    lens = np.full((3, 3), -1, np.int32)
    score = np.full((3, 3), -np.inf)
    ids[0, 0, :3], lens[0, 0], score[0, 0] = (a, b, c), 3, -0.25
    ids[0, 1, :4], lens[0, 1], score[0, 1] = (a, 1, b, c), 4, -2.5      # pad id 1: the same text, its own hypothesis
    lens[0, 2], score[0, 2] = 0, -7.0                                   # the empty string is a hypothesis
    ids[1, 0, :1], lens[1, 0], score[1, 0] = (c,), 1, -1.0              # one finite hypothesis, two missing; row 2: none
    got = make_hypotheses(tok, ids, lens, score)
    t = tok.id_to_token
    assert got == [[Hypothesis(t[a] + t[b] + t[c], -0.25, (a, b, c)), Hypothesis(t[a] + t[b] + t[c], -2.5, (a, 1, b, c)),
                    Hypothesis("", -7.0, ())], [Hypothesis(t[c], -1.0, (c,))], []]
    assert all(isinstance(h.log_prob, float) and all(isinstance(i, int) for i in h.ids) for row in got for h in row)


def test_first_matching():
    from ocr_vi_invoice_amd.rec import Hypothesis, first_matching
    hyps = [Hypothesis("0l2345", -0.1, ()), Hypothesis("012345", -1.2, ()), Hypothesis("912345", -3.0, ())]
    assert first_matching(hyps, re.compile(r"\d{6}")) is hyps[1]
    assert first_matching(hyps, lambda s: s.isdigit() and sum(map(int, s)) % 8 == 0) is hyps[2]
    assert first_matching(hyps, re.compile(r"\d{7}")) is hyps[0]
    assert first_matching(hyps, re.compile(r"\d")) is hyps[0]                 # fullmatch, not search
    assert first_matching([], str.isdigit) is None


def test_check_beam_raises_before_any_device_work():
    from ocr_vi_invoice_amd.rec import check_beam
    check_beam(None, 99, 5000, True)                                    # beam=None: nothing to check
    check_beam(64, 64, 1024)
    for args in ((0, 1), (65, 1), (4, 5), (4, 0), (4.0, 1), (4, 1, 1025)):
        with pytest.raises(ValueError):
            check_beam(*args)
    with pytest.raises(ValueError):
        check_beam(4, 1, 80, True)
