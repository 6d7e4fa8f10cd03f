"""The float64 / integer restatements of tests/eval_refs.py against goldens the reference's own modules produced
(tests/golden/make_eval_golden.py: DBLoss, compute_metrics and validate_epoch of the detector, SVTRv2Loss and nn.CTCLoss of the
recogniser), and the host side of ``ocr_vi_invoice_amd.val``.  No GPU.

Bounds: the reference computes in float32, the restatements in float64, so they differ by the reference's own rounding.  On a
[2,1,64,96] probe that was 2.1e-7 (l_prob), 6.2e-9 (l_binary), 1.3e-8 (l_thresh) absolute and 1.2e-7 relative for the CTC mean; the tests
assert 1e-6 relative (1e-6 absolute for l_binary), about ten float32 ulps.  Measured on the fixtures (|restatement - reference|):
  batch 0: l_prob 1.4e-08, l_binary 9.1e-08, l_thresh 3.8e-09, loss 8.2e-07 (relative 3.1e-08, 2.5e-07, 1.9e-08, 1.9e-07)
  batch 1: l_prob 5.6e-09, l_binary 3.5e-08, l_thresh 7.2e-10, loss 2.8e-07 (relative 2.3e-08, 2.5e-07, 3.9e-09, 1.0e-07)
  CTC: per-sequence nll at most 1.5e-07 relative, SVTRv2Loss mean 3.6e-08 relative (stored lengths), 8.0e-08 (default lengths)
Counts, k and the five metrics (float32 ratios of exact counts) are equal, not close."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_refs as ER  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(REPO, "tests", "golden")
MAPS = ("binary", "thresh", "thresh_binary", "bin_logits", "gt", "mask", "thresh_map", "thresh_mask")
METRICS = ("precision", "recall", "f1", "iou", "dice")
NEW_SYMBOLS = ("ocrvi_det_eval_workspace_bytes", "ocrvi_det_eval", "ocrvi_ctc_loss", "ocrvi_edit_distance")


@pytest.fixture(scope="module")
def det():
    return np.load(os.path.join(GOLDEN, "eval_det.npz"))


@pytest.fixture(scope="module")
def rec():
    return np.load(os.path.join(GOLDEN, "eval_rec.npz"))


@pytest.fixture(scope="module")
def det_records(det):
    return [ER.det_eval(*[det[f"b{i}_{k}"] for k in MAPS]) for i in range(2)]


def test_fixture_shapes_are_the_small_ones(det, rec):
    assert det["b0_binary"].shape == (2, 1, 32, 48) and det["b1_gt"].shape == (2, 1, 32, 48)
    assert rec["log_probs"].shape == (24, 6, 232)
    assert list(rec["target_lengths"]) == [0, 1, 5, 8, 7, 10] and rec["input_lengths"][4] < 24 and rec["input_lengths"][5] < 10
    t = rec["targets"][2]
    assert any(t[i] == t[i + 1] for i in range(4))
    frac = det["b0_gt"]
    assert ((frac > 0) & (frac < 1)).sum() >= 5 and ((det["b0_mask"] > 0) & (det["b0_mask"] < 1)).sum() >= 4


@pytest.mark.parametrize("i", [0, 1])
def test_det_counts_and_k_equal_the_reference(det, det_records, i):
    r = det_records[i]
    assert r["negative_count"] == int(det[f"b{i}_k"])
    # batch 0 is limited by the ratio, batch 1 by the number of negatives
    assert (r["negative_count"] == 3 * r["positive_count"] < r["negatives"]) if i == 0 else (r["negative_count"] == r["negatives"])
    got = ER.metrics(r["tp"], r["fp"], r["fn"])
    for k in METRICS:      # float32 ratios of the counts: equal only if tp, fp and fn are
        assert got[k] == float(det[f"b{i}_{k}"]), (k, got[k], float(det[f"b{i}_{k}"]))


@pytest.mark.parametrize("i", [0, 1])
def test_det_loss_terms_within_the_reference_rounding(det, det_records, i):
    got = ER.db_loss(det_records[i])
    for k in ("l_prob", "l_binary", "l_thresh", "loss"):
        want = float(det[f"b{i}_{k}"])
        diff = abs(got[k] - want)
        print(f"batch {i} {k}: restatement {got[k]!r} reference {want!r} diff {diff:.2e} rel {diff / abs(want):.2e}")
        assert diff <= (1e-6 if k == "l_binary" else 1e-6 * abs(want)), (k, got[k], want)


def test_validate_epoch_is_the_mean_over_batches(det, det_records):
    losses = [ER.db_loss(r)["loss"] for r in det_records]
    assert abs(np.mean(losses) - float(det["val_loss"])) <= 1e-6 * float(det["val_loss"])
    for k in METRICS:
        per = [ER.metrics(r["tp"], r["fp"], r["fn"])[k] for r in det_records]
        assert float(np.mean(per)) == float(det[f"val_{k}"]), k


def test_ctc_nll_within_the_reference_rounding(rec):
    for key, il in (("nll", rec["input_lengths"]), ("nll_full_length", None)):
        got = ER.ctc_nll(rec["log_probs"], rec["targets"], rec["target_lengths"], il)
        want = rec[key]
        assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
        fin = np.isfinite(want)
        rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
        print(f"{key}: max relative difference {rel.max():.2e}")
        assert rel.max() <= 1e-6
    assert np.isinf(rec["nll"][5]) and rec["nll"][5] > 0 and np.isfinite(rec["nll_full_length"]).all()


def test_ctc_mean_matches_svtrv2loss(rec):
    nll = ER.ctc_nll(rec["log_probs"], rec["targets"], rec["target_lengths"], rec["input_lengths"])
    got = ER.ctc_loss(nll, rec["target_lengths"])
    want = float(rec["loss_mean"])
    print(f"mean: {got!r} vs {want!r} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-6 * want
    # default lengths: every input is T long, target lengths are the non-pad counts
    lens = (rec["targets"] != 1).sum(1)
    assert list(lens) == list(rec["target_lengths"])
    got = ER.ctc_loss(ER.ctc_nll(rec["log_probs"], rec["targets"], lens, None), lens)
    want = float(rec["loss_mean_default"])
    print(f"default: {got!r} vs {want!r} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-6 * want


def test_ctc_edges_of_the_recursion():
    lp = np.log(np.full((3, 1, 3), 1 / 3))
    one = lambda t, L, il=None: ER.ctc_nll(lp, np.array([t]), [L], il)[0]   # noqa: E731
    assert abs(one([1, 1], 0) - 3 * np.log(3)) < 1e-12                 # the all-blank path alone
    assert abs(one([2, 2], 2) - (-np.log(1 / 27))) < 1e-12             # a b a is the one alignment of a repeat on three steps
    assert one([2, 2], 2, [2]) == np.inf                               # and there is none on two
    assert abs(one([1, 2], 2, [2]) - 2 * np.log(3)) < 1e-12            # distinct labels: a b
    assert abs(one([1, 2], 1) - (-np.log(6 / 27))) < 1e-12             # one label on three steps: 6 of the 27 paths collapse to it


def test_levenshtein_known_answers():
    from ocr_vi_invoice_amd.vocab import Tokenizer
    tok = Tokenizer()
    enc = lambda s: ER.encode_text(s, tok.token_to_id)   # noqa: E731
    assert ER.levenshtein("kitten", "sitting") == 3 == ER.levenshtein_recursive("kitten", "sitting")
    assert ER.levenshtein(enc("kitten"), enc("sitting")) == 3
    assert ER.levenshtein("", "abc") == 3 and ER.levenshtein("abc", "") == 3 and ER.levenshtein("", "") == 0
    # a ground truth with a character outside the alphabet: it becomes -2 and matches nothing, as in the string distance
    assert "中" not in tok.token_to_id
    gt = enc("a中c")
    assert gt[1] == -2 and ER.levenshtein(enc("abc"), gt) == 1 == ER.levenshtein("abc", "a中c")
    assert ER.levenshtein(enc("ac"), gt) == 1 and ER.levenshtein(enc("a中c"), gt) == 0
    # a prediction row containing pad id 1 (and a stray blank): dropped before the distance
    a, b, c = enc("abc")
    pred = np.array([[a, 1, b, 0, c, -1]], np.int32)
    assert ER.edit_distance(pred, [5], np.array([[a, b, c]], np.int32), [3])[0] == 0
    assert ER.edit_distance(pred, [3], np.array([[a, b, c]], np.int32), [3])[0] == 1     # the row ends before c
    assert ER.cer(["abd", ""], ["abc", "xy"]) == 3 / 5 and ER.acc(["abc", "x"], ["abc", "y"]) == 0.5
    assert ER.cer([], []) == 0.0 and ER.acc([], []) == 0.0


def test_the_two_levenshtein_definitions_agree():
    rng = np.random.default_rng(5)
    for _ in range(300):
        a = rng.integers(2, 5, rng.integers(0, 7)).tolist()
        b = rng.integers(2, 5, rng.integers(0, 7)).tolist()
        assert ER.levenshtein(a, b) == ER.levenshtein_recursive(a, b), (a, b)


def test_val_module_host_side():
    import torch
    import ocr_vi_invoice_amd
    from ocr_vi_invoice_amd import val
    for name in ("DBLoss", "compute_metrics", "SVTRv2Loss", "compute_cer", "compute_acc", "validate_detection", "validate_recognition"):
        assert getattr(ocr_vi_invoice_amd, name) is getattr(val, name), name
    with pytest.raises(NotImplementedError):
        val.SVTRv2Loss()(torch.zeros(4, 1, 232), torch.zeros(1, 2, dtype=torch.long), sgm_output={"sgm_left": None})
    with pytest.raises(ValueError):
        val.SVTRv2Loss(reduction="median")
    assert val.compute_acc(["abc", "x"], ["abc", "y"]) == 0.5 and val.compute_acc([], []) == 0.0
    # the ratios: float32 arithmetic on exact counts, the same numbers as the restatement
    for tp, fp, fn in ((0, 0, 0), (319, 220, 24), (5, 0, 0), (1 << 22, 3, 77)):
        assert val.metrics_from_counts(tp, fp, fn) == ER.metrics(tp, fp, fn)
    rec = dict(positive_count=10, negative_count=30, pos_bce=4.0, topk_bce=6.0, dice_inter=3.0, pred_mask=5.0, gt_mask=4.0, l1_num=2.0,
               thresh_mask=8.0)
    assert val.db_loss_terms(rec) == ER.db_loss(rec)
    ids, lens = val.encode_ground_truth(["ab", "", "a中"], val.Tokenizer())
    assert lens.tolist() == [2, 0, 2] and ids[2, 1] == -2 and ids.dtype == np.int32


def test_new_symbols_are_exported_and_declared():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "ocrvi.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.ocrvi_abi_version() == _lib.ABI_VERSION == 5
    defs = dict(re.findall(r"#define (OCRVI_[A-Z0-9_]+) (\d+)", header))
    assert int(defs["OCRVI_DET_EVAL_RECORD_BYTES"]) == _lib.DET_EVAL_RECORD_BYTES == 8 * (len(_lib.DET_EVAL_INT_SLOTS) + len(_lib.DET_EVAL_F64_SLOTS))
    order = ["TP", "FP", "FN", "POSITIVES", "NEGATIVES", "K", "POS_BCE", "TOPK_BCE", "DICE_INTER", "PRED_MASK", "GT_MASK", "L1_NUM", "THRESH_MASK"]
    assert [int(defs["OCRVI_DET_EVAL_" + n]) for n in order] == list(range(13))
    assert int(defs["OCRVI_CTC_LOSS_MAX_TARGET"]) == _lib.CTC_LOSS_MAX_TARGET
    assert int(defs["OCRVI_EDIT_DISTANCE_MAX_LEN"]) == _lib.EDIT_DISTANCE_MAX_LEN
    # host-side argument checks need no device
    n = __import__("ctypes").c_size_t()
    assert lib.ocrvi_det_eval_workspace_bytes(2, 32, 48, __import__("ctypes").byref(n)) == 0 and n.value >= 2 * 32 * 48 * 4
    assert lib.ocrvi_det_eval_workspace_bytes(0, 32, 48, __import__("ctypes").byref(n)) == -1
