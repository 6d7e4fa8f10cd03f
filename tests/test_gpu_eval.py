"""Validation on the device: ``ocrvi_det_eval``, ``ocrvi_ctc_loss`` and ``ocrvi_edit_distance`` through the C ABI against the float64 /
integer restatements of tests/eval_refs.py, and the ``ocr_vi_invoice_amd.val`` loops against the reference-run goldens.

Bounds.  det_eval: counts and k exact; every sum within 2e-6 relative of float64 -- each float32 term is good to a few ulps (at most
8 x 2^-23, about 1e-6 relative), the terms of one sum share a sign and the accumulation is float64; the bound doubles that -- and the
same bound, absolute, for the dice term l_binary.  ctc_loss: 1e-9 relative -- both sides run the same recursion in float64 from the same
float32 inputs, only exp / log differ -- with +inf exactly where the restatement has it.  edit_distance: exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_refs as ER  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(REPO, "tests", "golden")
MAPS = ("binary", "thresh", "thresh_binary", "bin_logits", "gt", "mask", "thresh_map", "thresh_mask")
INT_SLOTS = ("tp", "fp", "fn", "positive_count", "negatives", "negative_count")
F64_SLOTS = ("pos_bce", "topk_bce", "dice_inter", "pred_mask", "gt_mask", "l1_num", "thresh_mask")
SUM_BOUND = 2e-6
SENTINEL, PAD = 0xAB, 256


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- det_eval
def _maps(seed, shape, fill=0.1, logit_of=None):
    """Eight seeded maps: rectangles of text covering about `fill` of each page, logits that mostly agree with them, an ignored strip."""
    rng = np.random.default_rng(seed)
    N, _, H, W = shape
    gt = np.zeros(shape, np.float32)
    for n in range(N):
        while gt[n].mean() < fill:
            y, x = rng.integers(0, max(H - 4, 1)), rng.integers(0, max(W - 6, 1))
            gt[n, 0, y:y + rng.integers(2, 5), x:x + rng.integers(3, 7)] = 1
    mask = np.ones_like(gt)
    mask[..., :2] = 0
    logits = (rng.normal(0, 1.5, shape) + (gt * 4 - 2)).astype(np.float32) if logit_of is None else logit_of(rng, gt).astype(np.float32)
    binary = (1 / (1 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
    thresh = (1 / (1 + np.exp(-rng.normal(0, 1, shape)))).astype(np.float32)
    thresh_binary = (1 / (1 + np.exp(-50 * (binary.astype(np.float64) - thresh)))).astype(np.float32)
    thresh_map = (0.3 + 0.4 * rng.random(shape)).astype(np.float32)
    thresh_mask = (rng.random(shape) < 0.35).astype(np.float32)
    return dict(zip(MAPS, (binary, thresh, thresh_binary, logits, gt, mask, thresh_map, thresh_mask)))


def _golden_batch(i):
    z = np.load(os.path.join(GOLDEN, "eval_det.npz"))
    return {k: z[f"b{i}_{k}"] for k in MAPS}


def _case(name):
    if name in ("golden0", "golden1"):
        return _golden_batch(int(name[-1]))
    if name == "three_pages_32x160":
        return _maps(1, (3, 1, 32, 160))
    if name == "two_pages_256x256":
        return _maps(2, (2, 1, 256, 256), fill=0.15)
    if name == "few_negatives":                    # fewer than 3 x positives: k = every negative
        return _maps(3, (2, 1, 32, 48), fill=0.5)
    if name == "no_positives":                     # k = 0
        m = _maps(4, (2, 1, 32, 48))
        m["gt"][:] = 0
        return m
    if name == "every_logit_equal":                # every negative's loss ties at the k-th value
        return _maps(5, (2, 1, 32, 48), logit_of=lambda rng, gt: np.full(gt.shape, 0.75))
    if name == "two_loss_values":                  # k falls inside the lower of two groups of equal losses
        def two(rng, gt):
            return np.where(rng.random(gt.shape) < 0.1, 2.0, -1.0)
        return _maps(6, (2, 1, 32, 48), fill=0.12, logit_of=two)
    if name == "fractional_gt_and_mask":           # .byte() truncation, == 1 / == 0 on products that are neither
        m = _maps(7, (2, 1, 32, 48))
        m["gt"][0, 0, 5, 7:12] = [0.5, 0.25, 0.999, 0.75, 0.5]
        m["gt"][1, 0, 9, 3:6] = [0.5, 0.125, 0.875]
        m["mask"][1, 0, 20, 30:34] = [0.5, 0.999, 0.25, 0.75]
        m["mask"][0, 0, 5, 9] = 0.5
        return m
    if name == "odd_size":                         # 63 pixels: the scalar tail beside the groups of four
        return _maps(8, (1, 1, 7, 9), fill=0.2)
    raise KeyError(name)


DET_CASES = ("golden0", "golden1", "three_pages_32x160", "two_pages_256x256", "few_negatives", "no_positives", "every_logit_equal",
             "two_loss_values", "fractional_gt_and_mask", "odd_size")
_REF = {}


def _ref(name):
    if name not in _REF:                           # computed once per case and shared
        m = _case(name)
        _REF[name] = (m, ER.det_eval(*[m[k] for k in MAPS]))
    return _REF[name]


def _run_det_eval(maps, shift=0, ratio=3.0):
    """``ocrvi_det_eval`` with the maps `shift` floats into their buffers and sentinel bytes behind the workspace and around the record."""
    L, lib = _L()
    N, _, H, W = maps["gt"].shape
    n = N * H * W
    dev = []
    for k in MAPS:
        buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        buf[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(maps[k]).reshape(-1)).cuda()
        dev.append(buf)
    need = C.c_size_t()
    L.check(lib.ocrvi_det_eval_workspace_bytes(N, H, W, C.byref(need)))
    ws = torch.full((need.value + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rec = torch.full((L.DET_EVAL_RECORD_BYTES + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    L.check(lib.ocrvi_det_eval(0, *[b.data_ptr() + 4 * shift for b in dev], N, H, W, ratio, rec.data_ptr() + PAD, ws.data_ptr(), need.value,
                               _stream()))
    raw = rec.cpu().numpy()
    assert (ws[need.value:].cpu().numpy() == SENTINEL).all()
    assert (raw[:PAD] == SENTINEL).all() and (raw[PAD + L.DET_EVAL_RECORD_BYTES:] == SENTINEL).all()
    body = raw[PAD:PAD + L.DET_EVAL_RECORD_BYTES].copy()
    out = dict(zip(INT_SLOTS, (int(v) for v in body[:48].view(np.int64))))
    out.update(zip(F64_SLOTS, (float(v) for v in body[48:].view(np.float64))))
    return out, body.tobytes()


def _assert_record(got, want, name):
    for k in INT_SLOTS:
        assert got[k] == want[k], (name, k, got[k], want[k])
    for k in F64_SLOTS:
        diff = abs(got[k] - want[k])
        print(f"{name} {k}: kernel {got[k]!r} float64 {want[k]!r} rel {diff / abs(want[k]) if want[k] else diff:.2e}")
        assert diff <= SUM_BOUND * abs(want[k]), (name, k, got[k], want[k])
    g, w = ER.db_loss(got), ER.db_loss(want)
    assert abs(g["l_binary"] - w["l_binary"]) <= SUM_BOUND, (name, g, w)


@pytest.mark.parametrize("name", DET_CASES)
def test_det_eval_matches_float64_and_repeats_bit_for_bit(name):
    maps, want = _ref(name)
    # each case does exercise what its name says
    k, neg, pos = want["negative_count"], want["negatives"], want["positive_count"]
    if name in ("golden0", "three_pages_32x160", "two_pages_256x256"):
        assert 0 < k == 3 * pos < neg
    if name == "two_pages_256x256":
        assert maps["gt"].size > 16 * 4096           # many blocks
    if name in ("few_negatives", "golden1"):
        assert 0 < k == neg < 3 * pos
    if name == "no_positives":
        assert pos == 0 and k == 0 and want["topk_bce"] == 0.0 and want["pos_bce"] == 0.0
    if name == "every_logit_equal":
        assert 0 < k < neg
    if name == "two_loss_values":
        q = ((1 - maps["gt"]) * maps["mask"]) == 1
        hi = int((q & (maps["bin_logits"] == 2.0)).sum())
        assert 0 < hi < k < neg                      # the k-th largest lies among the equal lower losses
    if name == "fractional_gt_and_mask":
        gm = maps["gt"] * maps["mask"]
        assert ((gm > 0) & (gm < 1)).sum() >= 8
    got, bits = _run_det_eval(maps)
    _assert_record(got, want, name)
    again, bits2 = _run_det_eval(maps)
    assert bits == bits2, (name, got, again)


def test_det_eval_reads_unaligned_maps_the_same():
    maps, want = _ref("odd_size")
    got, _ = _run_det_eval(maps, shift=1)
    _assert_record(got, want, "odd_size+4B")
    maps, want = _ref("three_pages_32x160")
    got, _ = _run_det_eval(maps, shift=3)
    _assert_record(got, want, "three_pages+12B")


def test_det_eval_ratio_and_argument_checks():
    L, lib = _L()
    maps, _ = _ref("golden0")
    for ratio in (0.0, 0.5, 1e30):
        want = ER.det_eval(*[maps[k] for k in MAPS], negative_ratio=min(ratio, 1e6))
        got, _ = _run_det_eval(maps, ratio=ratio)
        assert got["negative_count"] == want["negative_count"], ratio
        assert abs(got["topk_bce"] - want["topk_bce"]) <= SUM_BOUND * want["topk_bce"]
    t = torch.zeros(64, device="cuda")
    ws = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    assert lib.ocrvi_det_eval(0, p, p, p, p, p, p, p, p, 1, 8, 8, 3.0, ws.data_ptr(), ws.data_ptr(), 1024, _stream()) == -3   # short workspace
    assert lib.ocrvi_det_eval(0, p, p, p, p, p, p, p, None, 1, 8, 8, 3.0, ws.data_ptr(), ws.data_ptr(), ws.numel(), _stream()) == -1
    assert lib.ocrvi_det_eval(0, p, p, p, p, p, p, p, p, 1, 8, 8, 3.0, ws.data_ptr(), ws.data_ptr() + 8, ws.numel() - 8, _stream()) == -1


# ---------------------------------------------------------------------------------------------- ctc_loss
def _run_ctc(lp, targets, tl, il, blank=0):
    L, lib = _L()
    T, B, Cn = lp.shape
    d_lp = torch.from_numpy(np.ascontiguousarray(lp, np.float32)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(targets, np.int32)).cuda()
    d_tl = torch.from_numpy(np.asarray(tl, np.int32)).cuda()
    d_il = None if il is None else torch.from_numpy(np.asarray(il, np.int32)).cuda()
    out = torch.full((B + 2,), -7.0, dtype=torch.float64, device="cuda")
    L.check(lib.ocrvi_ctc_loss(0, d_lp.data_ptr(), T, B, Cn, d_t.data_ptr(), targets.shape[1], d_tl.data_ptr(), L.ptr(d_il), blank,
                               out.data_ptr() + 8, _stream()))
    o = out.cpu().numpy()
    assert o[0] == -7.0 and o[-1] == -7.0
    return o[1:-1]


def _assert_nll(got, want, name):
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (name, got, want)
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print(f"{name}: nll {got} max rel {rel.max():.2e}")
    assert rel.max() <= 1e-9, (name, got, want)


@pytest.mark.parametrize("lengths", ["stored", "null"])
def test_ctc_loss_on_the_golden(lengths):
    z = np.load(os.path.join(GOLDEN, "eval_rec.npz"))
    il = z["input_lengths"] if lengths == "stored" else None
    want = ER.ctc_nll(z["log_probs"], z["targets"], z["target_lengths"], il)
    got = _run_ctc(z["log_probs"], z["targets"], z["target_lengths"], il)
    _assert_nll(got, want, f"golden/{lengths}")
    assert np.isposinf(got[5]) == (lengths == "stored")
    # and the reference's own float32 values, at its rounding
    ref = z["nll" if lengths == "stored" else "nll_full_length"]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and (np.abs(got[fin] - ref[fin]) <= 1e-6 * ref[fin]).all()


@pytest.fixture(scope="module")
def ctc_long():
    rng = np.random.default_rng(31)
    T, B, Cn = 96, 8, 232
    lens = np.array([0, 1, 5, 12, 31, 32, 33, 40], np.int32)
    lp = torch.log_softmax(torch.from_numpy(rng.normal(0, 3, (T, B, Cn)).astype(np.float32)), -1).numpy()
    targets = np.full((B, 40), 1, np.int32)
    for b, n in enumerate(lens):
        targets[b, :n] = rng.choice([2, 3, 7, 231], n)        # four labels: many adjacent repeats
    return lp, targets, lens


@pytest.mark.parametrize("lengths", ["mixed", "null"])
def test_ctc_loss_long_targets_with_repeats(ctc_long, lengths):
    lp, targets, lens = ctc_long
    assert 2 * lens.max() + 1 == 81                            # states cross a wave
    assert sum(int(targets[7, i] == targets[7, i + 1]) for i in range(39)) >= 3
    il = np.array([96, 1, 50, 10, 70, 64, 96, 81], np.int32) if lengths == "mixed" else None
    want = ER.ctc_nll(lp, targets, lens, il)
    if lengths == "mixed":
        assert np.isposinf(want[3]) and np.isfinite(np.delete(want, 3)).all()      # 12 labels on 10 steps
    else:
        assert np.isfinite(want).all()
    _assert_nll(_run_ctc(lp, targets, lens, il), want, f"long/{lengths}")


def test_ctc_loss_argument_checks():
    L, lib = _L()
    t = torch.zeros(64, device="cuda")
    i = torch.zeros(8, dtype=torch.int32, device="cuda")
    o = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.ocrvi_ctc_loss(0, t.data_ptr(), 2, 2, 8, i.data_ptr(), 2, i.data_ptr(), None, 8, o.data_ptr(), _stream()) == -1      # blank
    assert lib.ocrvi_ctc_loss(0, t.data_ptr(), 2, 2, 8, i.data_ptr(), L.CTC_LOSS_MAX_TARGET + 1, i.data_ptr(), None, 0, o.data_ptr(),
                              _stream()) == -1


# ---------------------------------------------------------------------------------------------- edit_distance
def _run_edit(pred, plen, gt, glen):
    L, lib = _L()
    B = len(plen)
    d = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in (pred, plen, gt, glen)]
    out = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    L.check(lib.ocrvi_edit_distance(0, d[0].data_ptr(), pred.shape[1], d[1].data_ptr(), d[2].data_ptr(), gt.shape[1], d[3].data_ptr(), B,
                                    out.data_ptr() + 4, _stream()))
    o = out.cpu().numpy()
    assert o[0] == -7 and o[-1] == -7
    return o[1:-1]


def test_edit_distance_is_exact():
    rng = np.random.default_rng(41)
    T, G = 140, 131
    rows = []          # (prediction ids, ground-truth ids)
    for m, n in ((0, 0), (0, 7), (7, 0), (1, 1), (63, 64), (64, 65), (65, 64), (100, 130), (130, 100), (64, 64)):
        rows.append((rng.integers(2, 6, m), rng.integers(2, 6, n)))
    same = rng.integers(2, 232, 90)
    rows.append((same, same.copy()))                                         # identical rows
    rows.append((rng.integers(2, 100, 70), rng.integers(100, 232, 80)))      # disjoint alphabets: max(m, n)
    base = rng.integers(2, 6, 60)
    sprinkled = np.insert(base, [0, 5, 5, 30, 60], [1, 0, 1, 1, 0])           # ids < 2 on the prediction side
    rows.append((sprinkled, base.copy()))
    holed = base.copy()
    holed[[3, 40]] = -2                                                      # characters outside the alphabet on the other
    rows.append((base.copy(), holed))
    rows.append((np.array([1, 1, 0, 1]), rng.integers(2, 6, 3)))             # nothing survives the filter
    B = len(rows)
    pred, gt = np.full((B, T), -1, np.int32), np.full((B, G), -1, np.int32)
    plen, glen = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (p, g) in enumerate(rows):
        pred[b, :len(p)], gt[b, :len(g)], plen[b], glen[b] = p, g, len(p), len(g)
    want = ER.edit_distance(pred, plen, gt, glen)
    assert want[0] == 0 and want[1] == 7 and want[10] == 0 and want[11] == 80 and want[12] == 0 and want[13] == 2 and want[14] == 3
    got = _run_edit(pred, plen, gt, glen)
    assert np.array_equal(got, want), (got, want)
    # ids behind a row's length are never read as part of it
    pred2 = pred.copy()
    for b in range(B):
        pred2[b, plen[b]:] = 3
    assert np.array_equal(_run_edit(pred2, plen, gt, glen), want)


# ---------------------------------------------------------------------------------------------- the loops of val.py
class _StoredMaps:
    """``DBNetPP``'s call signature over stored maps: the image carries the index of its batch."""

    def __init__(self, batches):
        self.batches = batches

    def __call__(self, x, binary_only=False):
        m = self.batches[int(x[0, 0, 0, 0])]
        return {k: torch.from_numpy(m[k]).cuda() for k in ("binary", "thresh", "thresh_binary", "bin_logits")}


def test_validate_detection_reproduces_the_reference():
    from ocr_vi_invoice_amd import DBLoss, compute_metrics, validate_detection
    z = np.load(os.path.join(GOLDEN, "eval_det.npz"))
    stored = [_golden_batch(i) for i in range(2)]
    batches = [dict(image=torch.full((2, 3, 32, 48), float(i)), gt=torch.from_numpy(m["gt"]), mask=torch.from_numpy(m["mask"]).cuda(),
                    thresh_map=torch.from_numpy(m["thresh_map"]), thresh_mask=torch.from_numpy(m["thresh_mask"]).cuda())
               for i, m in enumerate(stored)]                                # ground truth on the host and on the device
    criterion = DBLoss()
    model = _StoredMaps(stored)
    for i, b in enumerate(batches):
        loss, d = criterion(model(b["image"]), b)
        assert loss is d["loss"] and criterion.last_record["negative_count"] == int(z[f"b{i}_k"])
        for k in ("l_prob", "l_binary", "l_thresh", "loss"):
            want = float(z[f"b{i}_{k}"])
            assert abs(d[k].item() - want) <= (1e-6 if k == "l_binary" else 1e-6 * want), (i, k, d[k].item(), want)
        m = compute_metrics(model(b["image"])["binary"], b["gt"], b["mask"])
        assert m == {k: float(z[f"b{i}_{k}"]) for k in m}, m
    avg_loss, metrics = validate_detection(model, batches, criterion)
    assert abs(avg_loss - float(z["val_loss"])) <= 1e-6 * float(z["val_loss"])
    assert metrics == {k: float(z[f"val_{k}"]) for k in ("precision", "recall", "f1", "iou", "dice")}, metrics


class _StoredLogProbs:
    """``SVTRv2``'s call signature over stored log-probs."""
    blank_id = 0

    def __init__(self, lp):
        from ocr_vi_invoice_amd.vocab import Tokenizer
        self.lp, self.tokenizer = torch.from_numpy(lp).cuda(), Tokenizer()

    def __call__(self, x, targets=None):
        return self.lp


def test_validate_recognition_reproduces_the_reference_loss():
    from ocr_vi_invoice_amd import SVTRv2Loss, validate_recognition
    z = np.load(os.path.join(GOLDEN, "eval_rec.npz"))
    model = _StoredLogProbs(z["log_probs"])
    texts = model.tokenizer.decode([row[:n] for row, n in zip(z["targets"].tolist(), z["target_lengths"])])
    batch = dict(image=torch.zeros(6, 3, 32, 96), target=torch.from_numpy(z["targets"]).long(), target_length=torch.from_numpy(z["target_lengths"]),
                 input_length=torch.from_numpy(z["input_lengths"]), text=texts)
    loss, metrics = validate_recognition(model, [batch], SVTRv2Loss())
    assert abs(loss - float(z["loss_mean"])) <= 1e-6 * float(z["loss_mean"]), (loss, float(z["loss_mean"]))
    default = SVTRv2Loss()(model.lp, batch["target"]).item()                 # lengths from the pad id, every input T long
    assert abs(default - float(z["loss_mean_default"])) <= 1e-6 * float(z["loss_mean_default"])
    from oracle import svtrv2_cpu
    strings = model.tokenizer.decode(svtrv2_cpu.greedy_ids(torch.from_numpy(z["log_probs"])))    # the host greedy decode
    assert metrics == {"cer": ER.cer(strings, texts), "accuracy": ER.acc(strings, texts)}, metrics


def test_validate_recognition_end_to_end_on_tiny():
    from ocr_vi_invoice_amd import SVTRv2, SVTRv2Loss, compute_acc, compute_cer, synth, validate_recognition, weights
    model = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=3), dtype="f32", device="cuda:0")
    tok = model.tokenizer
    batches, all_lp, all_strings = [], [], []
    for i, n in enumerate((3, 2)):
        x = torch.from_numpy(synth.pad_crop_batch(synth.make_crops(5 + i, n, height=32, max_width=128), 32, 128))
        lp = model(x.cuda())
        strings = model.decode_probs(lp)
        # ground truth: the prediction itself, a corrupted copy, and a text with a character outside the alphabet
        texts = [strings[0], strings[1][1:] + "xy", "Tổng cộng: 中 12.000₫"][:n]
        enc = [tok.encode_one(t) for t in texts]                              # what the dataloader's targets hold: unknown characters dropped
        target = torch.ones(n, max(len(e) for e in enc) + 1, dtype=torch.long)
        for b, e in enumerate(enc):
            target[b, :len(e)] = torch.tensor(e, dtype=torch.long)
        lens = torch.tensor([len(e) for e in enc])
        batches.append(dict(image=x, target=target, target_length=lens, text=texts, input_length=torch.full((n,), lp.shape[0])))
        all_lp.append((lp.cpu().numpy(), target.numpy(), lens.numpy()))
        all_strings.append((strings, texts))
    loss, metrics = validate_recognition(model, batches, SVTRv2Loss())
    want_loss = np.mean([ER.ctc_loss(ER.ctc_nll(lp, t, n), n) for lp, t, n in all_lp])
    assert abs(loss - want_loss) <= 1e-9 * want_loss, (loss, want_loss)
    preds = [s for ss, _ in all_strings for s in ss]
    gts = [t for _, tt in all_strings for t in tt]
    assert metrics == {"cer": ER.cer(preds, gts), "accuracy": ER.acc(preds, gts)}, metrics
    assert metrics["accuracy"] >= 1 / 5 and metrics["cer"] > 0                # the copied prediction counts as correct, the others do not
    assert compute_cer(preds, gts) == ER.cer(preds, gts) and compute_acc(preds, gts) == ER.acc(preds, gts)
