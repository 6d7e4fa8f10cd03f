"""The confidence kernels against tests/ctcconf_ref.py, every output by exact equality (floats by bit pattern): ``ocrvi_ctc_greedy_conf`` on
constructed and seeded rows over the shapes where the collapse changes path (pass boundaries at 64 steps, four waves per workgroup),
``ocrvi_test_ctc_logsoftmax_conf`` against the parent's ``ocrvi_test_ctc_logsoftmax``, ``ocrvi_rec_forward_conf`` against
``ocrvi_rec_forward``, and ``decode_probs(return_confidence=True)`` against the float64 CTC forward of tests/eval_refs.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctcconf_ref as CR  # noqa: E402
import eval_refs as ER  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
I_GUARD, F_GUARD = -77, 12345.0


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _buf(n, dtype):
    """n elements followed by GUARD sentinel elements that must come back untouched."""
    return torch.full((n + GUARD,), I_GUARD if dtype == torch.int32 else F_GUARD, dtype=dtype, device="cuda")


def _tail_ok(t, n):
    return bool((t[n:] == (I_GUARD if t.dtype == torch.int32 else F_GUARD)).all())


def run_greedy_conf(lp, blank):
    L, lib = _L()
    T, B, C = lp.shape
    d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    am, ids, lens = _buf(B * T, torch.int32), _buf(B * T, torch.int32), _buf(B, torch.int32)
    blp, clp, span = _buf(B * T, torch.float32), _buf(B * T, torch.float32), _buf(B * T * 2, torch.int32)
    L.check(lib.ocrvi_ctc_greedy_conf(0, d.data_ptr(), T, B, C, blank, am.data_ptr(), ids.data_ptr(), lens.data_ptr(), blp.data_ptr(),
                                      clp.data_ptr(), span.data_ptr(), None))
    torch.cuda.synchronize()
    for t, n in ((am, B * T), (ids, B * T), (lens, B), (blp, B * T), (clp, B * T), (span, 2 * B * T)):
        assert _tail_ok(t, n), "an output was written past its end"
    # and the parent's entry on the same rows: argmax, ids and lens must be exactly its
    am0, ids0, lens0 = _buf(B * T, torch.int32), _buf(B * T, torch.int32), _buf(B, torch.int32)
    L.check(lib.ocrvi_ctc_greedy(0, d.data_ptr(), T, B, C, blank, am0.data_ptr(), ids0.data_ptr(), lens0.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(am, am0) and torch.equal(ids, ids0) and torch.equal(lens, lens0)
    h = lambda t, n, shape: t[:n].cpu().numpy().reshape(shape)  # noqa: E731
    return {"argmax": h(am, B * T, (B, T)), "ids": h(ids, B * T, (B, T)), "lens": h(lens, B, (B,)), "best_lp": h(blp, B * T, (B, T)),
            "char_lp": h(clp, B * T, (B, T)), "char_span": h(span, 2 * B * T, (B, T, 2))}


def assert_equals_ref(got, lp, blank, tag):
    want = CR.greedy_conf(lp, blank)
    for k in ("argmax", "ids", "lens", "char_span"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    for k in ("best_lp", "char_lp"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k, got[k], want[k])
    return want


@pytest.mark.parametrize("C", [3, 64, 65, 232])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 200])
def test_greedy_conf_on_constructed_and_seeded_rows(T, C):
    """Every constructed row that fits T steps, with blank 0 and with blank 2 (id 0 a character: a NaN row then lies inside a run), plus
    seeded peaked rows, cut into batches of 1, 3, 4, 5 and 9 rows (four waves per workgroup: full and ragged last groups)."""
    rng = np.random.default_rng(1000 * T + C)
    seen_lens_T = False
    for blank in (0, 2):
        cs = CR.cases(T, C, blank)
        rows = np.stack(list(cs.values()) + list(CR.random_peaked(rng, T, 6, C, blank).transpose(1, 0, 2)), 1)     # [T, n, C]
        names = list(cs) + ["seeded"] * 6
        lo, sizes = 0, [1, 3, 4, 5, 9]
        while lo < rows.shape[1]:
            B = sizes[(lo + T) % 5]
            chunk = rows[:, lo:lo + B]
            if chunk.shape[1] < B:                                      # the last batch: filled up from the start, so B stays in the set
                chunk = np.concatenate([chunk, rows[:, :B - chunk.shape[1]]], 1)
            chunk = np.ascontiguousarray(chunk)
            want = assert_equals_ref(run_greedy_conf(chunk, blank), chunk, blank, (T, C, blank, names[lo:lo + B]))
            seen_lens_T |= bool((want["lens"] == T).any())
            lo += B
    assert seen_lens_T                                                  # strict alternation: as many characters as steps


def test_greedy_conf_named_rows():
    """The rows the carry exists for, stated as numbers, on the device."""
    c = CR.cases(200, 65)
    lp = np.ascontiguousarray(np.stack([c["one_char_all_steps_max_last"], c["run_62_66_max_boundary_64"], c["run_crosses_two_boundaries"],
                                        c["run_ends_63_next_starts_64"], c["all_blank"]], 1))
    got = run_greedy_conf(lp, 0)
    assert got["lens"].tolist() == [1, 1, 1, 2, 0]
    assert got["char_span"][0, 0].tolist() == [0, 199] and got["char_lp"][0, 0] == np.float32(-0.5)
    assert got["char_span"][1, 0].tolist() == [62, 66] and got["char_lp"][1, 0] == np.float32(-0.0625)
    assert got["char_span"][2, 0].tolist() == [60, 129] and got["char_lp"][2, 0] == np.float32(-0.0625)
    assert got["char_span"][3, :2].tolist() == [[60, 63], [64, 64]] and got["char_lp"][3, 0] == np.float32(-0.1)
    assert (got["char_span"][4] == -1).all() and np.isneginf(got["char_lp"][4]).all()
    assert_equals_ref(got, lp, 0, "named")
    # a run of nothing but NaN is a character when id 0 is one: its record is that NaN
    lp = np.ascontiguousarray(CR.cases(130, 5, 2)["all_nan"][:, None, :])
    got = run_greedy_conf(lp, 2)
    assert got["lens"].tolist() == [1] and got["char_span"][0, 0].tolist() == [0, 129] and np.isnan(got["char_lp"][0, 0])
    assert_equals_ref(got, lp, 2, "all NaN")


def test_greedy_conf_optional_outputs_and_argument_checks():
    L, lib = _L()
    lp = np.ascontiguousarray(CR.random_peaked(np.random.default_rng(2), 70, 5, 9))
    full = run_greedy_conf(lp, 0)
    d = torch.from_numpy(lp).cuda()
    am, blp, clp = _buf(350, torch.int32), _buf(350, torch.float32), _buf(350, torch.float32)
    L.check(lib.ocrvi_ctc_greedy_conf(0, d.data_ptr(), 70, 5, 9, 0, am.data_ptr(), None, None, blp.data_ptr(), clp.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(clp[:350].cpu().numpy().reshape(5, 70)), _bits(full["char_lp"])) and _tail_ok(clp, 350)
    assert np.array_equal(_bits(blp[:350].cpu().numpy().reshape(5, 70)), _bits(full["best_lp"]))
    L.check(lib.ocrvi_ctc_greedy_conf(0, d.data_ptr(), 70, 5, 9, 0, am.data_ptr(), None, None, blp.data_ptr(), None, None, None))
    for bad in ((None, am.data_ptr(), blp.data_ptr()), (d.data_ptr(), None, blp.data_ptr()), (d.data_ptr(), am.data_ptr(), None)):
        assert lib.ocrvi_ctc_greedy_conf(0, bad[0], 70, 5, 9, 0, bad[1], None, None, bad[2], None, None, None) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the fused head
def _crafted_logits(rng, B, T, C, ld):
    x = rng.normal(0, 3, (B * T, ld)).astype(np.float32)
    n = B * T
    x[0, : C] = 0.25                                                    # every class equal: first index
    if n > 1:
        x[1, C - 1] = x[1, 0] = 50.0                                    # two equal maxima
    if n > 2:
        x[2, C // 2] = np.nan                                           # NaN logit -> NaN row
    if n > 3:
        x[3, 0] = np.inf                                                # +inf logit -> NaN row
    if n > 4:
        x[4, :C] = -np.inf                                              # nothing but -inf -> NaN row
    if n > 5:
        x[5, :C] = -np.inf
        x[5, C - 1] = 0.0                                               # one finite class: log-prob 0
    x[:, C:] = 1e30                                                     # columns C..ld-1 are never read
    return x


@pytest.mark.parametrize("B,T,C,pad", [(1, 1, 3, 0), (3, 5, 64, 0), (5, 65, 65, 3), (9, 7, 232, 0), (2, 3, 1024, 0), (4, 200, 232, 8)])
def test_logsoftmax_conf_kernel(B, T, C, pad):
    """log_probs and argmax_ids bit-equal to the parent's kernel; best_lp the gather of those log-probs at the reference argmax of them."""
    L, lib = _L()
    x = _crafted_logits(np.random.default_rng(B * 131 + T * 7 + C), B, T, C, C + pad)
    d = torch.from_numpy(x).cuda()
    lp0, am0 = _buf(T * B * C, torch.float32), _buf(B * T, torch.int32)
    L.check(lib.ocrvi_test_ctc_logsoftmax(0, d.data_ptr(), C + pad, B, T, C, lp0.data_ptr(), am0.data_ptr()))
    lp1, am1, blp = _buf(T * B * C, torch.float32), _buf(B * T, torch.int32), _buf(B * T, torch.float32)
    L.check(lib.ocrvi_test_ctc_logsoftmax_conf(0, d.data_ptr(), C + pad, B, T, C, lp1.data_ptr(), am1.data_ptr(), blp.data_ptr()))
    assert torch.equal(lp0.view(torch.int32), lp1.view(torch.int32)) and torch.equal(am0, am1)
    assert _tail_ok(blp, B * T) and _tail_ok(lp1, T * B * C) and _tail_ok(am1, B * T)
    lp = lp1[:T * B * C].cpu().numpy().reshape(T, B, C)
    am, best = CR.argmax_rows(lp)
    assert np.array_equal(am, am1[:B * T].cpu().numpy().reshape(B, T))
    got = blp[:B * T].cpu().numpy().reshape(B, T)
    assert np.array_equal(_bits(got), _bits(best)), (got, best)
    if B * T > 5:
        flat = got.reshape(-1)                                          # row = b * T + t
        assert np.isnan(flat[2:5]).all() and flat[5] == 0.0 and flat[0] == np.float32(lp.transpose(1, 0, 2).reshape(-1, C)[0, 0])
    # without the log-probs (what the engine asks for) and without the argmax: best_lp does not change
    blp2 = _buf(B * T, torch.float32)
    L.check(lib.ocrvi_test_ctc_logsoftmax_conf(0, d.data_ptr(), C + pad, B, T, C, None, None, blp2.data_ptr()))
    assert torch.equal(blp.view(torch.int32), blp2.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- the recogniser entry
@pytest.fixture(scope="module")
def crops():
    from ocr_vi_invoice_amd import synth
    return torch.from_numpy(synth.pad_crop_batch(synth.make_crops(5, 2, height=32, max_width=128), 32, 128)).cuda()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_rec_forward_conf_equals_rec_forward(crops, dtype):
    from ocr_vi_invoice_amd import SVTRv2, weights
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=3), dtype=dtype)
    B, _, H, W = crops.shape
    T, C = W // 4, rec.tokenizer.num_classes
    st = torch.cuda.current_stream().cuda_stream
    ws = rec._workspace(B, H, W)

    def parent():
        lp, am, ids, lens = _buf(T * B * C, torch.float32), _buf(B * T, torch.int32), _buf(B * T, torch.int32), _buf(B, torch.int32)
        rec.enqueue_forward(crops.data_ptr(), B, H, W, lp.data_ptr(), am.data_ptr(), ids.data_ptr(), lens.data_ptr(), ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        return lp, am, ids, lens

    def conf(with_lp, with_best):
        lp, am, ids, lens = _buf(T * B * C, torch.float32), _buf(B * T, torch.int32), _buf(B * T, torch.int32), _buf(B, torch.int32)
        blp, clp, span = _buf(B * T, torch.float32), _buf(B * T, torch.float32), _buf(2 * B * T, torch.int32)
        rec.enqueue_forward_conf(crops.data_ptr(), B, H, W, lp.data_ptr() if with_lp else None, am.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                 blp.data_ptr() if with_best else None, clp.data_ptr(), span.data_ptr(), ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        return lp, am, ids, lens, blp, clp, span

    want = parent()
    got = conf(True, True)
    for a, b in zip(got[:4], want):                                     # the four shared outputs, guards included
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    lp = got[0][:T * B * C].cpu().numpy().reshape(T, B, C)
    am = got[1][:B * T].cpu().numpy().reshape(B, T)
    best = np.take_along_axis(lp.transpose(1, 0, 2), am[..., None].astype(np.int64), -1)[..., 0]
    assert np.array_equal(_bits(got[4][:B * T].cpu().numpy().reshape(B, T)), _bits(best))
    ids, lens, clp, span = CR.collapse_conf(am, best, rec.blank_id)
    assert np.array_equal(ids, got[2][:B * T].cpu().numpy().reshape(B, T)) and np.array_equal(lens, got[3][:B].cpu().numpy())
    assert np.array_equal(_bits(clp), _bits(got[5][:B * T].cpu().numpy().reshape(B, T)))
    assert np.array_equal(span, got[6][:2 * B * T].cpu().numpy().reshape(B, T, 2))
    assert all(_tail_ok(t, n) for t, n in zip(got[4:], (B * T, B * T, 2 * B * T)))
    # the engine's form: no log-probs, no best_lp -- the records do not change, nothing is written where NULL was passed
    lean = conf(False, False)
    assert bool((lean[0] == F_GUARD).all()) and bool((lean[4] == F_GUARD).all())
    for k in (1, 2, 3, 5, 6):
        assert torch.equal(lean[k].view(torch.int32), got[k].view(torch.int32)), k
    assert rec.check_range() is None
    # the facade: the same strings, scores from the records, log_prob of the float64 forward
    texts = rec.decode_greedy(crops)
    recs = rec.decode_greedy(crops, return_confidence=True)
    want_recs = CR.recognitions(rec.tokenizer.id_to_token, ids, lens, clp, span)
    assert [r.text for r in recs] == texts == [w[0] for w in want_recs]
    assert [(r.score, r.char_scores, r.spans) for r in recs] == [w[1:4] for w in want_recs]
    _assert_log_prob([r.log_prob for r in recs], lp, ids, lens, dtype)


def _assert_log_prob(got, lp, ids, lens, tag):
    """-ocrvi_ctc_loss against the float64 recursion of tests/eval_refs.py, at the bar tests/test_gpu_eval.py holds it to: relative 1e-9."""
    want = -ER.ctc_nll(lp, ids, lens)
    got = np.asarray(got, np.float64)
    assert np.isfinite(want).all() and np.isfinite(got).all(), (tag, got, want)
    rel = np.abs(got - want) / np.abs(want)
    print(f"{tag}: log_prob {got} max rel {rel.max():.2e}")
    assert rel.max() <= 1e-9, (tag, got, want)


def test_decode_probs_with_confidence():
    from ocr_vi_invoice_amd import SVTRv2
    from ocr_vi_invoice_amd.rec import Recognition
    m = SVTRv2("tiny", dtype="bf16")
    rng = np.random.default_rng(9)
    T, B, C = 70, 5, 232
    lp = CR.random_peaked(rng, T, B, C)
    lp[:, 4] = np.log(np.float32(1 / C))                                # every class equal: blank everywhere, an empty string
    lp[3::7, 3, :] = -20.0
    lp[3::7, 3, 1] = -0.001                                             # pad id 1 on the greedy path of row 3: dropped on the host
    d = torch.from_numpy(lp).cuda()
    texts = m.decode_probs(d)
    recs = m.decode_probs(d, return_confidence=True)
    assert all(isinstance(r, Recognition) for r in recs) and [r.text for r in recs] == texts
    ref = CR.greedy_conf(lp)
    assert (ref["ids"][3] == 1).sum() >= 5
    want = CR.recognitions(m.tokenizer.id_to_token, ref["ids"], ref["lens"], ref["char_lp"], ref["char_span"])
    assert [(r.text, r.score, r.char_scores, r.spans) for r in recs] == [w[:4] for w in want]
    for r in recs:
        assert len(r.text) == len(r.char_scores) == len(r.spans)
        assert r.score == (math.fsum(r.char_scores) / len(r.char_scores) if r.text else 0.0)
    assert recs[4].text == "" and recs[4].score == 0.0
    _assert_log_prob([r.log_prob for r in recs], lp, ref["ids"], ref["lens"], "decode_probs")
    assert all(r.log_prob <= 0 for r in recs)
    # the known-answer paths and the multi-pass collapse of tests/test_gpu_models.py, now with spans
    long = torch.full((200, 2, 232), -5.0)
    long[::2, 0, 70] = 0.0
    long[1::2, 0, 0] = 0.0
    long[:, 1, 71] = -0.5
    long[131, 1, 71] = -0.25
    out = m.decode_probs(long, return_confidence=True)
    assert out[0].text == m.tokenizer.id_to_token[70] * 100 and out[0].spans == tuple((t, t) for t in range(0, 200, 2))
    assert out[0].char_scores == (1.0,) * 100 and out[0].score == 1.0
    assert out[1].text == m.tokenizer.id_to_token[71] and out[1].spans == ((0, 199),) and out[1].char_scores == (math.exp(-0.25),)
