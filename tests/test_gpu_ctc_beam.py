"""``ocrvi_ctc_beam`` against the float64 restatement of its definition (tests/ctcbeam_ref.py) on the shared case list
(tests/ctcbeam_cases.py): ids and lens exactly, score within 1e-9 relative -- the bound tests/test_gpu_eval.py holds ``ocrvi_ctc_loss`` to,
for the same reason: both sides run the same float64 recursion from the same float32 inputs.  Then the invariants with the library's own
``ocrvi_ctc_loss``, determinism, graph capture, the argument checks, the facades and the engine."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctcbeam_cases as CC  # noqa: E402
import ctcbeam_ref as BR  # noqa: E402
import ctcconf_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
I_GUARD, D_GUARD, B_GUARD = -77, 12345.0, 0xA5
REL = 1e-9


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


def _ws_bytes(T, B, C, W):
    import ctypes
    L, lib = _L()
    n = ctypes.c_size_t(0)
    L.check(lib.ocrvi_ctc_beam_workspace_bytes(T, B, C, W, ctypes.byref(n)))
    return int(n.value)


class Buffers:
    """Sentinel-filled outputs and workspace, each followed by a guard that must come back untouched."""

    def __init__(self, T, B, C, W, nbest):
        self.n_ids, self.n_row, self.n_ws = B * nbest * T, B * nbest, _ws_bytes(T, B, C, W)
        self.shape = (B, nbest, T)
        self.ids = torch.full((self.n_ids + GUARD,), I_GUARD, dtype=torch.int32, device="cuda")
        self.lens = torch.full((self.n_row + GUARD,), I_GUARD, dtype=torch.int32, device="cuda")
        self.score = torch.full((self.n_row + GUARD,), D_GUARD, dtype=torch.float64, device="cuda")
        self.ws = torch.full((self.n_ws + 4 * GUARD,), B_GUARD, dtype=torch.uint8, device="cuda")

    def args(self):
        return self.ids.data_ptr(), self.lens.data_ptr(), self.score.data_ptr(), self.ws.data_ptr(), self.n_ws

    def guards_ok(self):
        return bool((self.ids[self.n_ids:] == I_GUARD).all() and (self.lens[self.n_row:] == I_GUARD).all()
                    and (self.score[self.n_row:] == D_GUARD).all() and (self.ws[self.n_ws:] == B_GUARD).all())

    def untouched(self):
        return bool((self.ids == I_GUARD).all() and (self.lens == I_GUARD).all() and (self.score == D_GUARD).all()
                    and (self.ws == B_GUARD).all())

    def host(self):
        B, nbest, T = self.shape
        return (self.ids[:self.n_ids].cpu().numpy().reshape(B, nbest, T), self.lens[:self.n_row].cpu().numpy().reshape(B, nbest),
                self.score[:self.n_row].cpu().numpy().reshape(B, nbest))


def run_beam(y, blank, W, nbest, d=None):
    L, lib = _L()
    T, B, C = y.shape
    d = torch.from_numpy(np.ascontiguousarray(y)).cuda() if d is None else d
    buf = Buffers(T, B, C, W, nbest)
    L.check(lib.ocrvi_ctc_beam(0, d.data_ptr(), T, B, C, blank, W, nbest, *buf.args(), None))
    torch.cuda.synchronize()
    assert buf.guards_ok(), "an output or the workspace was written past its end"
    return buf.host()


def assert_equals_expected(got, want, tag):
    ids, lens, score = got
    wids, wlens, wscore = want
    assert np.array_equal(lens, wlens), (tag, lens, wlens)
    assert np.array_equal(ids, wids), (tag, np.argwhere(ids != wids)[:5])
    assert np.array_equal(np.isneginf(score), np.isneginf(wscore)), (tag, score, wscore)
    fin = np.isfinite(wscore)
    assert np.isfinite(score[fin]).all() and (np.isneginf(wscore) | fin).all()
    rel = np.abs(score[fin] - wscore[fin]) / np.maximum(np.abs(wscore[fin]), 1e-300) if fin.any() else np.zeros(1)
    exact0 = (wscore[fin] == 0.0) & (score[fin] == 0.0) if fin.any() else np.zeros(1, bool)
    rel = np.where(exact0, 0.0, rel)
    print(f"{tag}: {int(fin.sum())} hypotheses, score max rel {rel.max():.2e}")
    assert rel.max() <= REL, (tag, score, wscore)


_GOT = {}


def _got(name):
    if name not in _GOT:
        _, y, blank, W, nbest = CC.BY_NAME[name]
        _GOT[name] = run_beam(y, blank, W, nbest)
    return _GOT[name]


def _ctc_log_prob(y, blank, ids, lens):
    """-ocrvi_ctc_loss of every returned hypothesis: row b of y repeated once per hypothesis of that row.  The loss takes a NaN as it
    is, the beam search takes it as -inf: it is given the input the beam search saw."""
    L, lib = _L()
    y = np.where(np.isnan(y), np.float32(-np.inf), y)
    T, B, C = y.shape
    rows, tg, tl = [], [], []
    for b in range(B):
        for k in range(lens.shape[1]):
            if lens[b, k] >= 0:
                rows.append(b)
                tg.append(np.maximum(ids[b, k], 0))
                tl.append(lens[b, k])
    if not rows:
        return rows, np.zeros(0)
    lp = torch.from_numpy(np.ascontiguousarray(y[:, rows])).cuda()
    tgt = torch.from_numpy(np.ascontiguousarray(np.stack(tg).astype(np.int32))).cuda()
    tln = torch.from_numpy(np.asarray(tl, np.int32)).cuda()
    nll = torch.empty(len(rows), dtype=torch.float64, device="cuda")
    L.check(lib.ocrvi_ctc_loss(0, lp.data_ptr(), T, len(rows), C, tgt.data_ptr(), T, tln.data_ptr(), None, blank, nll.data_ptr(), None))
    return rows, -nll.cpu().numpy()


@pytest.mark.parametrize("name", [c[0] for c in CC.CASES])
def test_case_equals_the_reference_and_keeps_the_invariants(name):
    _, y, blank, W, nbest = CC.BY_NAME[name]
    got = _got(name)
    assert_equals_expected(got, CC.expected(name), name)
    ids, lens, score = got
    # missing hypotheses are the tail of each row; beyond a prefix everything is -1
    for b in range(y.shape[1]):
        n = int((lens[b] >= 0).sum())
        assert (lens[b, :n] >= 0).all() and (lens[b, n:] == -1).all() and (ids[b, n:] == -1).all() and np.isneginf(score[b, n:]).all()
        for k in range(n):
            assert (ids[b, k, lens[b, k]:] == -1).all() and (ids[b, k, :lens[b, k]] >= 0).all() and (ids[b, k, :lens[b, k]] != blank).all()
        assert all(score[b, k] >= score[b, k + 1] for k in range(n - 1))                       # non-increasing
        assert len({tuple(ids[b, k, :lens[b, k]]) for k in range(n)}) == n                     # no string twice
    # score is a lower bound of the labelling's probability over all alignments, and equal to it where nothing was pruned
    rows, full = _ctc_log_prob(y, blank, ids, lens)
    mine = np.array([s for b in range(y.shape[1]) for s, l in zip(score[b], lens[b]) if l >= 0])
    if len(rows):
        assert np.isfinite(full).all() and (mine <= full + REL * np.abs(full)).all(), (name, mine, full)
        if name.startswith("brute") or name == "one_hot":
            assert (np.abs(mine - full) <= REL * np.abs(full)).all(), (name, mine, full)


def test_rows_are_independent():
    """Five different rows in one launch against each launched alone, and three whose prefix tables are in the workspace; 300 copies of
    two rows (more rows than CUs)."""
    for name in ("rows5", "rows3_T140_C6_W64_workspace"):
        _, y, blank, W, nbest = CC.BY_NAME[name]
        together = _got(name)
        for b in range(y.shape[1]):
            alone = run_beam(np.ascontiguousarray(y[:, b:b + 1]), blank, W, nbest)
            assert all(np.array_equal(a[0], t[b]) and a[0].tobytes() == t[b].tobytes() for a, t in zip(alone, together)), (name, b)
    _, g, gblank, _, _ = CC.BY_NAME["golden_W8"]
    two = run_beam(g, gblank, 8, 4)
    many = run_beam(np.ascontiguousarray(np.tile(g, (1, 150, 1))), gblank, 8, 4)
    for b in range(300):
        assert all(np.array_equal(m[b], t[b % 2]) for m, t in zip(many, two)), b


def test_two_launches_and_a_graph_replay_give_the_same_bytes():
    L, lib = _L()
    _, y, blank, W, nbest = CC.BY_NAME["T80_C232_s6_W64"]
    T, B, C = y.shape
    d = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    first = run_beam(y, blank, W, nbest, d)
    second = run_beam(y, blank, W, nbest, d)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    buf = Buffers(T, B, C, W, nbest)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        L.check(lib.ocrvi_ctc_beam(0, d.data_ptr(), T, B, C, blank, W, nbest, *buf.args(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert buf.untouched()                                              # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert buf.guards_ok() and all(a.tobytes() == b.tobytes() for a, b in zip(buf.host(), first))
    buf.ids.fill_(I_GUARD), buf.lens.fill_(I_GUARD), buf.score.fill_(D_GUARD)
    g.replay()
    torch.cuda.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(buf.host(), first))


def test_argument_checks_leave_the_outputs_untouched():
    L, lib = _L()
    T, B, C, W, nbest = 12, 2, 4, 4, 2
    d = torch.from_numpy(np.ascontiguousarray(CC.BY_NAME["rows5"][1][:, :2])).cuda()
    buf = Buffers(T, B, C, W, nbest)
    ids, lens, score, ws, nws = buf.args()
    ok = dict(lp=d.data_ptr(), T=T, B=B, C=C, blank=0, W=W, nbest=nbest, ids=ids, lens=lens, score=score, ws=ws, nws=nws)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ocrvi_ctc_beam(0, a["lp"], a["T"], a["B"], a["C"], a["blank"], a["W"], a["nbest"], a["ids"], a["lens"], a["score"], a["ws"],
                                  a["nws"], None)

    bad = [dict(nbest=0), dict(nbest=W + 1), dict(W=0, nbest=1), dict(W=65), dict(C=1), dict(C=1025), dict(blank=-1), dict(blank=C), dict(T=0),
           dict(T=1025), dict(B=0), dict(lp=None), dict(ids=None), dict(lens=None), dict(score=None), dict(ws=None), dict(ws=ws + 8)]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # OCRVI_EINVAL
        assert L.last_error(), kw
    assert call(nws=nws - 1) == -3 and call(nws=0) == -3                # OCRVI_ENOMEM
    torch.cuda.synchronize()
    assert buf.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert buf.guards_ok() and not buf.untouched()


# ---------------------------------------------------------------------------------------------------- the facades
@pytest.fixture(scope="module")
def model():
    from ocr_vi_invoice_amd import SVTRv2
    return SVTRv2("tiny", dtype="f16x2")


def test_decode_probs_with_beam(model):
    from ocr_vi_invoice_amd.rec import Hypothesis, make_hypotheses
    _, y, blank, _, _ = CC.BY_NAME["golden_W8"]
    assert blank == model.blank_id and y.shape[2] == model.tokenizer.num_classes
    d = torch.from_numpy(y).cuda()
    got = model.decode_probs(d, beam=8, nbest=4)
    want = make_hypotheses(model.tokenizer, *BR.outputs(CC.reference("golden_W8")[0], y.shape[0], 4))
    assert len(got) == 2 and all(len(r) == 4 and all(isinstance(h, Hypothesis) for h in r) for r in got)
    for g, w in zip(got, want):
        assert [(h.text, h.ids) for h in g] == [(h.text, h.ids) for h in w]
        assert all(abs(a.log_prob - b.log_prob) <= REL * abs(b.log_prob) for a, b in zip(g, w))
    # (on these flat random-weight rows the best reading is not the greedy string, and a wider beam finds a better one)
    wide = model.decode_probs(d, beam=64, nbest=1)
    assert [r[0].ids for r in wide] == [r[0][0] for r in CC.reference("golden_W64")[0]]
    assert all(w[0].log_prob > g[0].log_prob for w, g in zip(wide, got))
    # rows with fewer hypotheses than nbest, and with none
    hard = np.stack([CC.BY_NAME[n][1][:, 0] for n in ("one_hot", "dead_step")], 1)
    lp = np.full((6, 2, y.shape[2]), -np.inf, np.float32)
    lp[:, :, :5] = hard
    out = model.decode_probs(torch.from_numpy(lp).cuda(), beam=4, nbest=4)
    assert [len(r) for r in out] == [1, 0] and out[0][0].ids == (2, 3) and out[0][0].log_prob == 0.0
    # the class count is the tensor's, as it is for the greedy decode
    assert model.decode_probs(torch.from_numpy(np.ascontiguousarray(hard)).cuda(), beam=4, nbest=4) == out


def test_decode_probs_without_beam_is_the_parents(model):
    L, lib = _L()
    y = CR.random_peaked(np.random.default_rng(9), 70, 5, 232)
    d = torch.from_numpy(y).cuda()
    am, ids, lens = (torch.empty((5, 70), dtype=torch.int32, device="cuda"), torch.empty((5, 70), dtype=torch.int32, device="cuda"),
                     torch.empty(5, dtype=torch.int32, device="cuda"))
    L.check(lib.ocrvi_ctc_greedy(0, d.data_ptr(), 70, 5, 232, model.blank_id, am.data_ptr(), ids.data_ptr(), lens.data_ptr(), None))
    want = model.tokenizer.decode([r[:n] for r, n in zip(ids.cpu().tolist(), lens.cpu().tolist())])
    assert model.decode_probs(d) == want == model.decode_probs(d, beam=None, nbest=3)
    ref = CR.greedy_conf(y)
    recs = model.decode_probs(d, return_confidence=True)
    wrec = CR.recognitions(model.tokenizer.id_to_token, ref["ids"], ref["lens"], ref["char_lp"], ref["char_span"])
    assert [(r.text, r.score, r.char_scores, r.spans) for r in recs] == [w[:4] for w in wrec] and [r.text for r in recs] == want


def test_beam_value_errors(model):
    d = torch.zeros((8, 1, 232), device="cuda")
    x = torch.zeros((1, 3, 32, 64), device="cuda")
    for kw in (dict(beam=0), dict(beam=65), dict(beam=4, nbest=5), dict(beam=4, nbest=0), dict(beam=4, return_confidence=True)):
        with pytest.raises(ValueError):
            model.decode_probs(d, **kw)
        with pytest.raises(ValueError):
            model.decode_greedy(x, **kw)
    with pytest.raises(ValueError):
        model.decode_probs(torch.zeros((1025, 1, 232)), beam=4)        # a host tensor: refused before it is moved
    from ocr_vi_invoice_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.recognize_text_batch(model, [np.zeros((8, 8, 3), np.uint8)], beam=4, return_confidence=True)


def test_decode_greedy_with_beam_and_recognize_text_batch(model):
    from ocr_vi_invoice_amd import pipeline, synth
    crops = synth.make_crops(5, 3, height=32, max_width=128)
    x = torch.from_numpy(synth.pad_crop_batch(crops, 32, 128)).cuda()
    lp = model(x)
    want = model.decode_probs(lp, beam=4, nbest=2)
    assert model.decode_greedy(x, beam=4, nbest=2) == want and all(1 <= len(r) <= 2 for r in want)
    texts, hyps = model.decode_greedy_and_beam(x, 4, 2)
    assert texts == model.decode_greedy(x) and hyps == want
    recs, hyps = model.decode_greedy_and_beam(x, 4, 2, return_confidence=True)
    assert [tuple(r) for r in recs] == [tuple(r) for r in model.decode_greedy(x, True)] and hyps == want
    batch = pipeline.recognize_text_batch(model, crops, img_size=(32, 128), batch_size=2, beam=4, nbest=2)
    alone = [pipeline.recognize_text_batch(model, [c], img_size=(32, 128), beam=4, nbest=2)[0] for c in crops]
    assert batch == alone and len(batch) == 3


# ---------------------------------------------------------------------------------------------------- the engine
DET_SIZE = 256
SIZES = [(400, 640), (480, 480), (400, 640)]            # three small pages of two detector shapes: 160x256 twice, 256x256


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)


class _Pages:
    """The pages and, per page, the rendered text kernel at its detector shape (tests/test_gpu_engine.py: kernel + 0.25 binary)."""

    def __init__(self):
        from ocr_vi_invoice_amd import synth
        from ocr_vi_invoice_amd.engine import plan_buckets
        self.pages, self.kern, self.page = [], [], 0
        shapes, scales, _ = plan_buckets(SIZES, DET_SIZE)
        for k, ((h, w), (H, W), (sh, sw)) in enumerate(zip(SIZES, shapes, scales)):
            img, boxes = synth.make_invoice(31 + k, h, w, lines=5)
            self.pages.append(img)
            m = np.zeros((1, H, W), np.float32)
            for x, y, bw, bh in boxes:
                x0, x1, y0, y1 = int(x * sw) + 2, int((x + bw) * sw) - 2, int(y * sh) + 1, int((y + bh) * sh) - 1
                if x1 - x0 >= 3 and y1 - y0 >= 2:
                    m[0, y0:y1, x0:x1] = 0.75
            self.kern.append(torch.from_numpy(m).cuda())

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


def test_engine_with_beam():
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, pipeline, weights
    from ocr_vi_invoice_amd.rec import Hypothesis, Recognition
    data = _Pages()
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=2, rec_batch=8, prob_hook=data.hook)
    plain = Engine(det, rec, _pp(), **kw).run(data.pages)
    assert all(len(r) == 3 for r in plain) and sum(len(r[0]) for r in plain) > 8         # more crops than one recogniser batch

    class Blended:                                                       # the page alone sees the map the hook gives the engine
        def __call__(self, x):
            return {"binary": torch.add(data.kern[data.page][None], det(x)["binary"], alpha=0.25)}

    alone = []
    for i, p in enumerate(data.pages):
        data.page = i
        alone.append(pipeline.detect_and_recognize(p, Blended(), rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), beam=4, nbest=2))
    for conf in (False, True):
        eng = Engine(det, rec, _pp(), beam=4, nbest=2, confidence=conf, **kw)
        for _ in range(2):                                              # the second run replays the captured graph
            got = eng.run(data.pages)
            assert all(len(r) == (5 if conf else 4) for r in got)
            for g, w, a in zip(got, plain, alone):
                assert len(g[0]) == len(w[0]) and all(np.array_equal(x, y) for x, y in zip(g[0], w[0]))
                assert g[1] == w[1] and g[2] == w[2]                    # boxes, scores and texts are the plain engine's
                assert a[2] == w[2] and len(a) == 4
                assert len(g[-1]) == len(g[2]) and g[-1] == a[3]        # the hypotheses of the same crops, page alone
                assert all(isinstance(h, Hypothesis) for hs in g[-1] for h in hs) and all(1 <= len(hs) <= 2 for hs in g[-1])
                if conf:
                    assert all(isinstance(r, Recognition) for r in g[3]) and [r.text for r in g[3]] == g[2]
    data.page = 0
    both = pipeline.detect_and_recognize(data.pages[0], Blended(), rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), beam=4, nbest=2,
                                         confidence=True)
    assert len(both) == 5 and both[4] == alone[0][3] and both[2] == alone[0][2]
    assert Engine(det, rec, _pp(), beam=4, nbest=2, **kw).run([]) == []
    with pytest.raises(ValueError):
        Engine(det, rec, _pp(), beam=2, nbest=3, **kw)
