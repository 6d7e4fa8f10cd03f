"""``ocrvi_ctc_beam_lm`` against the float64 restatement of its definition (tests/ctclm_ref.py) on the shared case list
(tests/ctclm_cases.py): ids and lens exactly, the three scores within 1e-9 relative (the bound tests/test_gpu_ctc_beam.py holds
``ocrvi_ctc_beam`` to: both sides run the same float64 recursion from the same float32 inputs) and ``lm_score`` bit for bit (sums of the same
doubles in the same order, no transcendental).  Then brute force, byte equality with ``ocrvi_ctc_beam`` at alpha = beta = 0, the
invariants, determinism, graph capture, the argument checks, the facades and the engine."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctcbeam_cases as CC  # noqa: E402
import ctclm_cases as LC  # noqa: E402
import ctclm_ref as LR  # noqa: E402
import test_gpu_ctc_beam as TB  # noqa: E402  (run_beam, the guarded buffers' constants, -ocrvi_ctc_loss of hypotheses, the engine's pages)

pytestmark = pytest.mark.gpu

GUARD, I_GUARD, D_GUARD, B_GUARD, REL = TB.GUARD, TB.I_GUARD, TB.D_GUARD, TB.B_GUARD, TB.REL


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


_HANDLES = {}


def handle(t: LR.Table):
    """A device handle of the REFERENCE's blob (the library's own builder is held to it on the CPU)."""
    if id(t) not in _HANDLES:
        L, lib = _L()
        h, blob = ctypes.c_void_p(), t.blob()
        L.check(lib.ocrvi_lm_create(0, blob, len(blob), ctypes.byref(h)))
        _HANDLES[id(t)] = (h, t)
    return _HANDLES[id(t)][0]


def _ws_bytes(T, B, C, W):
    L, lib = _L()
    n = ctypes.c_size_t(0)
    L.check(lib.ocrvi_ctc_beam_lm_workspace_bytes(T, B, C, W, ctypes.byref(n)))
    return int(n.value)


class Buffers:
    """Sentinel-filled outputs and workspace, each followed by a guard that must come back untouched."""

    def __init__(self, T, B, C, W, nbest):
        self.n_ids, self.n_row, self.n_ws = B * nbest * T, B * nbest, _ws_bytes(T, B, C, W)
        self.shape = (B, nbest, T)
        self.ids = torch.full((self.n_ids + GUARD,), I_GUARD, dtype=torch.int32, device="cuda")
        self.lens = torch.full((self.n_row + GUARD,), I_GUARD, dtype=torch.int32, device="cuda")
        self.scores = [torch.full((self.n_row + GUARD,), D_GUARD, dtype=torch.float64, device="cuda") for _ in range(3)]
        self.ws = torch.full((self.n_ws + 4 * GUARD,), B_GUARD, dtype=torch.uint8, device="cuda")

    def args(self):
        return (self.ids.data_ptr(), self.lens.data_ptr(), *[s.data_ptr() for s in self.scores], self.ws.data_ptr(), self.n_ws)

    def guards_ok(self):
        return bool((self.ids[self.n_ids:] == I_GUARD).all() and (self.lens[self.n_row:] == I_GUARD).all()
                    and all((s[self.n_row:] == D_GUARD).all() for s in self.scores) and (self.ws[self.n_ws:] == B_GUARD).all())

    def untouched(self):
        return bool((self.ids == I_GUARD).all() and (self.lens == I_GUARD).all() and all((s == D_GUARD).all() for s in self.scores)
                    and (self.ws == B_GUARD).all())

    def host(self):
        B, nbest, T = self.shape
        return (self.ids[:self.n_ids].cpu().numpy().reshape(B, nbest, T), self.lens[:self.n_row].cpu().numpy().reshape(B, nbest),
                *[s[:self.n_row].cpu().numpy().reshape(B, nbest) for s in self.scores])


def run_beam_lm(y, blank, W, nbest, t: LR.Table, alpha, beta, d=None):
    L, lib = _L()
    T, B, C = y.shape
    d = torch.from_numpy(np.ascontiguousarray(y)).cuda() if d is None else d
    buf = Buffers(T, B, C, W, nbest)
    L.check(lib.ocrvi_ctc_beam_lm(0, d.data_ptr(), T, B, C, blank, W, nbest, handle(t), alpha, beta, *buf.args(), None))
    torch.cuda.synchronize()
    assert buf.guards_ok(), "an output or the workspace was written past its end"
    return buf.host()


def _rel(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.isfinite(got[fin]).all() and (np.isneginf(want) | fin).all(), (got, want)
    if not fin.any():
        return 0.0
    rel = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
    return float(np.where((want[fin] == 0.0) & (got[fin] == 0.0), 0.0, rel).max())


def assert_equals_expected(got, want, tag):
    ids, lens, score, ctc, lms = got
    wids, wlens, wscore, wctc, wlms = want
    assert np.array_equal(lens, wlens), (tag, lens, wlens)
    assert np.array_equal(ids, wids), (tag, np.argwhere(ids != wids)[:5])
    rels = [_rel(score, wscore), _rel(ctc, wctc), _rel(lms, wlms)]
    print(f"{tag}: {int((wlens >= 0).sum())} hypotheses, max rel score {rels[0]:.2e} ctc {rels[1]:.2e} lm {rels[2]:.2e}")
    assert max(rels) <= REL, (tag, rels)
    assert lms.tobytes() == wlms.tobytes(), (tag, lms, wlms)             # bit-equal


_GOT = {}


def _got(name):
    if name not in _GOT:
        _, y, blank, W, nbest, tname, alpha, beta = LC.BY_NAME[name]
        _GOT[name] = run_beam_lm(y, blank, W, nbest, LC.table(tname), alpha, beta)
    return _GOT[name]


@pytest.mark.parametrize("name", [c[0] for c in LC.CASES])
def test_case_equals_the_reference_and_keeps_the_invariants(name):
    _, y, blank, W, nbest, tname, alpha, beta = LC.BY_NAME[name]
    got = _got(name)
    assert_equals_expected(got, LC.expected(name), name)
    ids, lens, score, ctc, lms = got
    for b in range(y.shape[1]):
        n = int((lens[b] >= 0).sum())
        assert (lens[b, :n] >= 0).all() and (lens[b, n:] == -1).all() and (ids[b, n:] == -1).all()
        assert all(np.isneginf(a[b, n:]).all() for a in (score, ctc, lms))                      # missing hypotheses are the tail
        for k in range(n):
            assert (ids[b, k, lens[b, k]:] == -1).all() and (ids[b, k, :lens[b, k]] >= 0).all() and (ids[b, k, :lens[b, k]] != blank).all()
        assert all(score[b, k] >= score[b, k + 1] for k in range(n - 1))                        # non-increasing
        assert len({tuple(ids[b, k, :lens[b, k]]) for k in range(n)}) == n                      # no string twice
    # ctc_score is a lower bound of the labelling's probability over all alignments, and equal to it where nothing was pruned
    rows, full = TB._ctc_log_prob(y, blank, ids, lens)
    mine = np.array([s for b in range(y.shape[1]) for s, l in zip(ctc[b], lens[b]) if l >= 0])
    if len(rows):
        assert np.isfinite(full).all() and (mine <= full + REL * np.abs(full)).all(), (name, mine, full)
        if name.startswith("brute") or name == "one_hot_lm":
            assert (np.abs(mine - full) <= REL * np.abs(full)).all(), (name, mine, full)


@pytest.mark.parametrize("name", [c[0] for c in LC.CASES if c[0].startswith("brute")])
def test_brute_force(name):
    """Nothing is pruned: every labelling comes back, R equal to brute force's within 1e-9, lm_score bit-equal to g(l)."""
    _, y, blank, W, nbest, tname, alpha, beta = LC.BY_NAME[name]
    want = LR.brute_lm(y[:, 0], blank, LC.table(tname), alpha, beta)
    ids, lens, score, ctc, lms = _got(name)
    n = int((lens[0] >= 0).sum())
    got = {tuple(ids[0, k, :lens[0, k]].tolist()): (score[0, k], ctc[0, k], lms[0, k]) for k in range(n)}
    assert n == len(want) and set(got) == set(want)
    for l, (R, s, g) in got.items():
        assert abs(R - want[l][0]) <= REL * abs(want[l][0]) and abs(s - want[l][1]) <= REL * abs(want[l][1]) and g == want[l][2], (l, R, s, g, want[l])


def test_the_lm_decides():
    """Two classes within 1e-3 of each other at two steps: alone the acoustic scores read (1, 1), with the bigram table (2, 2)."""
    a0, a1 = _got("decide_a0"), _got("decide_a1")
    assert a0[0][0, 0, :2].tolist() == [1, 1] and a1[0][0, 0, :2].tolist() == [2, 2] and a0[1][0, 0] == a1[1][0, 0] == 2
    assert [h[0] for h in LC.reference("decide_a0")[0][0]][0] == (1, 1) and [h[0] for h in LC.reference("decide_a1")[0][0]][0] == (2, 2)
    assert a1[4][0, 0] == -0.5 and a0[2][0, 0] == a0[3][0, 0]             # g((2, 2)); with alpha = 0 the score is the acoustic one


def _any_table(C, blank):
    return LR.random_table(900 + C + blank, 2, C, blank, per_level=0 if C <= 8 else 300)


_TABLES = {}


@pytest.mark.parametrize("name", [c[0] for c in CC.CASES])
def test_alpha_beta_zero_gives_the_bytes_of_ctc_beam(name):
    _, y, blank, W, nbest = CC.BY_NAME[name]
    key = (y.shape[2], blank)
    if key not in _TABLES:
        _TABLES[key] = _any_table(*key)
    want = TB.run_beam(y, blank, W, nbest)
    ids, lens, score, ctc, lms = run_beam_lm(y, blank, W, nbest, _TABLES[key], 0.0, 0.0)
    assert ids.tobytes() == want[0].tobytes() and lens.tobytes() == want[1].tobytes() and score.tobytes() == want[2].tobytes(), name
    assert ctc.tobytes() == score.tobytes()
    fin = lens >= 0
    assert np.isfinite(lms[fin]).all() and np.isneginf(lms[~fin]).all()
    for b, k in np.argwhere(fin)[:6]:                                    # the LM column is still the string's score
        assert lms[b, k] == _TABLES[key].g(tuple(ids[b, k, :lens[b, k]].tolist()))


def test_rows_are_independent():
    """Five different rows in one launch against each launched alone, and three whose prefix tables are in the workspace; 300 copies of
    two rows (more rows than CUs)."""
    for name in ("rows5", "rows3_T140_C6_W64_workspace"):
        _, y, blank, W, nbest, tname, alpha, beta = LC.BY_NAME[name]
        together = _got(name)
        for b in range(y.shape[1]):
            alone = run_beam_lm(np.ascontiguousarray(y[:, b:b + 1]), blank, W, nbest, LC.table(tname), alpha, beta)
            assert all(np.array_equal(a[0], t[b]) and a[0].tobytes() == t[b].tobytes() for a, t in zip(alone, together)), (name, b)
    _, g, gblank, _, _, gt, ga, gb = LC.BY_NAME["golden_W8"]
    two = run_beam_lm(g, gblank, 8, 4, LC.table(gt), ga, gb)
    many = run_beam_lm(np.ascontiguousarray(np.tile(g, (1, 150, 1))), gblank, 8, 4, LC.table(gt), ga, gb)
    for b in range(300):
        assert all(np.array_equal(m[b], t[b % 2]) for m, t in zip(many, two)), b


def test_two_launches_and_a_graph_replay_give_the_same_bytes():
    L, lib = _L()
    _, y, blank, W, nbest, tname, alpha, beta = LC.BY_NAME["text_like_W64"]
    t = LC.table(tname)
    T, B, C = y.shape
    d = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    first = run_beam_lm(y, blank, W, nbest, t, alpha, beta, d)
    second = run_beam_lm(y, blank, W, nbest, t, alpha, beta, d)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    buf = Buffers(T, B, C, W, nbest)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        L.check(lib.ocrvi_ctc_beam_lm(0, d.data_ptr(), T, B, C, blank, W, nbest, handle(t), alpha, beta, *buf.args(),
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert buf.untouched()                                              # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert buf.guards_ok() and all(a.tobytes() == b.tobytes() for a, b in zip(buf.host(), first))
    buf.ids.fill_(I_GUARD), buf.lens.fill_(I_GUARD), [s.fill_(D_GUARD) for s in buf.scores]
    g.replay()
    torch.cuda.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(buf.host(), first))


def test_argument_checks_leave_the_outputs_untouched():
    L, lib = _L()
    T, B, C, W, nbest = 12, 2, 4, 4, 2
    d = torch.from_numpy(np.ascontiguousarray(LC.BY_NAME["rows5"][1][:, :2])).cuda()
    buf = Buffers(T, B, C, W, nbest)
    ids, lens, score, ctc, lms, ws, nws = buf.args()
    h = handle(LC.table("rand4_o3"))
    foreign = ctypes.create_string_buffer(256)                           # memory that is no handle
    ok = dict(lp=d.data_ptr(), T=T, B=B, C=C, blank=0, W=W, nbest=nbest, lm=h, alpha=1.0, beta=0.5, ids=ids, lens=lens, score=score, ctc=ctc,
              lms=lms, ws=ws, nws=nws)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ocrvi_ctc_beam_lm(0, a["lp"], a["T"], a["B"], a["C"], a["blank"], a["W"], a["nbest"], a["lm"], a["alpha"], a["beta"], a["ids"],
                                     a["lens"], a["score"], a["ctc"], a["lms"], a["ws"], a["nws"], None)

    bad = [dict(nbest=0), dict(nbest=W + 1), dict(W=0, nbest=1), dict(W=65), dict(C=1), dict(C=1025), dict(blank=-1), dict(blank=C), dict(T=0),
           dict(T=1025), dict(B=0), dict(lp=None), dict(ids=None), dict(lens=None), dict(score=None), dict(ctc=None), dict(lms=None), dict(ws=None),
           dict(ws=ws + 8), dict(lm=None), dict(lm=ctypes.cast(foreign, ctypes.c_void_p)), dict(lm=handle(LC.table("rand5_o3"))),   # 5 classes
           dict(lm=handle(LC.table("hand3_o2"))), dict(blank=1), dict(lm=handle(LR.random_table(5, 2, 4, 2))),                    # BOS 2, blank 0
           dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("nan")), dict(beta=float("-inf"))]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # OCRVI_EINVAL
        assert L.last_error(), kw
    assert call(nws=nws - 1) == -3 and call(nws=0) == -3                # OCRVI_ENOMEM
    torch.cuda.synchronize()
    assert buf.untouched()
    assert call(alpha=0.0, beta=-2.0) == 0
    torch.cuda.synchronize()
    assert buf.guards_ok() and not buf.untouched()


# ---------------------------------------------------------------------------------------------------- the facades
@pytest.fixture(scope="module")
def model():
    from ocr_vi_invoice_amd import SVTRv2
    return SVTRv2("tiny", dtype="f16x2")


@pytest.fixture(scope="module")
def charlm():
    from ocr_vi_invoice_amd.lm import CharLM
    m = CharLM.train(LR.synthetic_lines(7, 300), LC.TOK, order=4)
    assert m.blob == LC.table("trained_o4").blob()
    return m


def test_decode_probs_with_beam_and_lm(model, charlm):
    from ocr_vi_invoice_amd.rec import Hypothesis, LMHypothesis
    _, y, blank, W, nbest, _, alpha, beta = LC.BY_NAME["golden_W8"]
    d = torch.from_numpy(y).cuda()
    got = model.decode_probs(d, beam=8, nbest=4, lm=charlm, lm_weight=alpha, len_bonus=beta)
    want = LC.reference("golden_W8")[0]
    assert len(got) == 2 and all(len(r) == 4 and all(isinstance(h, LMHypothesis) for h in r) for r in got)
    for g, w in zip(got, want):
        assert [h.ids for h in g] == [h[0] for h in w[:4]] and [h.text for h in g] == model.tokenizer.decode([h[0] for h in w[:4]])
        assert all(abs(a.score - b[1]) <= REL * abs(b[1]) and abs(a.log_prob - b[2]) <= REL * abs(b[2]) and a.lm_log_prob == b[3] for a, b in zip(g, w))
        assert all(h.lm_log_prob == charlm.score(h.ids) for h in g)
    # without lm: what the parent returns, Hypothesis with the same fields
    plain = model.decode_probs(d, beam=8, nbest=4)
    ids, lens, score = TB.run_beam(y, blank, 8, 4)
    from ocr_vi_invoice_amd.rec import make_hypotheses
    assert plain == make_hypotheses(model.tokenizer, ids, lens, score) and all(type(h) is Hypothesis for r in plain for h in r)
    assert plain == model.decode_probs(d, beam=8, nbest=4, lm=None, lm_weight=1.0, len_bonus=0.0)
    zero = model.decode_probs(d, beam=8, nbest=4, lm=charlm, lm_weight=0.0)
    assert [[(h.text, h.score, h.ids) for h in r] for r in zero] == [[tuple(h) for h in r] for r in plain]
    assert all(h.log_prob == h.score for r in zero for h in r)


def test_lm_value_errors(model, charlm):
    from ocr_vi_invoice_amd import pipeline
    from ocr_vi_invoice_amd.lm import CharLM
    d = torch.zeros((8, 1, 232), device="cuda")
    x = torch.zeros((1, 3, 32, 64), device="cuda")
    small = CharLM.from_ngrams({(1,): (-1.0, 0.0)}, 1, 40)
    other_blank = CharLM.from_ngrams({(2,): (-1.0, 0.0)}, 1, 232, blank_id=1)
    for kw in (dict(lm=charlm), dict(beam=4, lm=small), dict(beam=4, lm=other_blank), dict(beam=4, lm=charlm, lm_weight=-1.0),
               dict(beam=4, lm=charlm, len_bonus=float("nan")), dict(beam=4, lm_weight=0.5), dict(lm=charlm, beam=None, nbest=2)):
        with pytest.raises(ValueError):
            model.decode_probs(d, **kw)
        with pytest.raises(ValueError):
            model.decode_greedy(x, **kw)
        with pytest.raises(ValueError):
            pipeline.recognize_text_batch(model, [np.zeros((8, 8, 3), np.uint8)], **kw)
    with pytest.raises(ValueError):
        model.decode_greedy_and_beam(x, 4, 1, lm=small)


def test_decode_greedy_and_recognize_text_batch_with_lm(model, charlm):
    from ocr_vi_invoice_amd import pipeline, synth
    crops = synth.make_crops(5, 3, height=32, max_width=128)
    x = torch.from_numpy(synth.pad_crop_batch(crops, 32, 128)).cuda()
    kw = dict(lm=charlm, lm_weight=0.7, len_bonus=0.2)
    want = model.decode_probs(model(x), beam=4, nbest=2, **kw)
    assert model.decode_greedy(x, beam=4, nbest=2, **kw) == want and all(1 <= len(r) <= 2 for r in want)
    texts, hyps = model.decode_greedy_and_beam(x, 4, 2, **kw)
    assert texts == model.decode_greedy(x) and hyps == want
    batch = pipeline.recognize_text_batch(model, crops, img_size=(32, 128), batch_size=2, beam=4, nbest=2, **kw)
    alone = [pipeline.recognize_text_batch(model, [c], img_size=(32, 128), beam=4, nbest=2, **kw)[0] for c in crops]
    assert batch == alone and len(batch) == 3 and batch != pipeline.recognize_text_batch(model, crops, img_size=(32, 128), beam=4, nbest=2)


# ---------------------------------------------------------------------------------------------------- the engine
def test_engine_with_lm(charlm):
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, pipeline, weights
    from ocr_vi_invoice_amd.rec import Hypothesis, LMHypothesis
    data = TB._Pages()
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    kw = dict(det_size=TB.DET_SIZE, rec_size=(32, 256), det_chunk=2, rec_batch=8, prob_hook=data.hook)
    lmkw = dict(lm=charlm, lm_weight=0.8, len_bonus=0.3)

    class Blended:                                                       # the page alone sees the map the hook gives the engine
        def __call__(self, x):
            return {"binary": torch.add(data.kern[data.page][None], det(x)["binary"], alpha=0.25)}

    def alone(**more):
        out = []
        for i, p in enumerate(data.pages):
            data.page = i
            out.append(pipeline.detect_and_recognize(p, Blended(), rec, TB._pp(), "cuda:0", det_size=TB.DET_SIZE, rec_size=(32, 256), beam=8,
                                                     nbest=4, **more))
        return out

    with_lm, without = alone(**lmkw), alone()
    plain = Engine(det, rec, TB._pp(), **kw).run(data.pages)
    assert sum(len(r[0]) for r in plain) > 8                            # more crops than one recogniser batch
    eng = Engine(det, rec, TB._pp(), beam=8, nbest=4, **lmkw, **kw)
    for _ in range(2):                                                  # the second run replays the captured graph
        got = eng.run(data.pages)
        for g, w, a in zip(got, plain, with_lm):
            assert len(g) == 4 and all(np.array_equal(x, y) for x, y in zip(g[0], w[0])) and g[1] == w[1] and g[2] == w[2] == a[2]
            assert g[3] == a[3] and all(isinstance(h, LMHypothesis) for hs in g[3] for h in hs) and all(1 <= len(hs) <= 4 for hs in g[3])
    # without lm the engine returns what it returns without the argument: the non-LM path of the same test
    beam_only = Engine(det, rec, TB._pp(), beam=8, nbest=4, **kw).run(data.pages)
    for g, w, a in zip(beam_only, plain, without):
        assert len(g) == 4 and g[2] == w[2] and g[3] == a[3] and all(type(h) is Hypothesis for hs in g[3] for h in hs)
    assert any(g[3] != b[3] for g, b in zip(got, beam_only))
    assert [len(r) for r in plain] == [3] * len(plain)
    for bad in (dict(lm=charlm), dict(beam=4, lm=charlm, lm_weight=-1.0), dict(beam=4, lm_weight=2.0)):
        with pytest.raises(ValueError):
            Engine(det, rec, TB._pp(), **bad, **kw)
    page_kw = dict(det_size=TB.DET_SIZE, rec_size=(32, 256), rec_batch_size=8, beam=8, nbest=4)
    pages = pipeline.detect_and_recognize_pages(data.pages[:1], det, rec, TB._pp(), **page_kw, **lmkw)
    data.page = 0
    one = pipeline.detect_and_recognize(data.pages[0], det, rec, TB._pp(), "cuda:0", det_size=TB.DET_SIZE, rec_size=(32, 256), beam=8, nbest=4, **lmkw)
    assert pages[0][2] == one[2] and pages[0][3] == one[3]
