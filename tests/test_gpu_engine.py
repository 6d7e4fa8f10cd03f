"""Engine.run (ocr_vi_invoice_amd/engine.py) against the per-page product call it batches, pipeline.detect_and_recognize: the same boxes,
scores and strings for every page of a mixed-size set, in the modes where a page inside a chunk computes what it computes alone (f32,
f16x2), and the same results whatever the engine's batching knobs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DET_SIZE = 320
# (h, w): two originals of different scale in one 320x256 bucket, a wide page, a square one, a thin wide strip, and a duplicate
SIZES = [(1000, 760), (900, 700), (760, 1000), (640, 640), (333, 1001), (1000, 760)]
SEEDS = [11, 12, 13, 14, 15, 11]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


def _scaled_block_sd(sd, s):
    """SVTRv2 state_dict with stage 0 / block 0's MLP input driven to rms ~ s (as tests/test_gpu_f16x2_range.py does)."""
    out = {k: v.clone() for k, v in sd.items()}
    out["stages.0.blocks.0.norm2.weight"] *= s
    out["stages.0.blocks.0.norm2.bias"] *= s
    out["stages.0.blocks.0.mlp.fc1.weight"] /= s
    return out


class _Set:
    """The pages, and per page the rendered text kernels at its detector shape (random weights give a map without text structure:
    bench.py's blend, kernel + 0.25 binary)."""

    def __init__(self):
        from ocr_vi_invoice_amd import synth
        from ocr_vi_invoice_amd.engine import plan_buckets
        self.pages, kern = [], []
        shapes, scales, _ = plan_buckets(SIZES, DET_SIZE)
        for (h, w), seed, (H, W), (sh, sw) in zip(SIZES, SEEDS, shapes, scales):
            img, boxes = synth.make_invoice(seed, h, w, lines=8)
            self.pages.append(img)
            k = np.zeros((1, H, W), np.float32)
            for x, y, bw, bh in boxes:
                x0, x1 = int(x * sw) + 2, int((x + bw) * sw) - 2
                y0, y1 = int(y * sh) + 1, int((y + bh) * sh) - 1
                if x1 - x0 >= 3 and y1 - y0 >= 2:
                    k[0, y0:y1, x0:x1] = 0.75
            kern.append(torch.from_numpy(k).cuda())
        self.kern = kern

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


class _BlendedDet:
    """detect_and_recognize's detector for page `page`: the library detector, its binary map blended exactly as the engine's hook does."""

    def __init__(self, det, data):
        self.det, self.data, self.page = det, data, 0

    def __call__(self, x):
        out = self.det(x)
        return {"binary": torch.add(self.data.kern[self.page][None], out["binary"], alpha=0.25)}


@pytest.fixture(scope="module")
def data():
    return _Set()


def _models(dtype):
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, weights
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype=dtype)
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype=dtype)
    return det, rec


def _per_page(data, det, rec):
    from ocr_vi_invoice_amd import pipeline
    wrap = _BlendedDet(det, data)
    want = []
    for i, p in enumerate(data.pages):
        wrap.page = i
        want.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64))
    return want


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        for a, b in zip(gb, wb):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
        assert gs == ws, i
        assert gt == wt, i


_CACHE = {}


def _reference(data, dtype):
    if dtype not in _CACHE:
        det, rec = _models(dtype)
        _CACHE[dtype] = (det, rec, _per_page(data, det, rec))
    return _CACHE[dtype]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_engine_equals_detect_and_recognize_per_page(data, dtype):
    from ocr_vi_invoice_amd import Engine
    det, rec, want = _reference(data, dtype)
    assert sum(len(w[0]) for w in want) > 20 and all(len(w[0]) > 0 for w in want)
    eng = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    got = eng.run(data.pages)
    _assert_same(got, want)
    assert eng.stats["buckets"] == {"320x256": 3, "256x320": 1, "320x320": 1, "96x320": 1}
    _assert_same(got[5:], got[:1])                                  # the duplicate page
    # device tensors in, the same results out; a second call reuses the captured graphs
    _assert_same(eng.run([torch.from_numpy(p).cuda() for p in data.pages]), want)


@pytest.mark.parametrize("knob", [dict(graphs=False), dict(det_chunk=1), dict(rec_batch=8), dict(rec_batch=256), dict(max_pages=2),
                                  dict(graph_cache=1, det_chunk=2), dict(post_threads=1)])
def test_engine_results_do_not_depend_on_its_batching(data, knob):
    from ocr_vi_invoice_amd import Engine
    det, rec, want = _reference(data, "f16x2")
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    kw.update(knob)
    _assert_same(Engine(det, rec, _pp(), **kw).run(data.pages), want)


def test_engine_edge_cases(data):
    from ocr_vi_invoice_amd import Engine, pipeline
    det, rec, want = _reference(data, "f16x2")
    eng = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16)
    assert eng.run([]) == []
    blank = np.full((500, 400, 3), 255, np.uint8)
    # a page without text: no kernel in its blend (0.25 binary stays under the 0.3 threshold) -> three empty lists, as the per-page call
    eng_blank = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), prob_hook=lambda prob, idx: prob.mul_(0.25))
    assert eng_blank.run([blank, blank]) == [([], [], []), ([], [], [])]
    assert pipeline.detect_and_recognize(blank, lambda x: {"binary": det(x)["binary"] * 0.25}, rec, _pp(), det_size=DET_SIZE) == ([], [], [])
    for bad in (np.zeros((0, 100, 3), np.uint8), np.zeros((2000, 90, 3), np.uint8), data.pages[0].astype(np.float32),
                data.pages[0][:, :, 0], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            eng.run([data.pages[1], bad])
    # the one-shot wrapper, on the plain random-weight detector
    pp = _pp()
    pp.max_candidates = 50
    got = pipeline.detect_and_recognize_pages(data.pages[2:5], det, rec, pp, "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64)
    _assert_same(got, [pipeline.detect_and_recognize(p, det, rec, pp, "cuda:0", det_size=DET_SIZE) for p in data.pages[2:5]])


def test_engine_overflow_raises_and_the_next_run_is_clean(data):
    from ocr_vi_invoice_amd import Engine, SVTRv2, _lib, weights
    import ctypes
    det, rec, want = _reference(data, "f16x2")
    sd = weights.make_rec_state_dict("tiny", seed=22)
    bad = SVTRv2("tiny", state_dict=_scaled_block_sd(sd, 2.0 ** 17), dtype="f16x2")       # LayerNorm output ~ 2^17 > 65504
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    with pytest.raises(OverflowError):
        Engine(det, bad, _pp(), **kw).run(data.pages)
    flag = ctypes.c_int(1)
    _lib.check(_lib.load().ocrvi_range_flag(0, ctypes.byref(flag)))
    assert flag.value == 0                                                                 # reset before raising
    _assert_same(Engine(det, rec, _pp(), **kw).run(data.pages), want)
