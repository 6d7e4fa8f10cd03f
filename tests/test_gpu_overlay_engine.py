"""Engine(..., annotate=True).run(pages, quads, enhance): the fourth element of each page's result equals pipeline.draw_boxes_with_text on the
page pipeline.detect_and_recognize would have processed (rectified, enhanced), with that call's boxes and texts; the first three
elements equal those of the same run without annotate.  One page with a quad, one enhanced page, two plain ones, in two waves.  Then
pipeline.save_result: draw + imwrite."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

DET_SIZE = 320
SIZES = [(1000, 760), (900, 700), (760, 1000), (800, 600)]
SEEDS = [11, 12, 13, 14]
QUADS = [[(31.5, 22.25), (735.0, 40.5), (722.75, 978.0), (18.0, 960.5)], None, None, None]
ENHANCE = [False, True, False, False]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


class _Set:
    """The pages, and per page the rendered text kernels at the detector shape of the rectified page (as tests/test_gpu_enhance.py):
    random weights give a map without text structure."""

    def __init__(self):
        from ocr_vi_invoice_amd import pipeline, synth
        from ocr_vi_invoice_amd.engine import plan_rectified
        self.pages, self.kern = [], []
        _, _, shapes, scales, _ = plan_rectified(SIZES, QUADS, DET_SIZE)
        for (h, w), seed, quad, (H, W), (sh, sw) in zip(SIZES, SEEDS, QUADS, shapes, scales):
            img, boxes = synth.make_invoice(seed, h, w, lines=8)
            self.pages.append(img)
            fwd = np.eye(3) if quad is None else pipeline.four_point_geometry(quad)[0]
            k = np.zeros((1, H, W), np.float32)
            for x, y, bw, bh in boxes:
                c = WR.project(fwd, [(x, y), (x + bw, y), (x + bw, y + bh), (x, y + bh)])
                x0, x1 = int(c[:, 0].min() * sw) + 2, int(c[:, 0].max() * sw) - 2
                y0, y1 = int(c[:, 1].min() * sh) + 1, int(c[:, 1].max() * sh) - 1
                if x1 - x0 >= 3 and y1 - y0 >= 2 and x0 >= 0 and y0 >= 0:
                    k[0, y0:y1, x0:x1] = 0.75
            self.kern.append(torch.from_numpy(k).cuda())

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
def runs():
    """(pages, per-page reference results, the engine's results with annotate, without) -- computed once."""
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, pipeline, weights
    data = _Set()
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    wrap = _BlendedDet(det, data)
    want = []
    for i, (p, q, e) in enumerate(zip(data.pages, QUADS, ENHANCE)):
        wrap.page = i
        want.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64, quad=q,
                                                  enhance=e))
    pages = list(data.pages)
    pages[2] = torch.from_numpy(pages[2]).cuda()                  # a caller's device tensor: never written
    keep = pages[2].clone()
    eng = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=2, rec_batch=16, max_pages=3, prob_hook=data.hook,
                 annotate=True)
    with_a = eng.run(pages, QUADS, ENHANCE)
    eng.annotate = False                                          # the same engine, the switch off: the result it always gave
    without = eng.run(pages, QUADS, ENHANCE)
    assert torch.equal(pages[2], keep)
    return data.pages, want, with_a, without


def _same_three(got, want):
    assert len(got[0]) == len(want[0]) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[0], want[0]))
    assert got[1] == want[1] and got[2] == want[2]


def test_annotated_page_equals_draw_on_the_processed_page(runs):
    from ocr_vi_invoice_amd import pipeline
    pages, want, with_a, _ = runs
    assert all(len(r) == 4 for r in with_a) and all(len(w[0]) > 0 for w in want)
    for i, (p, q, e) in enumerate(zip(pages, QUADS, ENHANCE)):
        seen = pipeline.preprocess_image(p, q)                    # what detect_and_recognize processed
        if e:
            seen = pipeline.enhance_document(seen)
        if q is None and not e:
            assert np.array_equal(seen.cpu().numpy() if isinstance(seen, torch.Tensor) else seen, p)
        boxes, _, texts = want[i]
        painted = pipeline.draw_boxes_with_text(seen, boxes, texts)
        got = with_a[i][3]
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == painted.shape, i
        assert torch.equal(got, painted), i
        assert not torch.equal(painted.cpu(), torch.as_tensor(seen).cpu()), i      # the boxes are there


def test_first_three_elements_do_not_depend_on_annotate(runs):
    _, want, with_a, without = runs
    assert all(len(r) == 3 for r in without)
    for a, b, w in zip(with_a, without, want):
        _same_three(a[:3], b)
        _same_three(b, w)


def test_annotated_pages_are_separate_tensors(runs):
    _, _, with_a, _ = runs
    ptrs = [r[3].data_ptr() for r in with_a]
    assert len(set(ptrs)) == len(ptrs) and all(r[3].is_contiguous() for r in with_a)


def test_save_result_writes_a_file_imread_reads(runs, tmp_path):
    from ocr_vi_invoice_amd import pipeline
    pages, want, _, _ = runs
    path = str(tmp_path / "result.jpg")
    boxes, _, texts = want[3]
    assert pipeline.save_result(path, pages[3], boxes, texts) is True
    back = pipeline.imread(path)
    assert tuple(back.shape) == pages[3].shape
    # the file is the painted page's file
    assert open(path, "rb").read() == pipeline.imencode(pipeline.draw_boxes_with_text(pages[3], boxes, texts), 95)
    assert pipeline.save_result(str(tmp_path / "no" / "such" / "dir.jpg"), pages[3], boxes, texts) is False
