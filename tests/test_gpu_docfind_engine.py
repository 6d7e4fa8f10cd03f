"""Engine.run(pages, quads="auto") (ocr_vi_invoice_amd/engine.py): the corners found by pipeline.find_document_quads, then the existing
path.  Four pages of mixed sizes, two with a document to find (a host array and PNG bytes) and two constant ones (a device tensor and a
host array).  Random weights give a map without text structure, so bars are blended into it as tests/test_gpu_engine.py does."""
import numpy as np
import pytest
import torch

import docfind_ref as DR

pytestmark = pytest.mark.gpu

DET_SIZE = 320
_BARS = {}


def _hook(prob, idx):
    H, W = prob.shape[2], prob.shape[3]
    if (H, W) not in _BARS:
        k = np.zeros((1, H, W), np.float32)
        for j in range((H - 30) // 40):
            k[0, 20 + 40 * j:32 + 40 * j, W // 8 + 3 * j:W - W // 8] = 0.75
        _BARS[(H, W)] = torch.from_numpy(k).cuda()
    torch.add(_BARS[(H, W)].expand(prob.shape[0], 1, H, W), prob, alpha=0.25, out=prob)


def _engine():
    from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, weights
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2")
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2")
    pp = DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)
    return Engine(det, rec, pp, det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=_hook)


def _same(a, b):
    assert len(a) == len(b)
    for (ba, sa, ta), (bb, sb, tb) in zip(a, b):
        assert len(ba) == len(bb) and all(np.array_equal(x, y) for x, y in zip(ba, bb))
        assert np.array_equal(np.asarray(sa), np.asarray(sb)) and list(ta) == list(tb)


def test_run_with_auto_quads_equals_run_with_the_found_quads():
    from ocr_vi_invoice_amd import pipeline
    bright, dark = DR.photo("bright_on_dark")[0], DR.photo("dark_on_bright")[0]
    flat_a, flat_b = np.full((300, 260, 3), 200, np.uint8), np.full((420, 320, 3), 31, np.uint8)
    pages = [bright, torch.from_numpy(flat_a).cuda(), pipeline.imencode_png(torch.from_numpy(dark).cuda()), flat_b]
    quads = pipeline.find_document_quads(pages)
    assert quads[1] is None and quads[3] is None
    assert np.array_equal(quads[0], DR.find_quad(bright)) and np.array_equal(quads[2], DR.find_quad(dark))
    eng = _engine()
    want = eng.run(pages, quads)
    assert eng.stats["rectified"] == 2 and all(len(w[0]) >= 3 for w in want)
    got = eng.run(pages, quads="auto")
    assert eng.stats["rectified"] == 2 and eng.stats["pages"] == 4
    _same(got, want)
    _same([got[1], got[3]], [r for r in eng.run([flat_a, flat_b])])      # the constant pages come through unrectified
    assert eng.run([], quads="auto") == []
    with pytest.raises(ValueError, match="quads"):
        eng.run(pages, quads="find")
