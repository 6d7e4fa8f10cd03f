"""Engine.run(pages, quads="deskew") (ocr_vi_invoice_amd/engine.py): the skews estimated by pipeline.estimate_skews, the tilted pages given
pipeline.skew_quad, then the existing path.  Four pages of mixed sizes: two rotated synthetic invoices (a host array and PNG bytes), a
straight one (a device tensor) and a constant page.  Random weights give a map without text structure, so bars are blended into it as
tests/test_gpu_docfind_engine.py does."""
import numpy as np
import pytest
import torch

import skew_ref as SR

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


def test_run_with_deskew_equals_run_with_the_skew_quads():
    from ocr_vi_invoice_amd import pipeline, synth
    tilted_a = SR.rotated(synth.make_invoice(5, 400, 520, 14)[0], 4, enclose=True)
    tilted_b = SR.rotated(synth.make_invoice(6, 520, 380, 18)[0], -6, enclose=False)
    straight, flat = synth.make_invoice(7, 360, 480, 12)[0], np.full((300, 260, 3), 200, np.uint8)
    pages = [tilted_a, torch.from_numpy(straight).cuda(), pipeline.imencode_png(torch.from_numpy(tilted_b).cuda()), flat]
    skews = pipeline.estimate_skews(pages)
    assert [s.k for s in skews] == [SR.estimate(tilted_a).k, 0, SR.estimate(tilted_b).k, 0] and skews[0].k > 0 > skews[2].k
    quads = [pipeline.skew_quad(p.shape[0], p.shape[1], s.k) if s.k else None for p, s in zip([tilted_a, straight, tilted_b, flat], skews)]
    eng = _engine()
    want = eng.run(pages, quads)
    assert eng.stats["rectified"] == 2 and eng.stats["deskewed"] == 0 and all(len(w[0]) >= 3 for w in want)
    got = eng.run(pages, quads="deskew")
    assert eng.stats["rectified"] == 2 and eng.stats["deskewed"] == 2 and eng.stats["pages"] == 4
    _same(got, want)
    _same([got[1], got[3]], eng.run([straight, flat]))                  # the straight and the constant page come through as they are
    assert eng.stats["deskewed"] == 0
    eng.deskew_min_gain = 1e9                                            # a caller's knob: nothing is sure enough, nothing is turned
    kept = eng.run(pages, quads="deskew")
    assert eng.stats["deskewed"] == 0 and eng.stats["rectified"] == 0
    _same(kept, eng.run(pages))
    assert eng.run([], quads="deskew") == []
    with pytest.raises(ValueError, match="quads"):
        eng.run(pages, quads="find")
