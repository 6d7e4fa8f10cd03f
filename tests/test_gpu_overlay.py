"""ocrvi_overlay_pages through pipeline.draw_boxes_with_text / draw_boxes_pages against tests/overlay_ref.py: every painted page equals
the brute-force reference byte for byte.  The cases (tests/overlay_cases.py) are laid out against the kernel's 64 x 16 tiles, its rounds
of 256 primitives and its passes of 256 staged segments; tests/test_overlay_cpu.py shows that each wrong variant of the reference
changes at least one of them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as cases  # noqa: E402
import overlay_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    bad = np.argwhere((got != want).any(-1))
    return None if not len(bad) else (len(bad), [(int(y), int(x), got[y, x].tolist(), want[y, x].tolist()) for y, x in bad[:4]])


@pytest.mark.parametrize("name", sorted(cases.BOX_CASES))
def test_pages_equal_the_reference(name):
    from ocr_vi_invoice_amd import pipeline
    pages, boxes, texts, pairs, T = cases.box_case(name)
    saved = [p.copy() for p in pages]
    got = pipeline.draw_boxes_pages(pages, boxes, texts, thickness=T)
    assert len(got) == len(pages)
    for k, (g, p, b, n) in enumerate(zip(got, pages, boxes, pairs)):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == p.shape
        want = R.draw(p, b, n, thickness=T)
        assert _first_difference(g.cpu().numpy(), want) is None, (name, k)
        assert np.array_equal(p, saved[k])
        if b:
            assert (want != p).any()                                   # the case paints something on this page
    if name == "five_pages":
        assert np.array_equal(got[3].cpu().numpy(), pages[3])          # the page without boxes comes back as it went in
    if name == "inside":                                               # tiles the box's bounding box hits and none of its segments does
        assert np.array_equal(got[0].cpu().numpy()[32:176, 64:256], pages[0][32:176, 64:256])


def test_one_page_equals_its_place_in_the_batch():
    from ocr_vi_invoice_amd import pipeline
    pages, boxes, texts, pairs, T = cases.box_case("five_pages")
    batch = pipeline.draw_boxes_pages(pages, boxes, texts)
    for k in range(len(pages)):
        one = pipeline.draw_boxes_with_text(pages[k], boxes[k], None if texts[k] is None else texts[k])
        assert torch.equal(one, batch[k]), k


@pytest.mark.parametrize("name", sorted(cases.RAW_CASES))
def test_raw_segments_equal_the_reference(name):
    """Segment tables no box produces: the corners of the legal coordinate range on a 64 x 16384 page (the largest products of the rule),
    and segments of different thickness in one launch."""
    from ocr_vi_invoice_amd import pipeline
    page, segs, prims = cases.raw_case(name)
    dev = torch.from_numpy(page).cuda()
    pipeline.overlay_paint_([dev], segs.astype(np.int32), prims.astype(np.int32), np.asarray([0, len(prims)], np.int32))
    want = R.paint(page, segs)
    assert (want != page).any()
    assert _first_difference(dev.cpu().numpy(), want) is None


def test_facade_returns_a_new_tensor_and_keeps_its_input():
    from ocr_vi_invoice_amd import pipeline
    pages, boxes, _, pairs, T = cases.box_case("overlapping_labels")
    want = R.draw(pages[0], boxes[0], pairs[0])
    host = torch.from_numpy(pages[0].copy())
    dev = host.cuda()
    wide = torch.zeros((100, 120, 3), dtype=torch.uint8, device="cuda")
    wide[:, :90] = dev
    for src in (pages[0], host, dev, wide[:, :90]):                    # numpy, host tensor, device tensor, a view that is not contiguous
        out = pipeline.draw_boxes_with_text(src, boxes[0], ["a", "b", "c", "d"])
        assert out.is_cuda and out.is_contiguous() and np.array_equal(out.cpu().numpy(), want)
        if isinstance(src, torch.Tensor):
            assert out.data_ptr() != src.data_ptr()
            assert np.array_equal(src.cpu().numpy(), pages[0])
    assert np.array_equal(wide.cpu().numpy()[:, 90:], np.zeros((100, 30, 3), np.uint8))
    # zip: two texts, two pairs; other colours
    cut = pipeline.draw_boxes_with_text(dev, boxes[0], ["a", "b"], color=(1, 2, 3), label_color=(4, 5, 6), thickness=3)
    assert np.array_equal(cut.cpu().numpy(), R.draw(pages[0], boxes[0], 2, color=(1, 2, 3), label_color=(4, 5, 6), thickness=3))
    # nothing to draw: a copy
    none = pipeline.draw_boxes_with_text(dev, [])
    assert none.data_ptr() != dev.data_ptr() and torch.equal(none, dev)
    assert pipeline.draw_boxes_pages([], []) == []
