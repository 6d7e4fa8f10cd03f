"""Document finder, device half (csrc/docfind.hip; include/ocrvi.h, "Document finder"): every stage entry bit for bit against the Python
statement in tests/docfind_ref.py, the batched page-table entry against the stages, and the facades on the three synthetic photos."""
import ctypes

import numpy as np
import pytest
import torch

import docfind_ref as DR

pytestmark = pytest.mark.gpu

POL = {"auto": 0, "bright": 1, "dark": 2}


def _lib():
    from ocr_vi_invoice_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(seed, h, w):
    """A noisy page with a bright slanted block and a dark one, so that every stage has something to get wrong."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    img = 60 + rng.integers(-25, 26, (h, w, 3))
    img[(xs + ys // 3 > w // 4) & (xs < 3 * w // 4) & (ys > h // 5) & (ys < 4 * h // 5)] += 130
    img[(ys > h // 2 - 2) & (ys < h // 2 + 3) & (xs > w // 3)] -= 50
    return np.clip(img, 0, 255).astype(np.uint8)


def gpu_grey(img, work_h):
    L = _lib()
    ww, _ = DR.working_size(img.shape[0], img.shape[1], work_h)
    src, out = _dev(img), torch.full((work_h, ww), 0xAB, dtype=torch.uint8, device="cuda")
    L.check(L.load().ocrvi_doc_grey_u8(0, src.data_ptr(), img.shape[0], img.shape[1], work_h, out.data_ptr(), _stream()))
    return out.cpu().numpy()


def gpu_smooth(g):
    L = _lib()
    src, out = _dev(g), torch.full(g.shape, 0xAB, dtype=torch.uint8, device="cuda")
    L.check(L.load().ocrvi_doc_smooth_u8(0, src.data_ptr(), g.shape[0], g.shape[1], out.data_ptr(), _stream()))
    return out.cpu().numpy()


def gpu_hist(s):
    L = _lib()
    src, out = _dev(s), torch.full((256,), -5, dtype=torch.int32, device="cuda")
    L.check(L.load().ocrvi_doc_histogram(0, src.data_ptr(), s.shape[0], s.shape[1], out.data_ptr(), _stream()))
    return out.cpu().numpy()


def gpu_otsu(s, hist, polarity="auto"):
    L = _lib()
    ds, dh, out = _dev(s), _dev(hist.astype(np.int32)), torch.full((4,), -5, dtype=torch.int32, device="cuda")
    L.check(L.load().ocrvi_doc_otsu(0, ds.data_ptr(), dh.data_ptr(), s.shape[0], s.shape[1], POL[polarity], out.data_ptr(), _stream()))
    t, inv, z0, z1 = out.cpu().tolist()
    assert z0 == 0 and z1 == 0
    return t, bool(inv)


def gpu_bits(s, t, inv):
    L = _lib()
    wpr = (s.shape[1] + 31) // 32
    ds, thr = _dev(s), _dev(np.array([t, int(inv), 0, 0], np.int32))
    out = torch.full((s.shape[0], wpr), -1, dtype=torch.int32, device="cuda")          # every bit set: padding must be cleared by the kernel
    L.check(L.load().ocrvi_doc_mask_bits(0, ds.data_ptr(), s.shape[0], s.shape[1], thr.data_ptr(), out.data_ptr(), _stream()))
    return out.cpu().numpy().view(np.uint32)


def gpu_pages(images, work_h, polarity="auto", ww_cap=None):
    """ocrvi_doc_mask_pages on `images` (None: an invalid entry) -> the uint32 slots [n, mask_words]."""
    L = _lib()
    lib = L.load()
    devs = [None if im is None else _dev(im) for im in images]
    if ww_cap is None:
        ww_cap = max(DR.working_size(im.shape[0], im.shape[1], work_h)[0] for im in images if im is not None)
    ws, words = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L.check(lib.ocrvi_doc_mask_sizes(len(images), work_h, ww_cap, ctypes.byref(ws), ctypes.byref(words)))
    assert words.value == work_h * ((ww_cap + 31) // 32)
    table = _dev(np.array([(0, 7, 7, 0) if d is None else (d.data_ptr(), d.shape[0], d.shape[1], 0) for d in devs], np.int64))
    work = torch.full((ws.value,), 0xCD, dtype=torch.uint8, device="cuda")
    masks = torch.full((len(images), words.value), -1, dtype=torch.int32, device="cuda")
    L.check(lib.ocrvi_doc_mask_pages(0, table.data_ptr(), len(images), work_h, ww_cap, POL[polarity], masks.data_ptr(), work.data_ptr(), ws.value,
                                     _stream()))
    return masks.cpu().numpy().view(np.uint32)


def check_stages(img, work_h, polarity="auto"):
    """Every stage entry on the reference's input of that stage, then the batched entry against the stages."""
    ref = DR.stages(img, work_h, polarity)
    assert np.array_equal(gpu_grey(img, work_h), ref["grey"])
    assert np.array_equal(gpu_smooth(ref["grey"]), ref["smooth"])
    assert np.array_equal(gpu_hist(ref["smooth"]), ref["hist"])
    assert gpu_otsu(ref["smooth"], ref["hist"], polarity) == (ref["t"], ref["inverted"])
    assert np.array_equal(gpu_bits(ref["smooth"], ref["t"], ref["inverted"]), ref["bits"])
    slot = gpu_pages([img], work_h, polarity)[0]
    assert np.array_equal(slot.reshape(ref["bits"].shape), ref["bits"])
    return ref


def test_boxes_of_exactly_eight_rows_and_ragged_columns():
    L = _lib()
    img = _image(1, 296, 41)                      # 296 / 37 = 8 rows a box; 41 / 8 -> ww = 5: refused
    with pytest.raises(ValueError):
        DR.working_size(296, 41, 37)
    src, out = _dev(img), torch.zeros(37 * 8, dtype=torch.uint8, device="cuda")
    assert L.load().ocrvi_doc_grey_u8(0, src.data_ptr(), 296, 41, 37, out.data_ptr(), _stream()) == -1
    assert not gpu_pages([img, _image(2, 296, 75)], 37, ww_cap=16)[0].any()          # in a table: the page is left all zero
    ref = check_stages(_image(2, 296, 75), 37)    # the narrowest page of that height that is taken: ww = 9, columns of 8 and 9 pixels
    assert ref["grey"].shape == (37, 9) and ref["mask"].any()


def test_ragged_boxes_both_ways():
    ref = check_stages(_image(3, 300, 333), 37)
    assert ref["grey"].shape == (37, 41) and ref["mask"].any() and not ref["mask"].all()


def test_upscale_every_box_one_pixel():
    img = _image(4, 40, 70)
    ref = check_stages(img, 64)
    assert ref["grey"].shape == (64, 112)
    p = img.astype(np.int64)
    luma = (77 * p[:, :, 0] + 150 * p[:, :, 1] + 29 * p[:, :, 2] + 128) >> 8
    assert np.array_equal(ref["grey"], luma[(np.arange(64) * 40) // 64][:, (np.arange(112) * 70) // 112])


def test_two_pages_of_mixed_sizes_at_500_rows_in_one_launch():
    imgs = [_image(5, 1000, 760), _image(6, 1237, 911)]
    refs = [DR.stages(im, 500) for im in imgs]
    assert [r["grey"].shape for r in refs] == [(500, 380), (500, 368)]
    slots = gpu_pages(imgs, 500)
    for im, r, slot in zip(imgs, refs, slots):
        n = r["bits"].size
        assert np.array_equal(gpu_grey(im, 500), r["grey"])
        assert np.array_equal(slot[:n].reshape(r["bits"].shape), r["bits"]) and not slot[n:].any() and r["mask"].any()


def test_an_invalid_table_entry_in_the_middle():
    imgs = [_image(7, 120, 200), None, _image(8, 90, 77)]
    slots = gpu_pages(imgs, 40)
    assert not slots[1].any()
    for im, slot in zip(imgs, slots):
        if im is not None:
            bits = DR.stages(im, 40)["bits"]
            assert bits.any() and np.array_equal(slot[:bits.size].reshape(bits.shape), bits) and not slot[bits.size:].any()


def test_a_constant_page_has_no_threshold():
    img = np.full((100, 130, 3), 93, np.uint8)
    ref = check_stages(img, 50)
    assert ref["t"] == -1 and not ref["bits"].any()
    for pol in ("bright", "dark"):
        assert gpu_otsu(ref["smooth"], ref["hist"], pol) == (-1, False) and not gpu_pages([img], 50, pol).any()


def test_the_polarity_tie_keeps_the_mask():
    s = np.full((20, 30), 50, np.uint8)
    s[5:15, 5:25] = 200
    ring = np.ones(s.shape, bool)
    ring[1:-1, 1:-1] = False
    ys, xs = np.nonzero(ring)
    assert len(ys) == 96
    s[ys[:48], xs[:48]] = 200                        # exactly half of the ring is set
    hist = DR.histogram(s)
    assert DR.otsu(hist) == 50 and not DR.inverted(s, 50)
    assert gpu_otsu(s, hist) == (50, False)
    s[ys[48], xs[48]] = 200                          # one more: the frame is background
    hist = DR.histogram(s)
    assert DR.inverted(s, 50) and gpu_otsu(s, hist) == (50, True)


@pytest.mark.parametrize("polarity", ["bright", "dark"])
def test_a_forced_polarity_overrides_the_ring(polarity):
    img = _image(9, 150, 170)
    ref = check_stages(img, 60, polarity)
    assert ref["inverted"] == (polarity == "dark") and ref["mask"].any()
    other = DR.stages(img, 60, "dark" if polarity == "bright" else "bright")
    assert not np.array_equal(ref["bits"], other["bits"])


def test_the_widest_working_image_puts_d_at_its_bound():
    rng = np.random.default_rng(10)
    img = np.zeros((64, 8192, 3), np.uint8)
    img[:, 4096:] = 255                              # half the pixels in bin 0, half in bin 255: |d| is as large as 64 rows allow
    img[20:40, 1000:1200] = 255
    img[rng.integers(0, 64, 300), rng.integers(0, 8192, 300)] = 128
    ref = check_stages(img, 64)
    assert ref["grey"].shape == (64, 8192) and 0 <= ref["t"] < 255
    with pytest.raises(ValueError):
        DR.working_size(64, 8193, 64)


def test_a_one_pixel_line_is_erased_and_a_blob_on_all_four_edges_survives():
    s = np.zeros((40, 70), np.uint8)
    s[:, 33] = 255
    s[11, :] = 255
    assert not gpu_bits(s, 100, False).any() and not DR.opening(s > 100).any()
    ys, xs = np.mgrid[0:40, 0:70]
    blob = (((xs - 35) / 38.0) ** 2 + ((ys - 20) / 23.0) ** 2) <= 1          # an ellipse cut by all four edges
    assert blob[0].any() and blob[-1].any() and blob[:, 0].any() and blob[:, -1].any() and not blob.all()
    s = np.where(blob, 255, 0).astype(np.uint8)
    want = DR.opening(s > 100)
    assert want[0].any() and want[:, 0].any()        # the frame is background for the erosion, and the dilation brings the edge back
    assert np.array_equal(gpu_bits(s, 100, False), DR.pack_bits(want))
    assert np.array_equal(gpu_bits(s, 100, True), DR.pack_bits(DR.opening(~(s > 100))))


def test_mask_padding_bits_are_zero():
    s = np.full((16, 41), 255, np.uint8)
    bits = gpu_bits(s, 100, False)
    assert bits.shape == (16, 2) and (bits[:, 0] == 0xFFFFFFFF).all() and (bits[:, 1] == (1 << 9) - 1).all()


# ---------------------------------------------------------------------------------------------------- facades
_CACHE = {}


def _photos():
    if not _CACHE:
        for name in DR.PHOTOS:
            img, _ = DR.photo(name)
            _CACHE[name] = (img, DR.find_quad(img))
    return [_CACHE[n][0] for n in DR.PHOTOS], [_CACHE[n][1] for n in DR.PHOTOS]


def _equal(got, want):
    return len(got) == len(want) and all(g is not None and g.dtype == np.float64 and g.shape == (4, 2) and np.array_equal(g, w)
                                         for g, w in zip(got, want))


def test_find_document_quads_on_arrays_tensors_and_png_bytes():
    from ocr_vi_invoice_amd import pipeline
    imgs, want = _photos()
    assert all(w is not None for w in want)
    assert _equal(pipeline.find_document_quads(imgs), want)
    assert _equal(pipeline.find_document_quads([_dev(im) for im in imgs]), want)
    files = pipeline.imencode_png_pages([_dev(im) for im in imgs])
    assert _equal(pipeline.find_document_quads(files), want)
    mixed = pipeline.find_document_quads([imgs[0], np.full((64, 48, 3), 9, np.uint8), files[2], np.zeros((2000, 10, 3), np.uint8)])
    assert mixed[1] is None and mixed[3] is None and _equal([mixed[0], mixed[2]], [want[0], want[2]])
    assert np.array_equal(pipeline.find_document_quad(imgs[1]), want[1]) and pipeline.find_document_quads([]) == []


def test_the_facades_compose():
    import ocr_vi_invoice_amd as pkg
    from ocr_vi_invoice_amd import pipeline
    imgs, want = _photos()
    for im, w in zip(imgs[:2], want[:2]):
        ref = DR.stages(im)
        mask, ratio = pkg.document_mask(im)
        assert isinstance(mask, np.ndarray) and mask.dtype == np.uint8 and np.array_equal(mask, ref["mask"].astype(np.uint8) * 255)
        dmask, dratio = pkg.document_mask(_dev(im))
        assert dmask.is_cuda and dratio == ratio and np.array_equal(dmask.cpu().numpy(), mask)
        quad, kind = pkg.find_document_contour(mask, return_kind=True)
        assert kind == "polygon" and np.array_equal(quad.astype(np.float64) * ratio, w)
        assert np.array_equal(pkg.find_document_contour(dmask).astype(np.float64) * dratio, w)
    page = pipeline.preprocess_image(imgs[0], pkg.find_document_quad(imgs[0]))
    assert np.array_equal(page, pipeline.four_point_transform(imgs[0], want[0])) and page.shape != imgs[0].shape
    assert pipeline.preprocess_image(imgs[0], pkg.find_document_quad(np.full((64, 48, 3), 9, np.uint8))) is imgs[0]
    with pytest.raises(ValueError):
        pkg.document_mask(imgs[0], polarity="inverse")
    with pytest.raises(ValueError):
        pkg.document_mask(np.zeros((2000, 10, 3), np.uint8))
