"""The engine's page-table kernels (include/ocrvi.h, OCRVI_PAGE_ENTRY) against the single-page kernels they batch: bit for bit, on pages
of different sizes, and through a captured graph whose page table is rewritten after the pages moved."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


def _pages(sizes, seed=0):
    from ocr_vi_invoice_amd import synth
    return [synth.make_invoice(seed + i, h, w, lines=max(2, h // 40))[0] for i, (h, w) in enumerate(sizes)]


def _table(dev_pages):
    t = np.zeros((len(dev_pages), 4), np.int64)
    for i, p in enumerate(dev_pages):
        t[i] = (p.data_ptr(), p.shape[0], p.shape[1], 0)
    return torch.from_numpy(t).cuda()


# (source sizes, bucket H x W): identity, exact 2x (area path), up-scale, tall and wide originals squeezed into one shape
CASES = [([(320, 256), (640, 512), (100, 96), (1001, 333), (300, 700)], (320, 256)),
         ([(960, 1280), (480, 640), (1920, 2560), (961, 1279)], (960, 1280))]


@pytest.mark.parametrize("sizes,shape", CASES)
def test_resize_normalize_pages_equals_resize_then_normalize(sizes, shape):
    from oracle import preproc_cpu as P
    L, lib = _L()
    H, W = shape
    pages = [torch.from_numpy(p).cuda() for p in _pages(sizes)]
    tab = _table(pages)
    out = torch.empty((len(pages), 3, H, W), device="cuda")
    L.check(lib.ocrvi_resize_normalize_pages(0, tab.data_ptr(), len(pages), H, W, out.data_ptr(), None))
    got = out.cpu().numpy()
    for i, p in enumerate(pages):
        r = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        L.check(lib.ocrvi_resize_u8(0, p.data_ptr(), p.shape[0], p.shape[1], r.data_ptr(), H, W, None))
        want = torch.empty((1, 3, H, W), device="cuda")
        L.check(lib.ocrvi_normalize_u8(0, r.data_ptr(), 1, H, W, want.data_ptr(), None))
        np.testing.assert_array_equal(got[i], want[0].cpu().numpy(), err_msg=f"page {i} {tuple(p.shape)}")
        if p.shape[0] * p.shape[1] <= 700 * 700:         # the CPU oracle on the smaller pages (it is slow on the big ones)
            ref = P.normalize_det(P.resize_linear_u8(p.cpu().numpy(), (W, H)))
            np.testing.assert_array_equal(got[i], ref, err_msg=f"page {i} vs oracle")


def test_resize_normalize_pages_invalid_entry_and_unaligned_identity_page():
    L, lib = _L()
    H, W = 64, 96
    img = _pages([(H, W)])[0]
    buf = torch.zeros(H * W * 3 + 1, dtype=torch.uint8, device="cuda")
    buf[1:].copy_(torch.from_numpy(img).reshape(-1))          # an identity-size page at an odd address: the byte path
    t = np.zeros((2, 4), np.int64)
    t[0] = (buf.data_ptr() + 1, H, W, 0)
    tab = torch.from_numpy(t).cuda()                          # entry 1 stays all zero: invalid
    out = torch.empty((2, 3, H, W), device="cuda")
    L.check(lib.ocrvi_resize_normalize_pages(0, tab.data_ptr(), 2, H, W, out.data_ptr(), None))
    d = torch.from_numpy(img).cuda()
    want = torch.empty((1, 3, H, W), device="cuda")
    L.check(lib.ocrvi_normalize_u8(0, d.data_ptr(), 1, H, W, want.data_ptr(), None))
    assert torch.equal(out[0], want[0])
    zero = torch.empty((1, 3, H, W), device="cuda")
    z = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    L.check(lib.ocrvi_normalize_u8(0, z.data_ptr(), 1, H, W, zero.data_ptr(), None))
    assert torch.equal(out[1], zero[0])


def _crop_rects(sizes, oh, rng):
    rects = []
    for pg, (h, w) in enumerate(sizes):
        for _ in range(12):
            bw, bh = int(rng.integers(1, w)), int(rng.integers(1, min(h, 120)))
            rects.append((pg, int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh)), bw, bh))
        rects += [(pg, 3, 4, 2 * 60, 2 * oh),           # exact 2x decimation -> area path
                  (pg, 0, 0, w, h),                     # the whole page, squashed
                  (pg, w - 5, h - 7, 40, 40),           # over the right / bottom edge: clamped
                  (pg, -6, -3, 30, 20),                 # negative origin: clamped, width not reduced by the shift
                  (pg, 5, 5, 0, 10), (pg, 5, 5, 10, 0)]  # empty
    return rects


@pytest.mark.parametrize("oh,ow", [(32, 256), (48, 320)])
def test_crop_resize_normalize_pages_equals_the_single_page_kernel(oh, ow):
    L, lib = _L()
    sizes = [(192, 400), (333, 1001), (700, 300), (130, 140)]
    pages = [torch.from_numpy(p).cuda() for p in _pages(sizes, seed=3)]
    tab = _table(pages)
    rng = np.random.default_rng(4)
    rects = _crop_rects(sizes, oh, rng) + [(len(pages), 0, 0, 10, 10), (-1, 0, 0, 10, 10), (1 << 30, 0, 0, 10, 10)]   # bad indices
    b = torch.from_numpy(np.asarray(rects, np.int32)).cuda()
    out = torch.empty((len(rects), 3, oh, ow), device="cuda")
    L.check(lib.ocrvi_crop_resize_normalize_pages(0, tab.data_ptr(), len(pages), b.data_ptr(), len(rects), oh, ow, out.data_ptr(), None))
    got = out.cpu()
    for j, (pg, x, y, w, h) in enumerate(rects):
        if not 0 <= pg < len(pages):
            assert not got[j].any(), j
            continue
        p = pages[pg]
        one = torch.from_numpy(np.asarray([(0, x, y, w, h)], np.int32)).cuda()
        want = torch.empty((1, 3, oh, ow), device="cuda")
        L.check(lib.ocrvi_crop_resize_normalize(0, p.data_ptr(), 1, p.shape[0], p.shape[1], one.data_ptr(), 1, oh, ow, want.data_ptr(), None))
        assert torch.equal(got[j], want[0].cpu()), (j, rects[j])
        if w <= 0 or h <= 0:
            assert not got[j].any()


def test_crop_graph_reads_the_pages_the_table_points_at_after_the_arena_moved():
    L, lib = _L()
    oh, ow = 32, 256
    sizes = [(192, 400), (333, 1001)]
    imgs_a, imgs_b = _pages(sizes, seed=10), _pages(sizes, seed=20)
    rects = np.asarray([(0, 10, 20, 200, 40), (1, 100, 50, 300, 30), (1, 0, 0, 1001, 333), (0, 5, 5, 0, 3)], np.int32)
    s = torch.cuda.Stream()
    tab = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    d_rects = torch.from_numpy(rects).cuda()
    out = torch.empty((len(rects), 3, oh, ow), device="cuda")

    def fill(imgs):
        arena = torch.empty(sum(h * w * 3 + 256 for h, w in sizes), dtype=torch.uint8, device="cuda")
        t, off = np.zeros((2, 4), np.int64), 0
        for i, im in enumerate(imgs):
            arena[off:off + im.size].copy_(torch.from_numpy(im).reshape(-1))
            t[i] = (arena.data_ptr() + off, im.shape[0], im.shape[1], 0)
            off += (im.size + 255) // 256 * 256
        tab.copy_(torch.from_numpy(t))
        torch.cuda.synchronize()
        return arena

    def launch():
        L.check(lib.ocrvi_crop_resize_normalize_pages(0, tab.data_ptr(), 2, d_rects.data_ptr(), len(rects), oh, ow, out.data_ptr(), s.cuda_stream))

    def want(imgs):
        res = []
        for pg, x, y, w, h in rects:
            d = torch.from_numpy(imgs[pg]).cuda()
            o = torch.empty((1, 3, oh, ow), device="cuda")
            one = torch.from_numpy(np.asarray([(0, x, y, w, h)], np.int32)).cuda()
            L.check(lib.ocrvi_crop_resize_normalize(0, d.data_ptr(), 1, d.shape[0], d.shape[1], one.data_ptr(), 1, oh, ow, o.data_ptr(), None))
            res.append(o[0])
        torch.cuda.synchronize()
        return torch.stack(res)

    arena_a = fill(imgs_a)
    with torch.cuda.stream(s):
        launch()                                     # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want(imgs_a))
    arena_b = fill(imgs_b)                           # a new arena at another address; only the table's contents change
    del arena_a
    assert int(tab[0, 0]) == arena_b.data_ptr()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want(imgs_b))
    assert not torch.equal(want(imgs_a), want(imgs_b))
