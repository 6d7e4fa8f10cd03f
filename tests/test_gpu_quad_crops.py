"""ocrvi_crop_quad_resize_normalize_pages / ocrvi_crop_quad_resize_normalize (include/ocrvi.h, "Oriented text crops") on the device: float32-equal
to tests/quad_ref.crop_quad_preprocess (warp with a replicate border, then the recogniser's resize / pad / normalise), equal to the composition
of the two existing entries where that is defined, and equal to the rectangle crop on translation descriptors."""
import math

import numpy as np
import pytest
import torch

import quad_ref as QR
import warp_ref as WR

pytestmark = pytest.mark.gpu

PAGE_SIZES = [(97, 131), (64, 200)]
N_TABLE = 3          # two pages and an invalid entry


def _pages():
    rng = np.random.default_rng(42)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGE_SIZES]


def rot(cx, cy, w, h, deg):
    """Destination -> source matrix of a w x h crop centred on (cx, cy) whose rows run at ``deg`` degrees."""
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    ox, oy = (w - 1) / 2, (h - 1) / 2
    return np.array([c, -s, cx - c * ox + s * oy, s, c, cy - s * ox - c * oy, 0, 0, 1], np.float64)


def shift(x, y):
    return np.array([1, 0, x, 0, 1, y, 0, 0, 1], np.float64)


def descriptors(oh, ow):
    """[(page, w, h, m_inv, what)]: every path of the kernel for an oh x ow output."""
    D = []

    def add(what, pg, w, h, m):
        D.append((pg, int(w), int(h), np.asarray(m, np.float64).reshape(9), what))

    add("height 9: enlarging, +3 degrees", 0, 40, 9, rot(60, 45, 40, 9, 3))
    add("height = out_h: identity rows, -3 degrees", 1, 100, oh, rot(100, 32, 100, oh, -3))
    add("height 2 out_h with w = 2 new_w: the box filter", 0, 120, 2 * oh, rot(65, 48, 120, 2 * oh, 0.7))
    add("height 2 out_h, w odd: not the box filter", 1, 121, 2 * oh, rot(100, 32, 121, 2 * oh, -0.7))
    add("height 2 out_h + 1: skipped rows, +30 degrees", 0, 80, 2 * oh + 1, rot(65, 48, 80, 2 * oh + 1, 30))
    add("height 150: skipped rows, -30 degrees", 1, 60, 150, rot(100, 32, 60, 150, -30))
    add("new_w below out_w", 1, ow // 2 - 28, oh // 2, rot(100, 30, ow // 2 - 28, oh // 2, 3))
    add("new_w equal to out_w", 1, ow // 2, oh // 2, rot(100, 30, ow // 2, oh // 2, -3))
    add("new_w above out_w: squash", 1, ow // 2 + 22, oh // 2, rot(100, 30, ow // 2 + 22, oh // 2, 3))
    add("box filter at the full width", 0, 2 * ow, 2 * oh, rot(65, 48, 2 * ow, 2 * oh, 1.5))
    add("new_w = 0 -> 1", 0, 3, 100, rot(65, 48, 3, 100, -3))
    add("new_w = 1", 1, 1, 40, rot(100, 32, 1, 40, 3))
    add("one pixel past a 64-column tile", 1, 65, oh, rot(100, 32, 65, oh, 3))
    add("one pixel past two 64-column tiles", 1, 129, oh, rot(100, 32, 129, oh, -3))
    add("wider than a column tile", 1, 200, oh, rot(100, 32, 200, oh, 0.3))
    # more than 128 source columns under one 64-column tile: the tile form's compact column slots (2 out_h + 1 rows: compact row slots too)
    add("shrunk by more than 2 in both axes", 0, 2 * ow + 88, 2 * oh + 1, rot(65, 48, 2 * ow + 88, 2 * oh + 1, 2))
    add("44 degrees", 0, 70, 12, rot(65, 48, 70, 12, 44))
    add("-44 degrees", 1, 90, 14, rot(100, 30, 90, 14, -44))
    # a true perspective matrix: the four-point geometry of a trapezoid
    _, _, w, h, _, m_inv = WR.four_point_geometry([(20, 15), (110, 8), (120, 80), (12, 60)])
    assert m_inv[2, 0] != 0 and m_inv[2, 1] != 0
    add("perspective", 0, w, h, m_inv)
    add("overhangs the left edge", 0, 50, 10, rot(5, 48, 50, 10, 3))
    add("overhangs the right edge", 0, 50, 10, rot(126, 48, 50, 10, -3))
    add("overhangs the top edge", 0, 50, 10, rot(65, 2, 50, 10, 3))
    add("overhangs the bottom edge", 0, 50, 10, rot(65, 95, 50, 10, -3))
    add("overhangs a corner, translation", 1, 40, 20, shift(-7, 50))
    add("wholly outside: every tap clamped", 1, 30, 12, rot(-500, -400, 30, 12, 10))
    add("translation inside", 1, 90, 21, shift(17, 9))
    add("w = 0", 0, 0, 12, shift(3, 3))
    add("h = 0", 0, 12, 0, shift(3, 3))
    add("w < 0", 1, -5, 12, shift(3, 3))
    add("page -1", -1, 30, 12, shift(3, 3))
    add("page n_pages", N_TABLE, 30, 12, shift(3, 3))
    add("invalid table entry", 2, 30, 12, shift(3, 3))
    return D


_REF = {}


def _reference(size):
    """(descriptors, float32 [B,3,oh,ow]) for an output size: computed once, shared, never modified."""
    if size not in _REF:
        pages = _pages()
        D = descriptors(*size)
        out = np.stack([QR.crop_quad_preprocess(pages[pg] if 0 <= pg < len(pages) else None, (pg, w, h, 0), m, size) for pg, w, h, m, _ in D])
        out.setflags(write=False)
        _REF[size] = (D, out)
    return _REF[size]


def _table(pages_dev, n=N_TABLE):
    rows = [(p.data_ptr(), p.shape[0], p.shape[1], 0) for p in pages_dev]
    rows += [(0, 40, 40, 0)] * (n - len(rows))                    # a null address: invalid, never dereferenced
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


def _run_pages(table, n_pages, D, size, form="tile"):
    """The pages entry on descriptors D.  ``form``: the library takes its tile form (a workgroup per 64-column tile, 16-byte stores) when the
    output is 16-byte aligned and its direct form (a thread per pixel) otherwise: "direct" hands it an output 4 bytes past an aligned one."""
    from ocr_vi_invoice_amd import _lib
    crops = torch.tensor([(pg, w, h, 0) for pg, w, h, _, _ in D], dtype=torch.int32, device="cuda")
    mats = torch.from_numpy(np.stack([m for _, _, _, m, _ in D])).cuda()
    n = len(D) * 3 * size[0] * size[1]
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:n + 1].view((len(D), 3) + tuple(size)) if form == "direct" else buf[:n].view((len(D), 3) + tuple(size))
    _lib.check(_lib.load().ocrvi_crop_quad_resize_normalize_pages(0, table.data_ptr(), n_pages, crops.data_ptr(), mats.data_ptr(), len(D), size[0],
                                                                   size[1], out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


def test_descriptor_set_covers_the_paths():
    """A self-check of this file's descriptor list (it runs no library code): the cases the comparison below relies on are in it."""
    D, _ = _reference((32, 256))
    assert len(D) >= 24
    new_w = [int(w * (32 / h)) for _, w, h, _, _ in D if w > 0 and h > 0]
    assert min(new_w) == 0 and 256 in new_w and max(new_w) > 256 and 65 in new_w and 129 in new_w
    assert {9, 32, 64, 65, 150} <= {h for _, _, h, _, _ in D}


@pytest.mark.parametrize("form", ["tile", "direct"])
@pytest.mark.parametrize("size", [(32, 256), (48, 320), (32, 100)], ids=["32x256", "48x320", "32x100"])   # 100: a partial last column tile
def test_equals_the_reference(size, form):
    D, want = _reference(size)
    pages_dev = [torch.from_numpy(p).cuda() for p in _pages()]
    got = _run_pages(_table(pages_dev), N_TABLE, D, size, form)
    for i, (pg, w, h, _, what) in enumerate(D):
        diff = got[i] != want[i]
        if diff.any():
            c, y, x = np.argwhere(diff)[0]
            raise AssertionError(f"{what} (page {pg}, {w} x {h}): {diff.sum()} elements differ, first at c {c} y {y} x {x}: {got[i, c, y, x]!r} "
                                 f"!= {want[i, c, y, x]!r}")
    assert got.tobytes() == want.tobytes()
    zeros = [i for i, d in enumerate(D) if d[1] <= 0 or d[2] <= 0 or not 0 <= d[0] < 2]
    assert len(zeros) == 6 and not got[zeros].any()


def test_single_image_entry_equals_the_pages_entry():
    from ocr_vi_invoice_amd import pipeline
    size = (32, 256)
    D, want = _reference(size)
    page1 = torch.from_numpy(_pages()[1]).cuda()
    pick = [i for i, d in enumerate(D) if d[0] == 1]
    crops = [(0, D[i][1], D[i][2], 0) for i in pick] + [(1, 30, 12, 0), (-1, 30, 12, 0)]      # image index 0; 1 and -1 are out of range
    mats = [D[i][3] for i in pick] + [shift(3, 3)] * 2
    got = pipeline.preprocess_crops_quad(page1[None], crops, mats, size).cpu().numpy()
    assert got[:len(pick)].tobytes() == want[pick].tobytes()
    assert not got[len(pick):].any()


def test_equals_warp_then_rectangle_crop_inside_the_page():
    """Quads wholly inside the page: every tap is in range, the constant border of ocrvi_warp_perspective_u8 never shows, and the output is
    the composition of the two existing entries: the warp into a scratch image, then ocrvi_crop_resize_normalize on all of it."""
    from ocr_vi_invoice_amd import pipeline
    size = (32, 256)
    page = _pages()[0]
    page_dev = torch.from_numpy(page).cuda()
    D = [(0, 60, 20, rot(65, 48, 60, 20, 10), ""), (0, 90, 9, rot(65, 48, 90, 9, -3), ""), (0, 40, 32, rot(65, 48, 40, 32, 30), ""),
         (0, 50, 64, rot(65, 48, 50, 64, 3), ""), (0, 30, 70, rot(65, 48, 30, 70, -30), ""), (0, 100, 11, rot(65, 48, 100, 11, 20), "")]
    for _, w, h, m, _ in D:
        X, Y = WR.warp_coords(m, h, w)
        assert X.min() >= 0 and Y.min() >= 0 and (X.max() >> 5) + 1 < page.shape[1] and (Y.max() >> 5) + 1 < page.shape[0]
    got = _run_pages(_table([page_dev]), N_TABLE, D, size)
    for i, (_, w, h, m, _) in enumerate(D):
        scratch = pipeline.warp_perspective(page_dev, m, h, w)
        want = pipeline.preprocess_crops(scratch[None], [(0, 0, 0, w, h)], size).cpu().numpy()[0]
        assert got[i].tobytes() == want.tobytes(), (w, h)


def test_translation_descriptors_equal_the_rectangle_entry():
    from ocr_vi_invoice_amd import _lib
    pages_dev = [torch.from_numpy(p).cuda() for p in _pages()]
    table = _table(pages_dev)
    rects = [(0, 3, 5, 100, 20), (1, 0, 0, 200, 64), (0, 10, 20, 64, 64), (1, 50, 10, 9, 40), (0, 130, 96, 1, 1), (1, 20, 0, 150, 9),
             (0, 0, 0, 131, 97), (1, 7, 0, 128, 64)]
    assert all(x >= 0 and y >= 0 and x + w <= PAGE_SIZES[pg][1] and y + h <= PAGE_SIZES[pg][0] for pg, x, y, w, h in rects)
    D = [(pg, w, h, shift(x, y), "") for pg, x, y, w, h in rects]
    for size, form in (((32, 256), "tile"), ((48, 320), "tile"), ((32, 64), "tile"), ((32, 100), "tile"), ((32, 256), "direct"),
                       ((32, 66), "tile")):   # 100: a partial last column tile; 66 % 4 != 0: direct
        got = _run_pages(table, N_TABLE, D, size, form)
        r = torch.tensor(rects, dtype=torch.int32, device="cuda")
        want = torch.empty((len(rects), 3) + size, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ocrvi_crop_resize_normalize_pages(0, table.data_ptr(), N_TABLE, r.data_ptr(), len(rects), size[0], size[1],
                                                                  want.data_ptr(), torch.cuda.current_stream().cuda_stream))
        assert got.tobytes() == want.cpu().numpy().tobytes(), size


def test_tilted_line_fills_the_crop():
    """A white page with one black rectangle tilted by 10 degrees: the oriented crop of its exact quad is ink all the way into the corners,
    the rectangle crop of the same box starts with paper."""
    from ocr_vi_invoice_amd import _lib, pipeline
    size = (32, 256)
    H, W, L, T = 120, 200, 100.5, 66.5
    a = math.radians(10)
    u, v, c = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)]), np.array([100.0, 60.0])
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.stack([xx, yy], -1) - c
    inside = (np.abs(d @ u) <= L / 2) & (np.abs(d @ v) <= T / 2)
    page = np.where(inside[:, :, None], 0, 255).astype(np.uint8).repeat(3, axis=2)
    quad = np.array([c - u * L / 2 - v * T / 2, c + u * L / 2 - v * T / 2, c + u * L / 2 + v * T / 2, c - u * L / 2 + v * T / 2])
    crops, mats = np.empty((1, 4), np.int32), np.empty((1, 9))
    ids, hw, flags = np.zeros(1, np.int32), np.array([[H, W]], np.int32), np.zeros(1, np.int32)
    _lib.check(_lib.load().ocrvi_quad_crops(quad.ctypes.data, flags.ctypes.data, 1, ids.ctypes.data, hw.ctypes.data, crops.ctypes.data, mats.ctypes.data))
    assert crops[0].tolist() == [0, 100, 66, 0]
    page_dev = torch.from_numpy(page).cuda()
    got = pipeline.preprocess_crops_quad(page_dev[None], crops, mats, size).cpu().numpy()[0]
    assert got.tobytes() == QR.crop_quad_preprocess(page, crops[0], mats[0], size).tobytes()
    new_w = int(100 * (32 / 66))
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    ink, paper = (np.float32(0) - mean) / std, (np.float32(1) - mean) / std
    inner = got[:, 2:size[0] - 2, 2:new_w - 2]
    assert inner.size and (inner == ink[:, None, None]).all()
    assert (got[:, :, new_w:] == paper[:, None, None]).all()                        # the padding
    # the reference's crop of the same box: the bounding rectangle, whose corner lies outside the tilted line
    x, y, bw, bh = pipeline.crop_rect((H, W), np.stack([np.floor(quad.min(0)), np.ceil(quad.max(0))]).astype(np.int64))
    rect = pipeline.preprocess_crops(page_dev[None], [(0, x, y, bw, bh)], size).cpu().numpy()[0]
    assert (rect[:, 0, 0] == paper).all() and (got[:, 2, 2] == ink).all()
