"""Skew estimate, device half (csrc/skew.hip; include/ocrvi.h, "Skew estimate"): the stage entries against the numpy statement in
tests/skew_ref.py for equality, the batched page-table entry against the stages (guards, poisoned workspace, refused pages, a captured
graph that follows a rewritten table), and the facades on a rotated synthetic invoice."""
import ctypes

import numpy as np
import pytest
import torch

import docfind_ref as DR
import skew_ref as SR

pytestmark = pytest.mark.gpu

K = SR.K
GUARD = 0x5A5A5A5A5A5A5A5A


def _lib():
    from ocr_vi_invoice_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_edges(g):
    L = _lib()
    src, out = _dev(g), torch.full(g.shape, 0xAB, dtype=torch.uint8, device="cuda")
    L.check(L.load().ocrvi_skew_edges_u8(0, src.data_ptr(), g.shape[0], g.shape[1], out.data_ptr(), _stream()))
    return out.cpu().numpy()


def gpu_scores(e):
    L = _lib()
    src, out = _dev(e), torch.full((SR.ANGLES + 2,), GUARD, dtype=torch.int64, device="cuda")
    L.check(L.load().ocrvi_skew_scores(0, src.data_ptr(), e.shape[0], e.shape[1], out[1:].data_ptr(), _stream()))
    host = out.cpu().numpy().view(np.uint64)
    assert host[0] == GUARD and host[-1] == GUARD
    return host[1:-1]


def gpu_grey(img, work_h):
    L = _lib()
    ww, _ = DR.working_size(img.shape[0], img.shape[1], work_h)
    src, out = _dev(img), torch.full((work_h, ww), 0xAB, dtype=torch.uint8, device="cuda")
    L.check(L.load().ocrvi_doc_grey_u8(0, src.data_ptr(), img.shape[0], img.shape[1], work_h, out.data_ptr(), _stream()))
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("case", [0, 1, 2], ids=["8x8", "37x101", "64x257"])
def test_edges_around_the_floor_and_at_both_borders(case):
    g = SR.grey_cases()[case]
    want = SR.edges(g)
    assert g.shape == ((8, 8), (37, 101), (64, 257))[case] and 8 in want and 9 in want and 7 not in want and want[:, 0].any() and want[:, -1].any()
    assert np.array_equal(gpu_edges(g), want)


def test_one_pixel_scores_its_square_at_every_slope():
    for (h, ww), (i, j, v) in (((37, 101), (5, 70, 200)), ((8, 8), (0, 0, 255)), ((64, 8192), (63, 8191, 3))):
        e = np.zeros((h, ww), np.uint8)
        e[i, j] = v
        assert (gpu_scores(e) == v * v).all()


@pytest.mark.parametrize("h,ww,p0,p1", [(37, 101, (10, 3, 200), (14, 97, 31)), (64, 300, (40, 147, 7), (41, 150, 250)), (20, 8, (3, 0, 90), (2, 7, 100)),
                                        (64, 8192, (10, 0, 255), (58, 8191, 255))])
def test_two_pixels_meet_exactly_where_their_offsets_say(h, ww, p0, p1):
    (i0, j0, v0), (i1, j1, v1) = p0, p1
    assert j0 < (ww >> 1) <= j1
    e = np.zeros((h, ww), np.uint8)
    e[i0, j0], e[i1, j1] = v0, v1

    def o(j, k):
        return ((j - (ww >> 1)) * k + 256) >> 9                           # Python integers: >> floors

    meet = [k for k in range(-K, K + 1) if i0 - o(j0, k) == i1 - o(j1, k)]
    assert 0 < len(meet) < SR.ANGLES
    want = np.array([(v0 + v1) ** 2 if k in meet else v0 * v0 + v1 * v1 for k in range(-K, K + 1)], np.uint64)
    assert np.array_equal(SR.scores(e), want) and np.array_equal(gpu_scores(e), want)


@pytest.mark.parametrize("name", ["random_8x8", "random_512x8", "random_37x101", "random_64x8192"])
def test_scores_of_random_bytes(name):
    e = SR.score_cases()[name]
    assert np.array_equal(gpu_scores(e), SR.scores(e))


def test_scores_that_need_64_bits():
    want = SR.scores_constant(512, 8192, 255)
    assert int(want[K]) == 512 * (255 * 8192) ** 2 and (255 * 8192) ** 2 > 2 ** 32
    assert np.array_equal(gpu_scores(SR.score_cases()["all_255_512x8192"]), want)


# ---------------------------------------------------------------------------------------------------- the batched entry
def _noisy(seed, h, w):
    """Slanted dark bars on a noisy light page."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    img = 215 + rng.integers(-25, 26, (h, w))
    img[((ys * 8 + xs * (seed % 5 - 2)) // max(h // 4, 8)) % 3 == 0] -= 150
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8)[:, :, None].repeat(3, axis=2))


WORK_H = 64


def _page_set():
    rng = np.random.default_rng(3300)
    wide = np.ascontiguousarray(rng.integers(0, 256, (64, 8192, 1), dtype=np.uint8).repeat(3, axis=2))
    return [_noisy(1, 100, 130), wide, None, _noisy(2, 296, 300), _noisy(3, 64, 8), np.zeros((32, 8000, 3), np.uint8), _noisy(4, 37, 333)]


def _table(devs):
    return np.array([(0, 7, 7, 0) if d is None else (d.data_ptr(), d.shape[0], d.shape[1], 0) for d in devs], np.int64)


def test_pages_of_mixed_sizes_in_one_call_and_in_a_captured_graph():
    L = _lib()
    lib = L.load()
    imgs = _page_set()
    n, ww_cap = len(imgs), 8192
    refused = (2, 5)                                 # an invalid entry; a page 16000 working pixels wide
    want = np.zeros((n, SR.ANGLES), np.uint64)
    for i, im in enumerate(imgs):
        if i not in refused:
            g = DR.grey(im, WORK_H)
            want[i] = SR.scores(SR.edges(g))
            assert np.array_equal(gpu_scores(gpu_edges(gpu_grey(im, WORK_H))), want[i])      # the stage entries on that page
    assert len({DR.grey(im, WORK_H).shape for i, im in enumerate(imgs) if i not in refused}) == 5 and want[[0, 1, 3, 4, 6]].any(1).all()
    devs = [None if im is None else _dev(im) for im in imgs]
    ws = ctypes.c_size_t(0)
    L.check(lib.ocrvi_skew_sizes(n, WORK_H, ww_cap, ctypes.byref(ws)))
    table = _dev(_table(devs))
    work = torch.full((ws.value,), 0xCD, dtype=torch.uint8, device="cuda")
    buf = torch.full((n * SR.ANGLES + 16,), GUARD, dtype=torch.int64, device="cuda")
    scores = buf[8:8 + n * SR.ANGLES]

    def call():
        L.check(lib.ocrvi_skew_scores_pages(0, table.data_ptr(), n, WORK_H, ww_cap, scores.data_ptr(), work.data_ptr(), ws.value, _stream()))

    def result():
        torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint64)
        assert (host[:8] == GUARD).all() and (host[-8:] == GUARD).all()
        return host[8:-8].reshape(n, SR.ANGLES)

    call()
    assert np.array_equal(result(), want)
    assert lib.ocrvi_skew_scores_pages(0, table.data_ptr(), n, WORK_H, ww_cap, scores.data_ptr(), work.data_ptr(), ws.value - 1, _stream()) == -3
    # twice in one captured graph; between replays a page moves and the table is rewritten in place
    scores.fill_(GUARD)
    work.fill_(0xCD)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
        call()
    torch.cuda.synchronize()
    assert (buf == GUARD).all()                      # captured, not run
    graph.replay()
    assert np.array_equal(result(), want)
    moved = [devs[6].clone(), devs[3].clone(), devs[0], None, devs[4], devs[1], devs[5]]
    devs[6].zero_(), devs[3].zero_()                 # the old copies no longer hold the pages
    table.copy_(torch.from_numpy(_table(moved)))
    graph.replay()
    assert np.array_equal(result(), want[[6, 3, 0, 2, 4, 1, 5]])


# ---------------------------------------------------------------------------------------------------- facades
_CACHE = {}


def _rotated_page():
    if not _CACHE:
        from ocr_vi_invoice_amd import synth
        page = synth.make_invoice(1, 960, 1280, 30)[0]
        _CACHE["straight"] = page
        _CACHE["rotated"] = SR.rotated(page, 3, enclose=False)
        assert _CACHE["rotated"].shape == (960, 1280, 3)
    return _CACHE["straight"], _CACHE["rotated"]


def _close(got, want):
    return isinstance(got, tuple) and got.k == want.k and got.angle == pytest.approx(want.angle, rel=1e-12) and got.gain == pytest.approx(want.gain, rel=1e-12)


def test_estimate_skews_on_arrays_tensors_jpeg_and_png_bytes():
    from ocr_vi_invoice_amd import pipeline
    straight, rot = _rotated_page()
    jpeg, png = pipeline.imencode(rot, 90), pipeline.imencode_png(rot)
    want = SR.estimate(rot)
    want_jpeg = SR.estimate(pipeline.imdecode(jpeg).cpu().numpy())
    assert abs(want.k - 27) <= 2 and abs(want_jpeg.k - 27) <= 2
    got = pipeline.estimate_skews([rot, _dev(rot), jpeg, png, np.zeros((2000, 10, 3), np.uint8), straight])
    assert all(_close(g, w) for g, w in zip(got[:4], [want, want, want_jpeg, want])) and got[4] is None
    assert got[5].k == 0 and got[5].gain == 1.0 and got[5].angle == 0.0
    assert _close(pipeline.estimate_skew(_dev(rot)), want) and pipeline.estimate_skews([]) == []
    flat = pipeline.estimate_skew(np.full((64, 48, 3), 9, np.uint8))
    assert flat == pipeline.Skew(0, 0.0, 1.0)


def test_deskew_turns_a_rotated_page_and_leaves_a_straight_one():
    from ocr_vi_invoice_amd import pipeline
    straight, rot = _rotated_page()
    same, skew = pipeline.deskew(straight)
    assert same is straight and skew.k == 0
    tensor = _dev(straight)
    assert pipeline.deskew(tensor)[0] is tensor
    out, skew = pipeline.deskew(rot)
    assert skew.k == SR.estimate(rot).k != 0 and isinstance(out, np.ndarray)
    want = pipeline.four_point_transform(rot, pipeline.skew_quad(960, 1280, skew.k))
    assert out.shape == want.shape and out.shape[0] > 960 and out.shape[1] > 1280 and np.array_equal(out, want)
    dout, dskew = pipeline.deskew(_dev(rot))
    assert dout.is_cuda and dskew == skew and np.array_equal(dout.cpu().numpy(), want)
    assert abs(pipeline.estimate_skew(out).k) <= 2
    kept, kskew = pipeline.deskew(rot, min_gain=100.0)                # a stricter caller: the estimate is returned, the page kept
    assert kept is rot and kskew == skew
