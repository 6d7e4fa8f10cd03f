"""Four-point rectification on the device: ``ocrvi_warp_perspective_u8`` / ``ocrvi_warp_perspective_pages`` bit for bit against the
numpy statement of the same arithmetic (tests/warp_ref.py), ``pipeline.four_point_transform`` end to end, and ``Engine.run(pages, quads)``
against the per-page call and against the engine fed with pages rectified beforehand."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [(5.5, 3.2), (48.1, 6.7), (50.3, 33.9), (2.2, 30.1)]
SENTINEL = 0xAB
PAD = 64


def _L():
    from ocr_vi_invoice_amd import _lib
    return _lib, _lib.load()


def _src(seed=0, h=37, w=53):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _warp_single(src, m, dh, dw, shift=0):
    """``ocrvi_warp_perspective_u8`` into a buffer of sentinel bytes, the destination ``PAD + shift`` bytes in; the bytes either side of
    it must come back untouched."""
    L, lib = _L()
    d_src = torch.from_numpy(src).cuda()
    nb = dh * dw * 3
    buf = torch.full((nb + 2 * PAD + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    m = np.ascontiguousarray(np.asarray(m, np.float64).reshape(9))
    off = PAD + shift
    L.check(lib.ocrvi_warp_perspective_u8(0, d_src.data_ptr(), src.shape[0], src.shape[1], m.ctypes.data, buf.data_ptr() + off, dh, dw,
                                          torch.cuda.current_stream().cuda_stream))
    out = buf.cpu().numpy()
    assert (out[:off] == SENTINEL).all() and (out[off + nb:] == SENTINEL).all()
    return out[off:off + nb].reshape(dh, dw, 3)


def _small_quad_inverse():
    from ocr_vi_invoice_amd import pipeline
    _, m_inv, w, h = pipeline.four_point_geometry(SMALL)
    assert (w, h) == (48, 27)
    return m_inv


BORDERS = np.array([[1.3, 0.2, -8.0], [0.1, 1.4, -9.0], [0.002, 0.001, 1.0]])
CASES = {
    "identity": (np.eye(3), 37, 53),
    "integer_translation": (np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1.0]]), 37, 53),
    "fractional_translation": (np.array([[1, 0, 2.3], [0, 1, -1.7], [0, 0, 1.0]]), 37, 53),
    "small_quad": (None, 27, 48),
    "projective_across_all_borders": (BORDERS, 50, 70),
    "down_2x": (np.diag([2.0, 2.0, 1.0]), 18, 26),
    "up_3x": (np.diag([1 / 3, 1 / 3, 1.0]), 111, 159),
    "zero_denominator": (np.array([[1, 0, 0], [0, 1, 0], [1, 0, -5.0]]), 20, 30),
    "beyond_int32": (np.array([[1e8, 0, 0], [0, 1, 0], [0, 0, 1.0]]), 20, 30),
    "beyond_int32_negative": (np.array([[-1e9, 0, -1e9], [0, -1e9, -1e9], [0, 0, 1.0]]), 9, 11),
}


@pytest.mark.parametrize("name", list(CASES))
def test_warp_u8_is_bit_equal_to_the_reference(name):
    m, dh, dw = CASES[name]
    if m is None:
        m = _small_quad_inverse()
    src = _src()
    want = WR.warp_perspective(src, m, dh, dw)
    X, Y = WR.warp_coords(m, dh, dw)
    # each case does exercise what its name says
    if name == "identity":
        assert np.array_equal(want, src)
    if name == "projective_across_all_borders":
        sx, sy = X >> 5, Y >> 5
        assert sx.min() < -1 and sx.max() > 53 and sy.min() < -1 and sy.max() > 37
        assert ((sx == -1) & (sy >= 0) & (sy < 37)).any() and ((sx == 52) & (X & 31 > 0)).any()       # half-inside taps on both sides
        assert ((sy == -1) & (sx >= 0) & (sx < 53)).any() and ((sy == 36) & (Y & 31 > 0)).any()
    if name == "zero_denominator":
        assert (X[:, 5] == 0).all() and (Y[:, 5] == 0).all() and np.array_equal(want[:, 5], np.broadcast_to(src[0, 0], (dh, 3)))
    if name == "beyond_int32":
        assert (X[:, 1:] == 2147483647).all() and (X[:, 0] == 0).all() and not want[:, 1:].any() and want[:, 0].any()
    if name == "beyond_int32_negative":
        assert (X == -2147483648).all() and (Y == -2147483648).all() and not want.any()
    assert want.any() or name == "beyond_int32_negative"
    for shift in (0, 1):              # a destination that is a multiple of 4 (word stores) and an odd one (byte stores)
        got = _warp_single(src, m, dh, dw, shift)
        assert np.array_equal(got, want), (name, shift, int((got != want).sum()))


def test_warp_u8_of_a_real_quad_on_a_larger_page():
    from ocr_vi_invoice_amd import pipeline, synth
    src = synth.make_invoice(5, 400, 300, lines=6)[0]
    _, m_inv, w, h = pipeline.four_point_geometry([(20.5, 15.2), (280.3, 30.8), (270.1, 390.4), (10.7, 370.9)])
    assert 250 <= w <= 270 and 350 <= h <= 370
    want = WR.warp_perspective(src, m_inv, h, w)
    assert np.array_equal(_warp_single(src, m_inv, h, w), want)
    assert np.array_equal(_warp_single(src, m_inv, h, w, shift=3), want)


def test_warp_u8_rejects_bad_arguments():
    L, lib = _L()
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    m = np.eye(3).reshape(9)
    for args in ((None, 4, 4, m.ctypes.data, d.data_ptr(), 2, 2), (d.data_ptr(), 0, 4, m.ctypes.data, d.data_ptr(), 2, 2),
                 (d.data_ptr(), 4, 4, None, d.data_ptr(), 2, 2), (d.data_ptr(), 4, 4, m.ctypes.data, d.data_ptr(), 2, -1)):
        assert lib.ocrvi_warp_perspective_u8(0, *args, None) == -1 and L.last_error()
    assert lib.ocrvi_warp_perspective_pages(0, d.data_ptr(), d.data_ptr(), d.data_ptr(), 0, None) == -1


class _PageSet:
    """Sources, matrices and destination sizes of a launch; destinations are carved out of one buffer of sentinel bytes at the given byte
    offsets.  ``src_ok[i]`` False: the source entry is invalid (zeros expected); ``dst_mode[i]``: 'ok', 'null' (no address) or 'empty'
    (an address inside the buffer but height 0) -- the last two must leave every byte as it was."""

    def __init__(self, specs, seed):
        from ocr_vi_invoice_amd import _lib
        self.specs = specs
        self.srcs = [torch.from_numpy(_src(seed + i, sh, sw)).cuda() for i, (sh, sw, *_r) in enumerate(specs)]
        end = 0
        for (_sh, _sw, _m, dh, dw, off, _ok, _mode) in specs:
            end = max(end, off + dh * dw * 3)
        self.buf = torch.full((end + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        src_t, dst_t, mats = [], [], []
        for s, (sh, sw, m, dh, dw, off, ok, mode) in zip(self.srcs, specs):
            src_t.append((s.data_ptr(), sh, sw, 0) if ok else (0, sh, sw, 0))
            dst_t.append({"ok": (self.buf.data_ptr() + off, dh, dw, 0), "null": (0, dh, dw, 0), "empty": (self.buf.data_ptr() + off, 0, dw, 0)}[mode])
            mats.append(np.asarray(m, np.float64).reshape(9))
        self.src_table = np.asarray(src_t, np.int64).reshape(-1, _lib.PAGE_ENTRY)
        self.dst_table = np.asarray(dst_t, np.int64).reshape(-1, _lib.PAGE_ENTRY)
        self.mats = np.stack(mats)

    def expected(self):
        """The whole buffer as it must look afterwards, each written page through the single-page entry."""
        want = np.full(self.buf.numel(), SENTINEL, np.uint8)
        for s, (sh, sw, m, dh, dw, off, ok, mode) in zip(self.srcs, self.specs):
            if mode != "ok":
                continue
            page = _warp_single(s.cpu().numpy(), m, dh, dw) if ok else np.zeros((dh, dw, 3), np.uint8)
            if ok:
                assert np.array_equal(page, WR.warp_perspective(s.cpu().numpy(), m, dh, dw))
            want[off:off + dh * dw * 3] = page.reshape(-1)
        return want


def _specs_a():
    q = _small_quad_inverse()
    shift = np.array([[1, 0, 2.3], [0, 1, -1.7], [0, 0, 1.0]])
    #        src h, w   matrix   dst h, w   byte offset in the buffer      source ok   destination
    return [(37, 53, q, 27, 48, 256, True, "ok"),
            (41, 29, BORDERS, 33, 35, 256 + 4096 + 1, True, "ok"),          # an odd address
            (20, 64, shift, 19, 21, 256 + 8192 + 2, True, "ok"),            # 2 mod 4; 19 x 21 pixels leave a partial last group
            (37, 53, np.eye(3), 15, 17, 256 + 10240, False, "ok"),          # invalid source: zeros
            (37, 53, np.eye(3), 15, 17, 256 + 12288, True, "null"),         # invalid destinations: skipped
            (37, 53, np.eye(3), 15, 17, 256 + 12288, True, "empty"),
            (37, 53, np.diag([0.5, 0.5, 1.0]), 16, 16, 256 + 14336, True, "ok")]


def test_warp_pages_equals_the_single_form_and_touches_nothing_else():
    L, lib = _L()
    ps = _PageSet(_specs_a(), seed=10)
    want = ps.expected()
    st, dt, mt = torch.from_numpy(ps.src_table).cuda(), torch.from_numpy(ps.dst_table).cuda(), torch.from_numpy(ps.mats).cuda()
    L.check(lib.ocrvi_warp_perspective_pages(0, st.data_ptr(), dt.data_ptr(), mt.data_ptr(), len(ps.specs), torch.cuda.current_stream().cuda_stream))
    got = ps.buf.cpu().numpy()
    for (sh, sw, m, dh, dw, off, ok, mode) in ps.specs:
        if mode == "ok":
            assert np.array_equal(got[off:off + dh * dw * 3], want[off:off + dh * dw * 3]), (off, ok)
    assert np.array_equal(got, want)               # every sentinel byte between, before and after the pages included
    assert not got[256 + 10240:256 + 10240 + 15 * 17 * 3].any() and (got[256 + 12288:256 + 12288 + 15 * 17 * 3] == SENTINEL).all()


def test_warp_pages_strides_over_a_page_larger_than_its_grid():
    """More than 2^20 destination pixels: past what the page's blocks cover in one sweep of 4-pixel groups."""
    L, lib = _L()
    src = _src(3, 61, 67)
    m = np.array([[0.06, 0.004, -0.8], [-0.003, 0.058, 0.9], [1e-5, -2e-5, 1.0]])
    dh, dw = 1031, 1027
    want = WR.warp_perspective(src, m, dh, dw)
    assert dh * dw > (1 << 20) and want[-1].any() and want[0].any()
    d_src = torch.from_numpy(src).cuda()
    out = torch.full((dh * dw * 3 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.tensor([[d_src.data_ptr(), 61, 67, 0]], dtype=torch.int64, device="cuda")
    dt = torch.tensor([[out.data_ptr(), dh, dw, 0]], dtype=torch.int64, device="cuda")
    mt = torch.from_numpy(m.reshape(1, 9)).cuda()
    L.check(lib.ocrvi_warp_perspective_pages(0, st.data_ptr(), dt.data_ptr(), mt.data_ptr(), 1, torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    assert np.array_equal(got[:dh * dw * 3].reshape(dh, dw, 3), want) and (got[dh * dw * 3:] == SENTINEL).all()


def test_warp_pages_graph_survives_moved_pages():
    """Captured once; then other pages at other addresses, other sizes and matrices, written into the SAME tables: the replay computes
    the new set."""
    L, lib = _L()
    a = _PageSet(_specs_a(), seed=10)
    q = _small_quad_inverse()
    b = _PageSet([(29, 31, BORDERS, 30, 30, 512 + 3, True, "ok"),
                  (37, 53, np.eye(3), 9, 9, 512 + 4096, True, "null"),
                  (50, 40, q, 27, 48, 512 + 8192, True, "ok"),
                  (37, 53, np.eye(3), 15, 17, 512 + 16384 + 1, False, "ok"),
                  (37, 53, np.diag([2.0, 2.0, 1.0]), 18, 26, 512 + 20480 + 2, True, "ok"),
                  (37, 53, np.eye(3), 9, 9, 512 + 4096, True, "empty"),
                  (33, 47, np.array([[1, 0, 0.5], [0, 1, 0.25], [0, 0, 1.0]]), 33, 47, 512 + 24576, True, "ok")], seed=40)
    n = len(a.specs)
    assert len(b.specs) == n
    want_a, want_b = a.expected(), b.expected()
    st, dt, mt = torch.from_numpy(a.src_table).cuda(), torch.from_numpy(a.dst_table).cuda(), torch.from_numpy(a.mats).cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.ocrvi_warp_perspective_pages(0, st.data_ptr(), dt.data_ptr(), mt.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(a.buf.cpu().numpy(), want_a)
    a.buf.fill_(SENTINEL)
    st.copy_(torch.from_numpy(b.src_table))
    dt.copy_(torch.from_numpy(b.dst_table))
    mt.copy_(torch.from_numpy(b.mats))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(b.buf.cpu().numpy(), want_b)
    assert (a.buf.cpu().numpy() == SENTINEL).all()              # the first set's pages are no longer written


def test_four_point_transform_end_to_end():
    """Host geometry + device warp against the reference warp under the library's own inverse matrix (the matrices are held to numpy's in
    tests/test_rectify_cpu.py; another solver's last bits could move a 1/32-pixel coordinate across a rounding boundary)."""
    from ocr_vi_invoice_amd import pipeline
    src = _src(7)
    want = WR.warp_perspective(src, _small_quad_inverse(), 27, 48)
    got = pipeline.four_point_transform(src, SMALL)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (27, 48, 3) and np.array_equal(got, want)
    perm = [SMALL[2], SMALL[0], SMALL[3], SMALL[1]]
    dev = pipeline.four_point_transform(torch.from_numpy(src).cuda(), perm)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    assert np.array_equal(pipeline.preprocess_image(src, np.asarray(SMALL)[:, None, :]), want)
    assert pipeline.preprocess_image(src, None) is src
    with pytest.raises(ValueError):
        pipeline.four_point_transform(src, [(10, 0), (20, 10), (10, 20), (0, 10)])
    with pytest.raises(ValueError):
        pipeline.four_point_transform(src.astype(np.float32), SMALL)


# ---------------------------------------------------------------------------------------------------- the engine
# The setup of tests/test_gpu_engine.py: random weights, the rendered-kernel prob_hook, DET_SIZE 320, SVTRv2 tiny.
DET_SIZE = 320
SIZES = [(1000, 760), (900, 700), (760, 1000), (800, 600), (980, 740)]
SEEDS = [11, 12, 13, 14, 15]
QUADS = [[(31.5, 22.25), (735.0, 40.5), (722.75, 978.0), (18.0, 960.5)],
         [(690.25, 872.5), (24.0, 30.5), (12.5, 884.0), (668.5, 18.0)],            # corners in no particular order
         None, None,
         [(40.25, 35.0), (700.5, 52.75), (712.0, 940.25), (28.75, 955.5)]]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


class _Set:
    """The pages, their quads, and per page the rendered text kernels at the detector shape of the RECTIFIED page: each line box of the
    synthetic invoice goes through the quad's forward matrix, and the bounding rectangle of its image is drawn."""

    def __init__(self):
        from ocr_vi_invoice_amd import pipeline, synth
        from ocr_vi_invoice_amd.engine import plan_rectified
        self.pages, self.kern = [], []
        self.rect_sizes, _, shapes, scales, self.buckets = plan_rectified(SIZES, QUADS, DET_SIZE)
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
def data():
    return _Set()


_MODELS = {}


def _models(dtype):
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, weights
    if dtype not in _MODELS:
        _MODELS[dtype] = (DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype=dtype),
                          SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype=dtype))
    return _MODELS[dtype]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        for a, b in zip(gb, wb):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
        assert gs == ws, i
        assert gt == wt, i


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_engine_with_quads_equals_the_per_page_call_and_pre_rectified_pages(data, dtype):
    from ocr_vi_invoice_amd import Engine, pipeline
    det, rec = _models(dtype)
    assert data.buckets == {(320, 256): [0, 1, 3], (256, 320): [2], (320, 224): [4]}      # two rectified pages and a plain one share a bucket
    wrap = _BlendedDet(det, data)
    want = []
    for i, (p, q) in enumerate(zip(data.pages, QUADS)):
        wrap.page = i
        want.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64, quad=q))
    assert sum(len(w[0]) for w in want) > 15 and all(len(w[0]) > 0 for w in want)
    rectified = [p if q is None else pipeline.four_point_transform(p, q) for p, q in zip(data.pages, QUADS)]
    assert [r.shape[:2] for r in rectified] == data.rect_sizes
    pages = list(data.pages)
    pages[1] = torch.from_numpy(pages[1]).cuda()                 # one of the quad pages is a device tensor
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), rec_batch=16, prob_hook=data.hook)
    # det_chunk 4: pages 0, 1 (quads; one from the host, one on the device) and 3 (none) in one chunk; det_chunk 2: 0, 1 | 3
    for graphs, det_chunk in ((True, 4), (False, 2)):
        eng = Engine(det, rec, _pp(), graphs=graphs, det_chunk=det_chunk, **kw)
        got = eng.run(pages, QUADS)
        _assert_same(got, want)
        assert eng.stats["rectified"] == 3 and eng.stats["buckets"] == {"320x256": 3, "256x320": 1, "320x224": 1}
        _assert_same(eng.run(rectified), want)
        assert eng.stats["rectified"] == 0
        _assert_same(eng.run(pages, QUADS), want)                # again: cached graphs, buffers of the right size already there
        _assert_same(eng.run(rectified, [None] * 5), want)


def test_engine_validates_quads_before_any_gpu_work(data):
    from ocr_vi_invoice_amd import Engine
    det, rec = _models("f16x2")
    eng = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=2, rec_batch=16, prob_hook=data.hook)
    for bad in ([(10, 0), (20, 10), (10, 20), (0, 10)], [(0, 0), (1, 1)], [(0, 0), (50, 0), (50, float("nan")), (0, 40)]):
        with pytest.raises(ValueError, match="page 1"):
            eng.run(data.pages[:2], [QUADS[0], bad])
    with pytest.raises(ValueError, match="quads"):
        eng.run(data.pages[:2], [QUADS[0]])
    assert eng.run([], []) == []
