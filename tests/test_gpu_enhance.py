"""enhance_document on the device (src/preprocess/scanner.py:55-76): every stage entry and ``ocrvi_enhance_u8`` bit for bit against the
numpy statement of the same arithmetic (tests/enhance_ref.py), destinations inside sentinel bytes at an aligned and at an odd address,
then ``pipeline.enhance_document``, ``detect_and_recognize(enhance=True)`` and ``Engine.run(pages, quads, enhance)``."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enhance_ref as ER  # noqa: E402
import warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
PAD = 64
SHAPES = [(16, 16), (37, 53), (150, 203)]


_INIT = []


def _L():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    _lib.check(lib.ocrvi_enhance_init(0))
    _INIT.append(0)
    return _lib, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, src, shift=0, want_rc=0):
    """Entry ``name`` on the page ``src`` (numpy [h,w,3]).  Source and destination lie ``PAD + shift`` bytes inside buffers of sentinel
    bytes (shift 1: odd addresses, the byte paths); every byte around the destination must come back untouched."""
    L, lib = _L()
    h, w = src.shape[:2]
    nb = h * w * 3
    off = PAD + shift
    sbuf = torch.full((nb + 2 * PAD + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    sbuf[off:off + nb] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).cuda()
    dbuf = torch.full((nb + 2 * PAD + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    args = [0, sbuf.data_ptr() + off, h, w, dbuf.data_ptr() + off]
    if name in ("ocrvi_clahe_lab_u8", "ocrvi_enhance_u8"):
        n = ctypes.c_size_t(L.CLAHE_WORKSPACE_BYTES)
        if name == "ocrvi_enhance_u8":
            L.check(lib.ocrvi_enhance_workspace_bytes(h, w, ctypes.byref(n)))
        ws = torch.empty(n.value + 1, dtype=torch.uint8, device="cuda")
        args += [ws.data_ptr() + shift, n.value]
    rc = getattr(lib, name)(*args, _stream())
    assert rc == want_rc, (name, rc, L.last_error())
    out = dbuf.cpu().numpy()
    assert (out[:off] == SENTINEL).all() and (out[off + nb:] == SENTINEL).all(), name
    assert (sbuf.cpu().numpy()[off:off + nb] == np.ascontiguousarray(src).reshape(-1)).all()
    return out[off:off + nb].reshape(h, w, 3)


def _check(name, src, want):
    for shift in (0, 1):
        got = _call(name, src, shift)
        bad = int((got != want).sum())
        assert bad == 0, (name, src.shape, shift, bad, np.argwhere(got != want)[:4].tolist())


def _rand(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _lattice():
    lv = np.arange(0, 256, 3)
    assert lv.size == 86 and lv[-1] == 255
    return np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(86 * 86, 86, 3).astype(np.uint8)


def test_entries_refuse_a_device_without_init():
    """First in the file, and no earlier file of the suite enhances anything: device 0 has no tables yet."""
    from ocr_vi_invoice_amd import _lib, pipeline
    if _INIT or pipeline._ENHANCE_READY:
        return                              # (run out of order: test_bad_arguments covers a second device where there is one)
    lib = _lib.load()
    src = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((16 * 16 * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    for name in ("ocrvi_rgb_to_lab_u8", "ocrvi_lab_to_rgb_u8", "ocrvi_nlm_lab_u8", "ocrvi_sharpen_u8"):
        assert getattr(lib, name)(0, src.data_ptr(), 16, 16, dst.data_ptr(), _stream()) == -1 and "ocrvi_enhance_init" in _lib.last_error()
    for name in ("ocrvi_clahe_lab_u8", "ocrvi_enhance_u8"):
        assert getattr(lib, name)(0, src.data_ptr(), 16, 16, dst.data_ptr(), src.data_ptr(), 1 << 20, _stream()) == -1
        assert "ocrvi_enhance_init" in _lib.last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- colour
def test_rgb_to_lab_on_the_lattice_and_on_random_pixels():
    lat = _lattice()
    want = ER.rgb_to_lab(lat)
    assert want[..., 0].min() == 0 and want[..., 0].max() == 255 and want[..., 1].min() < 60 and want[..., 2].max() > 200
    _check("ocrvi_rgb_to_lab_u8", lat, want)
    rnd = _rand(1, 37, 53)
    _check("ocrvi_rgb_to_lab_u8", rnd, ER.rgb_to_lab(rnd))


def test_lab_to_rgb_on_the_lattice_and_on_random_triples():
    lab = ER.rgb_to_lab(_lattice())
    _check("ocrvi_lab_to_rgb_u8", lab, ER.lab_to_rgb(lab))
    rnd = _rand(2, 37, 53)                      # random Lab triples: most lie outside the RGB gamut
    want = ER.lab_to_rgb(rnd)
    assert (want == 0).mean() > 0.05 and (want == 255).mean() > 0.05
    _check("ocrvi_lab_to_rgb_u8", rnd, want)
    rnd = _rand(3, 203, 150)
    _check("ocrvi_lab_to_rgb_u8", rnd, ER.lab_to_rgb(rnd))


# ---------------------------------------------------------------------------------------------------- CLAHE
def _clahe_inputs(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    ab = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    two = np.where((np.add.outer(np.arange(h) // 3, np.arange(w) // 5) % 2) == 0, 40, 210)
    ramp = (np.add.outer(np.arange(h) * 2, np.arange(w) * 3) * 255 // max(2 * (h - 1) + 3 * (w - 1), 1))
    planes = {"random": rng.integers(0, 256, (h, w)), "constant": np.full((h, w), 100), "two_level": two, "ramp": ramp}
    return {k: np.concatenate([p.astype(np.uint8)[..., None], ab], -1) for k, p in planes.items()}


@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (64, 96), (203, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_clahe_is_bit_equal_to_the_reference(hw):
    for kind, lab in _clahe_inputs(*hw).items():
        want = ER.clahe_lab(lab)
        assert np.array_equal(want[..., 1:], lab[..., 1:])
        if kind != "constant":
            assert (want[..., 0] != lab[..., 0]).any(), kind
        _check("ocrvi_clahe_lab_u8", lab, want)


# ---------------------------------------------------------------------------------------------------- NLM
_NLM_REF = {}


def _noisy_invoice_lab():
    from ocr_vi_invoice_amd import synth
    img = synth.make_invoice(5, 150, 203, lines=4)[0]
    noise = np.random.default_rng(0).normal(0, 6, img.shape)
    return ER.rgb_to_lab(np.clip(img + noise, 0, 255).round().astype(np.uint8))


def _nlm_case(kind, hw):
    """(input Lab page, reference output), computed once."""
    if (kind, hw) not in _NLM_REF:
        h, w = hw
        if kind == "invoice":
            lab = np.ascontiguousarray(_noisy_invoice_lab()[:h, 203 - w:])      # the top right corner holds text at every size
        elif kind == "constant":
            lab = np.full((h, w, 3), 255, np.uint8)
        else:
            lab = _rand(7, h, w)
        st = {}
        _NLM_REF[(kind, hw)] = (lab, ER.nlm_lab(lab, st), st)
    return _NLM_REF[(kind, hw)]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["invoice", "constant", "random"])
def test_nlm_is_bit_equal_to_the_reference(kind, hw):
    lab, want, st = _nlm_case(kind, hw)
    if kind == "invoice":       # the comparison is not one of identities: most offsets carry weight and most pixels change
        assert st["L"] >= 220 and st["ab"] >= 220 and min((want[..., c] != lab[..., c]).mean() for c in range(3)) > 0.5
    elif kind == "constant":    # every one of the 441 weights is 255: the largest sums
        assert st["L"] == 440 and st["ab"] == 440 and np.array_equal(want, lab)
    else:
        assert np.array_equal(want, lab) and st["L"] == 0
    _check("ocrvi_nlm_lab_u8", lab, want)


# ---------------------------------------------------------------------------------------------------- sharpen
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sharpen_is_bit_equal_to_the_reference(hw):
    h, w = hw
    rnd = _rand(9, h, w)
    want = ER.sharpen(rnd)
    assert (want == 0).mean() > 0.1 and (want == 255).mean() > 0.1            # saturates at both ends
    _check("ocrvi_sharpen_u8", rnd, want)
    soft = (100 + _rand(10, h, w) % 7).astype(np.uint8)                        # and a page on which nothing saturates
    want = ER.sharpen(soft)
    assert 0 < want.min() and want.max() < 255
    _check("ocrvi_sharpen_u8", soft, want)


# ---------------------------------------------------------------------------------------------------- the whole stage
_ENH_REF = {}


def _page(hw, seed=5):
    from ocr_vi_invoice_amd import synth
    h, w = hw
    img = synth.make_invoice(seed, h, w, lines=4)[0] if h >= 100 else synth.make_invoice(seed, 150, 203, lines=4)[0][:h, 203 - w:]
    noise = np.random.default_rng(seed).normal(0, 6, img.shape)
    return np.ascontiguousarray(np.clip(img + noise, 0, 255).round().astype(np.uint8))


def _enhanced(hw, seed=5):
    if (hw, seed) not in _ENH_REF:
        p = _page(hw, seed)
        _ENH_REF[(hw, seed)] = (p, ER.enhance(p))
    return _ENH_REF[(hw, seed)]


@pytest.mark.parametrize("hw", [(37, 53), (150, 203)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_enhance_equals_the_composition_of_the_stage_references(hw):
    page, want = _enhanced(hw)
    assert (want != page).mean() > 0.5
    _check("ocrvi_enhance_u8", page, want)
    # and the stage entries chained on the device give the same bytes
    x = page
    for name in ("ocrvi_rgb_to_lab_u8", "ocrvi_clahe_lab_u8", "ocrvi_lab_to_rgb_u8", "ocrvi_rgb_to_lab_u8", "ocrvi_nlm_lab_u8",
                 "ocrvi_lab_to_rgb_u8", "ocrvi_sharpen_u8"):
        x = _call(name, x)
    assert np.array_equal(x, want)


def test_enhance_graph_replays_on_new_input_in_the_same_buffers():
    L, lib = _L()
    hw = (150, 203)
    (p1, w1), (p2, w2) = _enhanced(hw), _enhanced(hw, seed=6)
    assert not np.array_equal(w1, w2)
    n = ctypes.c_size_t()
    L.check(lib.ocrvi_enhance_workspace_bytes(hw[0], hw[1], ctypes.byref(n)))
    src, dst = torch.from_numpy(p1).cuda(), torch.zeros(hw + (3,), dtype=torch.uint8, device="cuda")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.ocrvi_enhance_u8(0, src.data_ptr(), hw[0], hw[1], dst.data_ptr(), ws.data_ptr(), n.value, _stream()))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), w1)
    src.copy_(torch.from_numpy(p2))
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), w2)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), w2)


def test_bad_arguments_return_their_codes_and_touch_nothing():
    L, lib = _L()
    h, w = 16, 20
    nb = h * w * 3
    src = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * nb,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    s, d, k, st = src.data_ptr(), dst.data_ptr(), ws.data_ptr(), _stream()
    plain = ("ocrvi_rgb_to_lab_u8", "ocrvi_lab_to_rgb_u8", "ocrvi_nlm_lab_u8", "ocrvi_sharpen_u8")
    for name in plain + ("ocrvi_clahe_lab_u8", "ocrvi_enhance_u8"):
        fn = getattr(lib, name)
        tail = (st,) if name in plain else (k, 1 << 16, st)
        for args in ((None, h, w, d), (s, h, w, None), (s, 15, w, d), (s, h, 15, d), (s, h, -1, d),
                     (d, h, w, d), (d, h, w, d + nb - 1), (d + 1, h, w, d)):               # the last three: dst overlaps src
            assert fn(0, *args, *tail) == -1 and L.last_error(), (name, args)
        assert fn(1000, s, h, w, d, *tail) == -1                                           # no such device
        if torch.cuda.device_count() > 1:                                                  # a device without init (the tests use device 0 alone)
            assert fn(1, s, h, w, d, *tail) == -1 and "enhance_init" in L.last_error()
    assert lib.ocrvi_clahe_lab_u8(0, s, h, w, d, None, 1 << 16, st) == -1
    assert lib.ocrvi_clahe_lab_u8(0, s, h, w, d, k, L.CLAHE_WORKSPACE_BYTES - 1, st) == -3 and L.last_error()
    n = ctypes.c_size_t()
    L.check(lib.ocrvi_enhance_workspace_bytes(h, w, ctypes.byref(n)))
    assert lib.ocrvi_enhance_u8(0, s, h, w, d, None, n.value, st) == -1
    assert lib.ocrvi_enhance_u8(0, s, h, w, d, k, n.value - 1, st) == -3 and L.last_error()
    assert lib.ocrvi_enhance_init(-1) == -1 and lib.ocrvi_enhance_init(0) == 0             # idempotent
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- Python
def test_pipeline_enhance_document_on_numpy_and_on_a_device_tensor():
    from ocr_vi_invoice_amd import pipeline
    page, want = _enhanced((150, 203))
    got = pipeline.enhance_document(page)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    dev = pipeline.enhance_document(torch.from_numpy(page).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    strided = torch.from_numpy(np.concatenate([page, page], 1)).cuda()[:, :203]          # a non-contiguous view
    assert np.array_equal(pipeline.enhance_document(strided).cpu().numpy(), want)
    with pytest.raises(ValueError, match="enhance_document"):
        pipeline.enhance_document(page[:15])
    with pytest.raises(ValueError, match="enhance_document"):
        pipeline.enhance_document(page.astype(np.float32))
    with pytest.raises(NotImplementedError, match="enhance_document"):
        pipeline.preprocess_image(page, None, enhance=True)


# ---------------------------------------------------------------------------------------------------- detect_and_recognize and the engine
# The setup of tests/test_gpu_rectify.py: random weights, the rendered-kernel prob_hook, DET_SIZE 320, SVTRv2 tiny.
DET_SIZE = 320
SIZES = [(1000, 760), (900, 700), (760, 1000), (800, 600)]
SEEDS = [11, 12, 13, 14]
QUADS = [[(31.5, 22.25), (735.0, 40.5), (722.75, 978.0), (18.0, 960.5)], None, None, None]
ENHANCE = [True, True, False, False]


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


def _per_page(data, det, rec, enhance):
    from ocr_vi_invoice_amd import pipeline
    wrap = _BlendedDet(det, data)
    out = []
    for i, (p, q, e) in enumerate(zip(data.pages, QUADS, enhance)):
        wrap.page = i
        out.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64, quad=q,
                                                 enhance=e))
    return out


def test_detect_and_recognize_with_enhance_equals_the_call_on_the_enhanced_page(data):
    from ocr_vi_invoice_amd import pipeline
    det, rec = _models("f16x2")
    wrap = _BlendedDet(det, data)
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64)
    for i in (0, 1):                       # with and without a quad
        wrap.page = i
        got = pipeline.detect_and_recognize(data.pages[i], wrap, rec, _pp(), "cuda:0", quad=QUADS[i], enhance=True, **kw)
        pre = pipeline.enhance_document(pipeline.preprocess_image(data.pages[i], QUADS[i]))
        assert pre.shape[:2] == tuple(data.rect_sizes[i]) and (pre != pipeline.preprocess_image(data.pages[i], QUADS[i])).mean() > 0.2
        _assert_same([got], [pipeline.detect_and_recognize(pre, wrap, rec, _pp(), "cuda:0", **kw)])
        assert len(got[0]) > 0


def test_engine_with_mixed_enhance_equals_the_per_page_call(data):
    from ocr_vi_invoice_amd import Engine
    det, rec = _models("f16x2")
    want = _per_page(data, det, rec, ENHANCE)
    plain = _per_page(data, det, rec, [False] * 4)
    assert all(len(w[0]) > 0 for w in want)
    assert any(w[2] != p[2] for w, p in zip(want[:2], plain[:2]))          # the enhancement does change what is read
    pages = list(data.pages)
    pages[1] = torch.from_numpy(pages[1]).cuda()                 # an enhanced page that is a device tensor: it must not be modified
    keep = pages[1].clone()
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), rec_batch=16, prob_hook=data.hook)
    for graphs, det_chunk in ((True, 4), (False, 2)):
        eng = Engine(det, rec, _pp(), graphs=graphs, det_chunk=det_chunk, **kw)
        _assert_same(eng.run(pages, QUADS, enhance=ENHANCE), want)
        assert eng.stats["enhanced"] == 2 and eng.stats["rectified"] == 1
        _assert_same(eng.run(pages, QUADS), plain)                # a run without enhance afterwards: the plain result
        assert eng.stats["enhanced"] == 0
        _assert_same(eng.run(pages, QUADS, enhance=np.asarray(ENHANCE)), want)
        all_on = eng.run(pages[:2], QUADS[:2], enhance=True)
        _assert_same(all_on, want[:2])
        assert eng.stats["enhanced"] == 2
        _assert_same(eng.run(pages, QUADS, enhance=False), plain)
    assert torch.equal(pages[1], keep)
    with pytest.raises(ValueError, match="enhance"):
        eng.run(pages, QUADS, enhance=[True])
    with pytest.raises(ValueError, match="page 1"):
        eng.run([data.pages[0], np.zeros((12, 40, 3), np.uint8)], None, enhance=[False, True])
