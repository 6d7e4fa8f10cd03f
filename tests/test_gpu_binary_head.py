"""GPU: DBNetPP.forward_binary / ocrvi_det_forward_binary -- the detector forward that computes the binarise branch of the DB head alone
(head.py:34; the page loop reads preds['binary'] and nothing else, pipeline2.py:318) -- against the five-map forward it is a part of.

The binarise columns see the same packed weight bits (the two head layers are launched on views of the two-branch pack), the same K order
and the same epilogue arithmetic as in the five-map forward, so in the f32 and f16x2 modes the map is expected to be the same BITS, on
every shape and on whichever kernel the dispatcher picks."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [(2, 64, 96), (2, 96, 64)]                       # the shapes of tests/test_gpu_models.py
# 512 x 512 x 2 = 32 768 quarter-resolution pixels: past the 16 384-row threshold tests/conftest.py sets for the ring's 3x3 mode
MID = [(1, 32, 32), (2, 512, 512)]
FULL = [(2, 960, 1280), (2, 736, 960)]                   # whole 16 x 16 quarter-resolution tiles / 184 rows: a partial tile row
THRESH_FLOPS_PER_PIXEL = 2 * (64 * 2304 + 256 * 64)      # the threshold branch per quarter-resolution pixel: 3x3 conv + deconv1

_MODELS = {}


def _model(dt, seed=21):
    from ocr_vi_invoice_amd import DBNetPP, weights
    if (dt, seed) not in _MODELS:
        _MODELS[(dt, seed)] = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=seed), dtype=dt)
    return _MODELS[(dt, seed)]


def _pages(N, H, W, first_seed=1):
    from ocr_vi_invoice_amd import synth
    lines = 3 if H * W <= 96 * 96 else 20
    return torch.from_numpy(np.stack([synth.normalize_chw(synth.make_invoice(first_seed + i, H, W, lines=lines)[0]) for i in range(N)]))


def _same_bits(dt, shape):
    N, H, W = shape
    m = _model(dt)
    x = _pages(N, H, W).cuda()
    want = m(x)["binary"]
    got = m.forward_binary(x)
    torch.cuda.synchronize()
    assert got.shape == (N, 1, H, W) and got.dtype == torch.float32
    diff = float((got - want).abs().max())
    print(f"\n[{dt} {N}x{H}x{W}] forward_binary vs forward['binary']: max |diff| {diff:.3e}, differing elements {int((got != want).sum())}")
    assert torch.equal(got, want), (dt, shape, diff)


# ---------------------------------------------------------------------------------------------------------------- 1. same bits
@pytest.mark.parametrize("shape", SMALL + MID)
@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_forward_binary_has_the_bits_of_the_five_map_forward(dt, shape):
    _same_bits(dt, shape)


@pytest.mark.parametrize("shape", FULL)
def test_forward_binary_has_the_same_bits_at_full_size_f16x2(shape):
    _same_bits("f16x2", shape)


# ---------------------------------------------------------------------------------------------------------------- 2. f16 / bf16
@pytest.mark.parametrize("shape", SMALL + MID)
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_forward_binary_has_the_same_bits_in_the_16_bit_modes(dt, shape):
    """Equality holds in f16 / bf16 as well, although at 2 x 512 x 512 the dispatcher picks two kernel families for the head convolution: the
    128-column layer of the five-map forward runs on the ring GEMM's 3x3 mode (`ring_conv3x3_128x128`, 256-row tiles, chosen from 16 384 rows
    up under tests/conftest.py), the 64-column layer of forward_binary on `conv_gemm`'s 128 x 64 tile (`conv3x3_128x64`; the ring's 3x3 mode
    takes 128-column layers only).  Both accumulate a column over K in the order (tap, channel) and the maps come out with the same bits on every
    shape here (0 differing elements measured); the oracle budget of the 16-bit modes is held as well, in the test below."""
    _same_bits(dt, shape)


@pytest.mark.parametrize("dt,tol", [("bf16", 0.033), ("f16", 0.0053)])
def test_forward_binary_lowp_error_budget(dt, tol):
    """The budget tests/test_gpu_models.py::test_dbnet_lowp_error_budget holds forward to, on its input and seed."""
    from ocr_vi_invoice_amd import synth, weights
    from oracle import dbnet_cpu
    sd = weights.make_det_state_dict(seed=21)
    x = torch.from_numpy(synth.normalize_chw(synth.make_invoice(1, 64, 96, lines=3)[0]))[None]
    ref = dbnet_cpu.forward(sd, x)
    out = _model(dt).forward_binary(x.cuda())
    err = float((out.cpu() - ref["binary"]).abs().max())
    print(f"\n[{dt}] forward_binary max-abs-err vs the oracle {err:.4f}")
    assert err < tol


# ---------------------------------------------------------------------------------------------------------------- 3. oracle
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_forward_binary_matches_the_oracle(dt, shape):
    from ocr_vi_invoice_amd import weights
    from oracle import dbnet_cpu
    N, H, W = shape
    x = _pages(N, H, W)
    ref = dbnet_cpu.forward(weights.make_det_state_dict(seed=21), x)["binary"]
    got = _model(dt).forward_binary(x.cuda()).cpu()
    err = float((got - ref).abs().max())
    print(f"\n[{dt} {N}x{H}x{W}] forward_binary vs oracle max-abs-err {err:.3e}")
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=1e-3)          # north_star: 1e-3


# ---------------------------------------------------------------------------------------------------------------- 4. the work is gone
def _profiled(fn):
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.ocrvi_prof_reset()
    lib.ocrvi_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.ocrvi_prof_enable(0)
    rep = _lib.prof_report()
    lib.ocrvi_prof_reset()
    return rep


@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_threshold_branch_is_not_computed(dt):
    N, H, W = 2, 96, 64
    m = _model(dt)
    x = _pages(N, H, W).cuda()
    m(x), m.forward_binary(x)                            # workspaces allocated outside the profiled calls
    full = _profiled(lambda: m(x))
    part = _profiled(lambda: m.forward_binary(x))
    want = N * (H // 4) * (W // 4) * THRESH_FLOPS_PER_PIXEL
    got = sum(v["flops"] for v in full.values()) - sum(v["flops"] for v in part.values())
    print(f"\n[{dt}] profiler FLOPs: five-map {sum(v['flops'] for v in full.values()):.6e}, binary {sum(v['flops'] for v in part.values()):.6e}, "
          f"difference {got:.6e} (threshold branch {want:.6e})")
    assert abs(got - want) <= 1e-4 * want, (got, want)

    def launches(rep, prefix):
        return sum(v["launches"] for k, v in rep.items() if k.startswith(prefix))
    assert launches(full, "db_maps") == 1 and launches(part, "db_maps") == 0
    assert launches(part, "deconv2x2_dbbin") == 1 and launches(full, "deconv2x2_dbbin") == 0
    assert launches(full, "deconv2x2_dbtail") == 1 and launches(part, "deconv2x2_dbtail") == 0


# ---------------------------------------------------------------------------------------------------------------- 5. workspace
def _ws_bytes(m, fn, N, H, W):
    from ocr_vi_invoice_amd import _lib
    n = C.c_size_t()
    _lib.check(getattr(_lib.load(), fn)(m._handle, N, H, W, C.byref(n)))
    return n.value


@pytest.mark.parametrize("dt", ["f32", "f16x2", "f16", "bf16"])
def test_binary_workspace_is_never_larger(dt):
    m = _model(dt)
    for N, H, W in SMALL + MID + FULL + [(16, 960, 1280)]:
        b, f = _ws_bytes(m, "ocrvi_det_binary_workspace_bytes", N, H, W), _ws_bytes(m, "ocrvi_det_workspace_bytes", N, H, W)
        print(f"\n[{dt} {N}x{H}x{W}] workspace: binary {b} B, five-map {f} B")
        assert 0 < b <= f, (dt, N, H, W, b, f)


def test_forward_binary_argument_errors():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    m = _model("f16x2")
    N, H, W = 2, 64, 96
    need = _ws_bytes(m, "ocrvi_det_binary_workspace_bytes", N, H, W)
    x = _pages(N, H, W).cuda()
    out = torch.empty((N, 1, H, W), device="cuda")
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    st = torch.cuda.current_stream().cuda_stream
    assert lib.ocrvi_det_forward_binary(m._handle, x.data_ptr(), N, H, W, out.data_ptr(), base, need - 1, st) == -3          # OCRVI_ENOMEM
    assert lib.ocrvi_det_forward_binary(m._handle, x.data_ptr(), N, H, W, out.data_ptr(), base + 16, need, st) == -1        # OCRVI_EINVAL
    assert lib.ocrvi_det_forward_binary(m._handle, x.data_ptr(), N, H, W, None, base, need, st) == -1
    assert lib.ocrvi_det_forward_binary(m._handle, x.data_ptr(), N, 60, W, out.data_ptr(), base, need, st) == -1            # H % 32
    n = C.c_size_t()
    assert lib.ocrvi_det_binary_workspace_bytes(m._handle, N, H, 100, C.byref(n)) == -1
    with pytest.raises(ValueError):
        m.forward_binary(torch.zeros(1, 3, 64, 100, device="cuda"))
    # exactly the reported size, aligned: runs, and gives the facade's map
    assert lib.ocrvi_det_forward_binary(m._handle, x.data_ptr(), N, H, W, out.data_ptr(), base, need, st) == 0
    assert torch.equal(out, m.forward_binary(x))


# ---------------------------------------------------------------------------------------------------------------- 6. graph capture
def test_forward_binary_is_graph_capturable():
    m = _model("f16x2")
    N, H, W = 2, 96, 64
    xs = _pages(N, H, W, first_seed=1).cuda()
    m.forward_binary(xs)                                  # workspace allocated before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = m.forward_binary(xs)
    torch.cuda.synchronize()
    for seed in (5, 9):
        xn = _pages(N, H, W, first_seed=seed).cuda()
        xs.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = m.forward_binary(xn)
        torch.cuda.synchronize()
        assert torch.equal(got, want), seed
    assert not torch.equal(m.forward_binary(_pages(N, H, W, 5).cuda()), m.forward_binary(_pages(N, H, W, 9).cuda()))


def test_forward_binary_leaves_a_captured_forward_its_workspace():
    """A captured graph of ``forward`` holds its workspace's address: ``forward_binary``, at the same shape and at another, must neither
    free nor replace that buffer (the workspace cache keeps one resident shape per forward kind, each kind's apart)."""
    from ocr_vi_invoice_amd import DBNetPP, weights
    m = DBNetPP("resnet18", dcn=False, state_dict=weights.make_det_state_dict(seed=21, backbone="resnet18", dcn=False), dtype="f32")
    x = _pages(1, 64, 64).cuda()
    m(x)                                                  # warm-up: the workspace is allocated before the capture
    ws = m._workspace(1, 64, 64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = m(x)
    torch.cuda.synchronize()
    m.forward_binary(x)
    m.forward_binary(_pages(1, 64, 96).cuda())
    torch.cuda.synchronize()
    out["binary"].zero_()
    g.replay()
    torch.cuda.synchronize()
    got = out["binary"].clone()
    assert m._workspace(1, 64, 64) is ws
    assert torch.equal(got, m(x)["binary"])


# ---------------------------------------------------------------------------------------------------------------- 7. range flag
def test_forward_binary_reports_an_f16x2_overflow_like_forward():
    from ocr_vi_invoice_amd import DBNetPP, weights
    m = _model("f16x2")
    x = _pages(1, 64, 96).cuda()
    m.reset_range()
    try:
        m.forward_binary(x)
        m.check_range()                                   # a clean input raises nothing
        bad = x.clone()
        bad[0, 1, 20, 30] = 70000.0                       # an input element fp16 cannot carry
        m(bad)
        try:
            m.check_range()
            raised = False
        except OverflowError:
            raised = True
        m.reset_range()
        print(f"\n[range] 70000.0 in the input raises through forward: {raised}")
        if not raised:                                    # the input cast did not catch it: overflow the binarise branch's head conv instead
            sd = {k: v.clone() for k, v in weights.make_det_state_dict(seed=21).items()}
            sd["head.bin_conv.0.bn.weight"] *= 2.0 ** 17
            m = DBNetPP(pretrained=False, state_dict=sd, dtype="f16x2")
            bad = x
            m(bad)
            with pytest.raises(OverflowError):
                m.check_range()
            m.reset_range()
        m.forward_binary(bad)
        with pytest.raises(OverflowError):
            m.check_range()
    finally:
        m.reset_range()                                   # the flag is per device and sticky: do not leak it into later tests
        torch.cuda.synchronize()
    m.forward_binary(x)
    m.check_range()


# ---------------------------------------------------------------------------------------------------------------- 8. engine / pipeline
DET_SIZE = 320
# the mixed page set of tests/test_gpu_engine.py
SIZES = [(1000, 760), (900, 700), (760, 1000), (640, 640), (333, 1001), (1000, 760)]
SEEDS = [11, 12, 13, 14, 15, 11]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)


class _Set:
    def __init__(self):
        from ocr_vi_invoice_amd import synth
        from ocr_vi_invoice_amd.engine import plan_buckets
        self.pages, kern = [], []
        shapes, scales, _ = plan_buckets(SIZES, DET_SIZE)
        for (h, w), seed, (H, W), (sh, sw) in zip(SIZES, SEEDS, shapes, scales):
            img, boxes = synth.make_invoice(seed, h, w, lines=8)
            self.pages.append(img)
            k = np.zeros((1, H, W), np.float32)
            for x, y, bw, bh in boxes:
                x0, x1 = int(x * sw) + 2, int((x + bw) * sw) - 2
                y0, y1 = int(y * sh) + 1, int((y + bh) * sh) - 1
                if x1 - x0 >= 3 and y1 - y0 >= 2:
                    k[0, y0:y1, x0:x1] = 0.75
            kern.append(torch.from_numpy(k).cuda())
        self.kern = kern

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


class _BlendedDet:
    """detect_and_recognize's detector for page `page`: the library detector, its binary map blended exactly as the engine's hook does."""

    def __init__(self, det, data):
        self.det, self.data, self.page = det, data, 0
        self.calls = {"forward": 0, "forward_binary": 0}

    def __call__(self, x):
        self.calls["forward"] += 1
        return {"binary": torch.add(self.data.kern[self.page][None], self.det(x)["binary"], alpha=0.25)}

    def forward_binary(self, x):
        self.calls["forward_binary"] += 1
        return torch.add(self.data.kern[self.page][None], self.det.forward_binary(x), alpha=0.25)


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        for a, b in zip(gb, wb):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
        assert gs == ws, i
        assert gt == wt, i


@pytest.fixture(scope="module")
def data():
    return _Set()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_engine_and_pipeline_with_the_binary_head(data, dtype):
    from ocr_vi_invoice_amd import Engine, SVTRv2, pipeline, weights
    det = _model(dtype)
    rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype=dtype)
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    off = Engine(det, rec, _pp(), **kw)
    assert off.binary_head is False
    want = off.run(data.pages)
    assert sum(len(w[0]) for w in want) > 20 and all(len(w[0]) > 0 for w in want)
    on = Engine(det, rec, _pp(), binary_head=True, **kw)
    assert on.det_ws.numel() <= off.det_ws.numel()
    _assert_same(on.run(data.pages), want)
    _assert_same(on.run(data.pages), want)                                       # second run: the captured graphs replay
    _assert_same(Engine(det, rec, _pp(), binary_head=True, graphs=False, **kw).run(data.pages), want)
    wrap = _BlendedDet(det, data)
    per_page = []
    for i, p in enumerate(data.pages):
        wrap.page = i
        per_page.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64,
                                                      binary_head=True))
    assert wrap.calls == {"forward": 0, "forward_binary": len(data.pages)}
    _assert_same(per_page, want)
    # the one-shot wrapper passes the option on (plain random-weight detector, as tests/test_gpu_engine.py calls it)
    pp = _pp()
    pp.max_candidates = 50
    a = pipeline.detect_and_recognize_pages(data.pages[2:5], det, rec, pp, "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), binary_head=True)
    b = pipeline.detect_and_recognize_pages(data.pages[2:5], det, rec, pp, "cuda:0", det_size=DET_SIZE, rec_size=(32, 256))
    _assert_same(a, b)
