"""ocrvi_png_encode_pages through pipeline.imencode_png / imencode_png_pages / imwrite / save_result against tests/pngenc_ref.py: the
whole file byte for byte on every small case, the stored SHA-256 on the page, and every stage -- filter bytes, filtered stream,
histograms, code lengths, code-length symbols, block types, bit offsets, Adler, CRC -- read from the workspace through the layout
include/ocrvi.h states, so a failure names its stage.  Needs numpy, zlib and the repository only.

The small cases have one to four deflate blocks of 16384 bytes; the page has 226, more than the 128 workgroups that share a page; a
grey 2112 x 2048 page has 265, more than one 256-block chunk of png_scan_kernel."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngenc_ref  # noqa: E402
from pngenc_cases import BIG, NAMES, PAGE, code_histograms, filters, golden, image, ref  # noqa: E402

pytestmark = pytest.mark.gpu

_ONE = {}


def one_by_one():
    """Every small case encoded alone from a host array, once."""
    from ocr_vi_invoice_amd import pipeline
    if not _ONE:
        for n in NAMES:
            _ONE[n] = pipeline.imencode_png(image(n), filters(n))
    return _ONE


def first_difference(a: bytes, b: bytes):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return (len(a), len(b), k)


def rgb(img):
    return img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)


def test_file_equals_the_reference_on_every_case():
    got = one_by_one()
    bad = [(n,) + first_difference(got[n], ref(n).data) for n in NAMES if got[n] != ref(n).data]
    assert not bad, bad            # (case, bytes got, bytes wanted, first differing byte)
    g = golden()
    assert all(hashlib.sha256(got[n]).digest() == g["h_" + n].tobytes() for n in NAMES)


def test_file_equals_the_stored_digest_on_the_page():
    from ocr_vi_invoice_amd import pipeline
    page = image(PAGE)
    data = pipeline.imencode_png(page)
    g = golden()
    assert (len(data), hashlib.sha256(data).hexdigest()) == (int(g["n_" + PAGE]), g["h_" + PAGE].tobytes().hex())
    assert np.array_equal(pipeline.imdecode(data).cpu().numpy(), page)


def test_file_equals_the_stored_digest_on_more_blocks_than_one_scan_chunk():
    """265 blocks: png_scan_kernel carries the bit position and the Adler sums from its first chunk of 256 blocks into the second, whose
    blocks are stored ones."""
    from ocr_vi_invoice_amd import pipeline
    page = image(BIG)
    data = pipeline.imencode_png(page)
    g = golden()
    assert (len(data), hashlib.sha256(data).hexdigest()) == (int(g["n_" + BIG]), g["h_" + BIG].tobytes().hex())
    assert np.array_equal(pipeline.imdecode(data).cpu().numpy(), rgb(page))


@pytest.mark.parametrize("name", ["rgb_7x6", "walk_26x20_adaptive", "walk_26x20_paeth", "tie_5x9", "tie_types_1x40", "run_262", "run_517", "B_plus_1",
                                  "cross_130x127", "noise_64x64", "mix_385x127", "rgb_70x90"])
def test_stages_equal_the_reference(name):
    from ocr_vi_invoice_amd import pipeline
    e = ref(name)
    job = pipeline.PngEncodeJob([image(name)], filters(name)).launch()
    data = job.collect()[0]
    st = job.stage(0)
    nb, h = len(e.blocks), image(name).shape[0]
    assert np.array_equal(st["filters"][:h], e.filters), "the filter of every row"
    assert np.array_equal(st["stream"][:len(e.stream)], e.stream), "the filtered stream"
    hist = st["hist"].view(np.uint32).reshape(nb, 288)
    assert np.array_equal(hist, np.stack([b.hist for b in e.blocks])), "histograms (286: the matches)"
    lens = st["lens"].reshape(nb, 320)
    assert np.array_equal(lens[:, :286], np.stack([b.lens for b in e.blocks])), "literal / length code lengths"
    assert np.array_equal(lens[:, 288:307], np.stack([b.cl_lens for b in e.blocks])), "code-length code lengths"
    assert not lens[:, 286:288].any() and not lens[:, 307:].any()
    tok = st["cl_tokens"].view(np.uint16).reshape(nb, 320)
    rec = st["records"].view(np.uint32).reshape(nb, 8)
    for k, b in enumerate(e.blocks):
        assert [int(v) for v in tok[k, :len(b.cl_tok)]] == [s | (x << 8) for s, x in b.cl_tok] and not tok[k, len(b.cl_tok):].any(), k
        assert [int(v) for v in rec[k]] == [b.hi - b.lo, b.fixed_bits, b.dynamic_bits, b.hlit, b.hclen, len(b.cl_tok), b.type,
                                            b.adler_a | (b.adler_b << 16)], (k, rec[k])
    assert [int(v) for v in st["bit_offsets"].view(np.uint64)[:nb + 1]] == e.bit_offsets, "bit offsets"
    info = [int(v) for v in st["info"].view(np.uint64)[:4]]
    assert info == [len(e.deflate), e.adler, e.crc, len(e.data)], "deflate bytes, Adler-32, CRC-32, file bytes"
    assert e.adler == zlib.adler32(e.stream.tobytes()) and e.crc == zlib.crc32(data[37:-16])
    parts = pngenc_ref.crc32_segments(e.data[37:-16], 37)[1]
    assert [int(v) for v in st["crc_partials"].view(np.uint32)[:len(parts)]] == parts, "raw CRC partials"
    assert data == e.data


def test_code_lengths_equal_the_reference():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    for label, counts, limit in code_histograms():
        d_counts = torch.from_numpy(counts.view(np.int32).copy()).cuda()          # the same 32 bits: torch has no uint32 arithmetic to need
        out = torch.zeros(counts.shape, dtype=torch.uint8, device="cuda")
        _lib.check(lib.ocrvi_test_png_code_lengths(0, d_counts.data_ptr(), counts.shape[0], counts.shape[1], limit, out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
        got = out.cpu().numpy()
        for k, row in enumerate(counts):
            want = pngenc_ref.code_lengths(row, limit)
            assert np.array_equal(got[k], want), (label, k, row.tolist(), got[k].tolist(), want.tolist())
            assert sum(1 << (limit - int(v)) for v in got[k] if v) == 1 << limit and got[k].max() <= limit, (label, k)
    bad = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((1, 1, 15), (1, 289, 15), (1, 19, 4), (0, 19, 7), (1, 19, 16)):
        assert lib.ocrvi_test_png_code_lengths(0, bad.data_ptr(), *args, bad.data_ptr(), None) == -1, args


def test_round_trip_through_the_decoder():
    from ocr_vi_invoice_amd import pipeline
    got = one_by_one()
    out = pipeline.imdecode([got[n] for n in NAMES])
    for n, t in zip(NAMES, out):
        assert np.array_equal(t.cpu().numpy(), rgb(image(n))), n
    x = torch.from_numpy(image("rgb_70x90")).cuda()
    assert torch.equal(pipeline.imdecode(pipeline.imencode_png(x)), x)


def test_pages_of_mixed_sizes_equal_one_by_one_and_repeat():
    from ocr_vi_invoice_amd import pipeline
    names = ["mix_385x127", "rgb_7x6", "g_1x1", "rgb_70x90", "B_plus_1", "walk_26x20_adaptive"]
    assert len({filters(n) for n in names[1:]}) == 1
    got = one_by_one()
    pages = [image(n) for n in names[1:]]
    batch = pipeline.imencode_png_pages(pages)
    assert batch == [got[n] for n in names[1:]]
    assert pipeline.imencode_png_pages(pages) == batch                      # two runs, equal bytes
    assert pipeline.imencode_png_pages([image(names[0]), image("run_517")], "none") == [got[names[0]], got["run_517"]]
    assert pipeline.imencode_png_pages([]) == []


def test_host_and_device_inputs_give_the_same_bytes():
    from ocr_vi_invoice_amd import pipeline
    got = one_by_one()
    for n in ("rgb_70x90", "B_plus_1"):
        img = image(n)
        assert pipeline.imencode_png(torch.from_numpy(img)) == got[n]
        assert pipeline.imencode_png(torch.from_numpy(img).cuda()) == got[n]
        wide = torch.zeros((img.shape[0], img.shape[1] + 5) + img.shape[2:], dtype=torch.uint8, device="cuda")
        wide[:, :img.shape[1]] = torch.from_numpy(img).cuda()
        assert pipeline.imencode_png(wide[:, :img.shape[1]]) == got[n]      # a view that is not contiguous
    mixed = pipeline.imencode_png_pages([torch.from_numpy(image("rgb_70x90")).cuda(), image("rgb_7x6"), torch.from_numpy(image("g_1x1")).cuda()])
    assert mixed == [got["rgb_70x90"], got["rgb_7x6"], got["g_1x1"]]


def test_strided_rows_bad_entries_and_short_regions_are_skipped():
    """The C entry alone: a source with padded rows, and entries the device must skip without touching their output."""
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    n = "rgb_70x90"
    img = image(n)
    h, w = img.shape[:2]
    s = pipeline.png_encode_sizes(h, w, 3)
    cap, wsb = (s["out_capacity"] + 255) // 256 * 256, s["workspace_bytes"]
    stride = 3 * w + 7
    src = torch.zeros(h * stride + 64, dtype=torch.uint8)
    src[:h * stride].view(h, stride)[:, :3 * w] = torch.from_numpy(img).reshape(h, 3 * w)
    src = src.cuda()
    count = 7
    table = np.zeros((count, _lib.PNG_ENC_ENTRY), np.int64)
    for k in range(count):
        _lib.check(lib.ocrvi_png_encode_table_entry(w, h, 3, 5, 0, stride, k * cap, cap, k * wsb, table[k].ctypes.data))
    table[1, 2] = 0                     # width 0
    table[2, 8] = count * wsb           # workspace region outside the workspace
    table[3, 7] = s["out_capacity"] - 1     # output capacity below the bound
    table[4, 5] = 6                     # a filter mode the encoder lacks
    table[5, 4] = 4                     # RGBA
    out = torch.full((count * cap,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.empty(count * wsb, dtype=torch.uint8, device="cuda")
    lengths = torch.full((count,), -7, dtype=torch.int64, device="cuda")
    d_tab = torch.from_numpy(table).cuda()
    _lib.check(lib.ocrvi_png_encode_pages(0, src.data_ptr(), d_tab.data_ptr(), count, out.data_ptr(), lengths.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    want = ref(n).data
    assert lengths.cpu().tolist() == [len(want), 0, 0, 0, 0, 0, len(want)]
    host = out.cpu().numpy().reshape(count, cap)
    assert host[0, :len(want)].tobytes() == want and host[6, :len(want)].tobytes() == want      # the neighbours are intact
    assert (host[0, len(want):] == 0xA5).all() and (host[1:6] == 0xA5).all() and (host[6, len(want):] == 0xA5).all()
    short = torch.empty(wsb - 256, dtype=torch.uint8, device="cuda")                             # a workspace one page does not fit
    _lib.check(lib.ocrvi_png_encode_pages(0, src.data_ptr(), d_tab.data_ptr(), 1, out.data_ptr(), lengths.data_ptr(),
                                          short.data_ptr(), short.numel(), torch.cuda.current_stream().cuda_stream))
    assert lengths.cpu().tolist()[0] == 0
    with pytest.raises(ValueError):
        _lib.check(lib.ocrvi_png_encode_pages(0, src.data_ptr(), None, 1, out.data_ptr(), lengths.data_ptr(), ws.data_ptr(), ws.numel(), None))


def test_imwrite_and_save_result_write_png_and_keep_jpeg(tmp_path):
    from ocr_vi_invoice_amd import pipeline
    img = image("rgb_70x90")
    path = str(tmp_path / "page.png")
    assert pipeline.imwrite(path, img, format="png") is True
    with open(path, "rb") as f:
        assert f.read() == one_by_one()["rgb_70x90"]
    assert np.array_equal(pipeline.imread(path).cpu().numpy(), img)
    assert pipeline.imwrite(path, img, 5, "4:4:4", format="png") is True        # quality and subsampling are ignored
    with open(path, "rb") as f:
        assert f.read() == one_by_one()["rgb_70x90"]
    boxes = [np.array([[10, 10], [60, 10], [60, 40], [10, 40]])]
    drawn = pipeline.draw_boxes_with_text(img, boxes, ["a"])
    res = str(tmp_path / "result.png")
    assert pipeline.save_result(res, img, boxes, ["a"], format="png") is True
    assert torch.equal(pipeline.imread(res), drawn)
    assert pipeline.imwrite(str(tmp_path / "no" / "such" / "dir.png"), img, format="png") is False
    assert pipeline.save_result(str(tmp_path / "no" / "such" / "dir.png"), img, boxes, ["a"], format="png") is False
    # format=None: today's JPEG, whatever the suffix
    jpg = str(tmp_path / "still_jpeg.png")
    assert pipeline.imwrite(jpg, img, 85) is True and pipeline.imwrite(jpg + "2", img, 85, format=None) is True
    with open(jpg, "rb") as f, open(jpg + "2", "rb") as f2:
        data = f.read()
        assert data == f2.read() == pipeline.imencode(img, 85) and data[:2] == b"\xff\xd8"
    assert pipeline.save_result(jpg, img, boxes, ["a"]) is True
    with open(jpg, "rb") as f:
        assert f.read() == pipeline.imencode(drawn, 95)
    for bad in ("jpeg", "PNG", ".png"):
        with pytest.raises(ValueError):
            pipeline.imwrite(jpg, img, format=bad)


def test_refusals_raise_value_error_and_launch_nothing():
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    ok = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    lib.ocrvi_prof_reset()
    lib.ocrvi_prof_enable(1)
    try:
        for args in ((torch.zeros((8, 8, 3), device="cuda"),), (torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda"),),
                     (torch.zeros((0, 8, 3), dtype=torch.uint8, device="cuda"),), (torch.zeros((3, 65501), dtype=torch.uint8),),
                     (ok, "best"), (ok, 3)):
            with pytest.raises(ValueError):
                pipeline.imencode_png(*args)
        torch.cuda.synchronize()
        report = _lib.prof_report()                    # every launch of the library is bracketed while the profiler is on
    finally:
        lib.ocrvi_prof_enable(0)
        lib.ocrvi_prof_reset()
    assert not report, report
