"""The encoder's arithmetic and host entries without a GPU: tests/jpegenc_ref.py against the bytes PIL (libjpeg-turbo) wrote
(tests/golden/jpeg_encode_cases.npz, byte for byte, every case), and the library's host entries -- quantisation tables, header, sizes,
table entry -- against the reference.  Reads the archive only (no PIL)."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegenc_ref  # noqa: E402
from jpegenc_cases import KIND, MODE, NAMES, PAGE, QUALITY, SUB, Z, image, ref  # noqa: E402


def test_the_archive_holds_the_cases_the_header_lists():
    for size in ("1x1", "8x8", "16x16", "17x23", "33x50", "31x18", "40x57"):
        for mode in ("420", "444", "grey"):
            assert f"s{size}_{mode}_q85" in NAMES
    for q in (1, 30, 100):
        for mode in ("420", "444", "grey"):
            assert f"s33x50_{mode}_q{q}" in NAMES
    for n in ("noise_48x64_420_q100", "checker_32x32_420_q60", "checker_32x32_420_q10", "blocks_32x32_grey_q100", "flat_24x40_420_q85", "noise_200x328_420_q100", PAGE):
        assert n in NAMES


@pytest.mark.parametrize("name", [n for n in NAMES if KIND[n] == "pil"])
def test_reference_equals_pil_byte_for_byte(name):
    assert ref(name).data == Z["j_" + name].tobytes()


def test_reference_equals_pil_on_the_page():
    assert hashlib.sha256(ref(PAGE).data).digest() == Z["h_" + PAGE].tobytes()


def test_the_cases_reach_the_rules_they_are_there_for():
    assert ref("s17x23_420_q85").dummy.sum() > 0 and ref("s33x50_420_q85").dummy.sum() > ref("s17x23_420_q85").dummy.sum()
    assert ref("noise_48x64_420_q100").scan.count(b"\xff\x00") >= 10
    for n in ("checker_32x32_grey_q10", "checker_32x32_420_q10"):      # a run above 15 before a non-zero coefficient: ZRL
        runs = [np.diff(np.flatnonzero(np.concatenate([[1], b[1:]]))).max(initial=0) for b in ref(n).coef]
        assert max(runs) > 16, n
    e = ref("blocks_32x32_grey_q100")                                  # DC category 11
    assert np.abs(np.diff(e.coef[:, 0])).max() >= 1024
    e = ref("flat_24x40_grey_q85")                                     # EOB only
    assert not e.coef[:, 1:].any()
    assert len(ref("noise_200x328_420_q100").bits) > 1024 and len(ref(PAGE).bits) > 1024        # more blocks than one chunk of a per-page loop


def test_exports_and_abi_version():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    for n in ("ocrvi_jpeg_quant_tables", "ocrvi_jpeg_encode_header", "ocrvi_jpeg_encode_sizes", "ocrvi_jpeg_encode_table_entry", "ocrvi_jpeg_encode_pages"):
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.ocrvi_abi_version() == 5 == _lib.ABI_VERSION


@pytest.mark.parametrize("q", [1, 2, 25, 49, 50, 51, 75, 95, 99, 100])
def test_quant_tables_equal_the_reference(q):
    from ocr_vi_invoice_amd import pipeline
    luma, chroma = pipeline.jpeg_quant_tables(q)
    rl, rc = jpegenc_ref.quant_tables(q)
    assert np.array_equal(luma, rl) and np.array_equal(chroma, rc)


@pytest.mark.parametrize("q", [1, 50, 95, 100])
@pytest.mark.parametrize("nc,sub", [(3, "4:2:0"), (3, "4:4:4"), (1, "4:2:0")])
def test_header_equals_the_reference(q, nc, sub):
    from ocr_vi_invoice_amd import _lib, pipeline
    for h, w in ((1, 1), (33, 50), (65500, 300)):
        got = pipeline.jpeg_encode_header(h, w, nc, sub, q)
        assert got == jpegenc_ref.header(h, w, nc, sub, q)
        assert len(got) <= _lib.JPEG_HEADER_MAX


def test_header_equals_the_golden_files():
    from ocr_vi_invoice_amd import pipeline
    for n in NAMES:
        if KIND[n] != "pil":
            continue
        img = Z["i_" + n]
        head = pipeline.jpeg_encode_header(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, SUB[MODE[n]], QUALITY[n])
        assert Z["j_" + n].tobytes().startswith(head), n


def test_capacity_and_workspace():
    """scan_capacity = 2 x 208 x blocks + 16 (include/ocrvi.h: 1660 bits a block, doubled by stuffing): at least every reference scan,
    and at least twice the unstuffed bytes on the quality-100 noise cases -- the margin stuffing can take."""
    from ocr_vi_invoice_amd import pipeline
    for n in NAMES:
        e = ref(n)
        img = image(n)
        s = pipeline.jpeg_encode_sizes(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, SUB[MODE[n]])
        assert s["blocks"] == len(e.bits), n
        assert s["scan_capacity"] == 2 * 208 * s["blocks"] + 16
        assert s["scan_capacity"] >= len(e.scan), n
        assert int(e.bits.max()) <= 1660, n
        assert s["workspace_bytes"] % 256 == 0 and s["workspace_bytes"] >= s["offsets"][7] + 16
        assert s["offsets"][5] - s["offsets"][4] >= 8 * (s["blocks"] + 1)
        assert s["offsets"][6] - s["offsets"][5] >= 208 * s["blocks"] + 16 >= len(e.unstuffed) + 16
    for n in ("noise_48x64_420_q100", "noise_200x328_420_q100"):
        img = image(n)
        s = pipeline.jpeg_encode_sizes(img.shape[0], img.shape[1], 3, "4:2:0")
        assert s["scan_capacity"] >= 2 * len(ref(n).unstuffed) + 16
        assert len(ref(n).scan) > len(ref(n).unstuffed)


def test_table_entry_fields_and_refusals():
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    entry = np.full(_lib.JPEG_ENC_ENTRY, -1, np.int64)
    cap = pipeline.jpeg_encode_sizes(33, 50, 3, "4:2:0")["scan_capacity"]
    _lib.check(lib.ocrvi_jpeg_encode_table_entry(50, 33, 3, 2, 30, -4096, 150, 512, cap, 256, entry.ctypes.data))
    assert list(entry[:10]) == [-4096, 150, 50, 33, 3, 2, 512, cap, 256, 30] and not entry[10:16].any() and not entry[48:].any()
    rl, rc = jpegenc_ref.quant_tables(30)
    assert np.array_equal(entry[16:48].view(np.uint16).reshape(2, 64), np.stack([rl, rc]))
    for args in ((0, 33, 3, 2, 30, 0, 150, 0, cap, 0), (50, 65501, 3, 2, 30, 0, 150, 0, cap, 0), (50, 33, 2, 2, 30, 0, 150, 0, cap, 0),
                 (50, 33, 3, 3, 30, 0, 150, 0, cap, 0), (50, 33, 3, 2, 0, 0, 150, 0, cap, 0), (50, 33, 3, 2, 101, 0, 150, 0, cap, 0),
                 (50, 33, 3, 2, 30, 0, 149, 0, cap, 0), (50, 33, 3, 2, 30, 0, 150, 0, cap - 1, 0), (50, 33, 3, 2, 30, 0, 150, 0, cap, 8)):
        assert lib.ocrvi_jpeg_encode_table_entry(*args, entry.ctypes.data) == -1, args
    used = C.c_size_t()
    buf = np.zeros(64, np.uint8)
    assert lib.ocrvi_jpeg_encode_header(50, 33, 3, 2, 30, buf.ctypes.data, buf.size, C.byref(used)) == -3      # OCRVI_ENOMEM


def test_job_refuses_before_the_device_is_touched():
    """Every refusal is a ValueError raised by the constructor, which has no device code in it (this test runs without a GPU)."""
    from ocr_vi_invoice_amd import pipeline
    ok = np.zeros((8, 8, 3), np.uint8)
    bad = [dict(images=[np.zeros((8, 8, 3), np.float32)]), dict(images=[np.zeros((8, 8, 4), np.uint8)]), dict(images=[np.zeros((8,), np.uint8)]),
           dict(images=[np.zeros((0, 8, 3), np.uint8)]), dict(images=[np.zeros((8, 65501), np.uint8)]), dict(images=[[1, 2, 3]]),
           dict(images=[ok], subsampling="4:2:2"), dict(images=[ok], quality=0), dict(images=[ok], quality=101), dict(images=[ok], quality=50.0),
           dict(images=[ok, ok], quality=[50])]
    for kw in bad:
        with pytest.raises(ValueError):
            pipeline.JpegEncodeJob(**kw)
    job = pipeline.JpegEncodeJob([ok, np.zeros((5, 9), np.uint8)], quality=[10, 90], subsampling="4:4:4")
    assert job.geom == [(8, 8, 3, 1), (5, 9, 1, 1)]
