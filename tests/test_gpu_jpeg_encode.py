"""ocrvi_jpeg_encode_pages through pipeline.imencode / imencode_pages / imwrite against tests/golden/jpeg_encode_cases.npz: the bytes PIL
(libjpeg-turbo) wrote, the whole file, on every case; the transform kernel's coefficients and bit counts against tests/jpegenc_ref.py
through the workspace layout include/ocrvi.h states, so a failure names its stage.  Reads the archive only (no PIL).

The two large cases have 1638 (200 x 328) and 2304 (500 x 380) blocks and scans of about 130 KB and 33 KB: more than one trip of the
1024-block chunks of jpeg_bits_kernel, several 32-block groups per workgroup of jpeg_fdct_kernel, and on the noise case 32 stuffing
segments of 4096 bytes, which the 64 workgroups of a page share."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpegenc_cases import KIND, MODE, NAMES, PAGE, QUALITY, SUB, Z, image, ref  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [n for n in NAMES if KIND[n] == "pil"]
_ONE = {}


def one_by_one():
    """Every stored case encoded alone from a host array, once."""
    from ocr_vi_invoice_amd import pipeline
    if not _ONE:
        for n in SMALL:
            _ONE[n] = pipeline.imencode(image(n), QUALITY[n], SUB[MODE[n]])
    return _ONE


def first_difference(a: bytes, b: bytes):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return (len(a), len(b), k)


def test_imencode_equals_pil_on_every_case():
    got = one_by_one()
    bad = [(n,) + first_difference(got[n], Z["j_" + n].tobytes()) for n in SMALL if got[n] != Z["j_" + n].tobytes()]
    assert not bad, bad            # (case, bytes got, bytes wanted, first differing byte)


def test_imencode_equals_pil_on_the_page():
    from ocr_vi_invoice_amd import pipeline
    data = pipeline.imencode(image(PAGE), QUALITY[PAGE], "4:2:0")
    assert hashlib.sha256(data).digest() == Z["h_" + PAGE].tobytes(), first_difference(data, ref(PAGE).data)


@pytest.mark.parametrize("name", ["s17x23_420_q85", "s33x50_420_q100", "noise_48x64_420_q100", "blocks_32x32_grey_q100", "checker_32x32_420_q10",
                                  "noise_200x328_420_q100"])
def test_stages_equal_the_reference(name):
    """Coefficients, DC values, bits per block, bit offsets, the scan before stuffing and its length, read from the workspace."""
    from ocr_vi_invoice_amd import pipeline
    e = ref(name)
    job = pipeline.JpegEncodeJob([image(name)], QUALITY[name], SUB[MODE[name]]).launch()
    scans = job.collect_scans()
    img = image(name)
    s = pipeline.jpeg_encode_sizes(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, SUB[MODE[name]])
    nb, o = s["blocks"], s["offsets"]
    ws = job._ws.cpu().numpy()
    assert nb == len(e.bits)
    coef = ws[o[0]:o[0] + 128 * nb].view(np.int16).reshape(nb, 64).astype(np.int32)
    real = ~e.dummy
    assert np.array_equal(coef[real], e.coef[real]), "coefficients of real blocks"
    assert not coef[e.dummy].any(), "dummy blocks hold no coefficients"
    dc = ws[o[1]:o[1] + 2 * nb].view(np.int16)
    assert np.array_equal(dc[real], e.coef[real, 0]), "DC values"
    pred = np.zeros(nb, np.int64)
    for c in range(3):
        idx = np.flatnonzero(e.comp == c)
        pred[idx[1:]] = e.coef[idx[:-1], 0]
    assert np.array_equal(ws[o[2]:o[2] + 2 * nb].view(np.int16), e.coef[:, 0] - pred), "DC differences (dummy blocks inherit)"
    assert np.array_equal(ws[o[3]:o[3] + 4 * nb].view(np.uint32), e.bits), "bits per block"
    assert np.array_equal(ws[o[4]:o[4] + 8 * (nb + 1)].view(np.uint64), np.concatenate([[0], np.cumsum(e.bits)])), "bit offsets"
    n = int(ws[o[7]:o[7] + 8].view(np.uint64)[0])
    assert n == len(e.unstuffed)
    assert ws[o[5]:o[5] + n].tobytes() == e.unstuffed, "the scan before stuffing"
    assert scans[0] == e.scan


def test_pages_of_mixed_sizes_equal_one_by_one_and_repeat():
    from ocr_vi_invoice_amd import pipeline
    names = ["s33x50_grey_q85", "s17x23_420_q85", "noise_200x328_420_q100", "s1x1_420_q85"]
    quals = [85, 30, 100, 85]
    pages = [image(n) for n in names]
    want = [pipeline.imencode(p, q) for p, q in zip(pages, quals)]
    got = pipeline.imencode_pages(pages, quals)
    assert got == want
    assert pipeline.imencode_pages(pages, quals) == got                   # two runs, equal bytes
    assert want[0] == one_by_one()[names[0]] and want[2] == one_by_one()[names[2]] and want[3] == one_by_one()[names[3]]
    assert want[1] != one_by_one()[names[1]]                              # quality 30 is not quality 85
    same = pipeline.imencode_pages(pages[:2], 85)                         # a scalar quality serves every page
    assert same == [one_by_one()[names[0]], one_by_one()[names[1]]]
    assert pipeline.imencode_pages([]) == []


def test_round_trip_through_the_decoder():
    """imdecode(imencode(x)) is PIL's decode of PIL's file: the bytes are equal, and the merged decoder equals PIL on them."""
    from ocr_vi_invoice_amd import pipeline
    got = one_by_one()
    out = pipeline.imdecode([got[n] for n in SMALL])
    for n, t in zip(SMALL, out):
        assert np.array_equal(t.cpu().numpy(), Z["d_" + n]), n


def test_host_and_device_inputs_give_the_same_bytes():
    from ocr_vi_invoice_amd import pipeline
    got = one_by_one()
    for n in ("s33x50_420_q85", "s33x50_grey_q85", "s40x57_444_q85"):
        img = image(n)
        q, sub = QUALITY[n], SUB[MODE[n]]
        assert pipeline.imencode(torch.from_numpy(img), q, sub) == got[n]
        assert pipeline.imencode(torch.from_numpy(img).cuda(), q, sub) == got[n]
        wide = torch.zeros((img.shape[0], img.shape[1] + 5) + img.shape[2:], dtype=torch.uint8, device="cuda")
        wide[:, :img.shape[1]] = torch.from_numpy(img).cuda()
        assert pipeline.imencode(wide[:, :img.shape[1]], q, sub) == got[n]          # a view that is not contiguous
    mixed = pipeline.imencode_pages([torch.from_numpy(image("s33x50_420_q85")).cuda(), image("s17x23_420_q85"),
                                     torch.from_numpy(image("s16x16_420_q85")).cuda()], 85)
    assert mixed == [got["s33x50_420_q85"], got["s17x23_420_q85"], got["s16x16_420_q85"]]


def test_imwrite_writes_a_file_imread_reads(tmp_path):
    from ocr_vi_invoice_amd import pipeline
    n = "s40x57_420_q85"
    path = str(tmp_path / "page.jpg")
    assert pipeline.imwrite(path, image(n), 85) is True
    with open(path, "rb") as f:
        assert f.read() == Z["j_" + n].tobytes()
    assert np.array_equal(pipeline.imread(path).cpu().numpy(), Z["d_" + n])
    assert pipeline.imwrite(str(tmp_path / "no" / "such" / "dir.jpg"), image(n), 85) is False


def test_strided_rows_bad_entries_and_short_regions_are_skipped():
    """The C entry alone: a source with padded rows, and entries the device must skip without touching their output."""
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    n = "s33x50_420_q85"
    img = image(n)
    h, w = img.shape[:2]
    s = pipeline.jpeg_encode_sizes(h, w, 3, "4:2:0")
    cap, wsb = (s["scan_capacity"] + 255) // 256 * 256, s["workspace_bytes"]
    stride = 3 * w + 7
    src = torch.zeros(h * stride + 64, dtype=torch.uint8)
    src[:h * stride].view(h, stride)[:, :3 * w] = torch.from_numpy(img).reshape(h, 3 * w)
    src = src.cuda()
    table = np.zeros((5, _lib.JPEG_ENC_ENTRY), np.int64)
    for k in range(5):
        _lib.check(lib.ocrvi_jpeg_encode_table_entry(w, h, 3, 2, 85, 0, stride, k * cap, cap, k * wsb, table[k].ctypes.data))
    table[1, 2] = 0                     # width 0
    table[2, 8] = 5 * wsb               # workspace region outside the workspace
    table[3, 7] = cap // 2              # output capacity below the bound
    table[4, 5] = 3                     # a sampling factor the encoder lacks
    out = torch.full((5 * cap,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.empty(5 * wsb, dtype=torch.uint8, device="cuda")
    lengths = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    d_tab = torch.from_numpy(table).cuda()
    _lib.check(lib.ocrvi_jpeg_encode_pages(0, src.data_ptr(), d_tab.data_ptr(), 5, out.data_ptr(), lengths.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    lens = lengths.cpu().tolist()
    e = ref(n)
    assert lens == [len(e.scan), 0, 0, 0, 0]
    host = out.cpu().numpy()
    assert host[:lens[0]].tobytes() == e.scan
    assert (host[lens[0]:] == 0xA5).all()
    with pytest.raises(ValueError):
        _lib.check(lib.ocrvi_jpeg_encode_pages(0, src.data_ptr(), None, 1, out.data_ptr(), lengths.data_ptr(), ws.data_ptr(), ws.numel(), None))


def test_refusals_raise_value_error_and_launch_nothing():
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    ok = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    lib.ocrvi_prof_reset()
    lib.ocrvi_prof_enable(1)
    try:
        for args in ((torch.zeros((8, 8, 3), device="cuda"),), (torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda"),),
                     (torch.zeros((0, 8, 3), dtype=torch.uint8, device="cuda"),), (torch.zeros((3, 65501), dtype=torch.uint8),),
                     (ok, 0), (ok, 101), (ok, 95, "4:2:2"), (ok, 95, "420")):
            with pytest.raises(ValueError):
                pipeline.imencode(*args)
        with pytest.raises(ValueError):
            pipeline.imencode_pages([ok, ok], [95])
        with pytest.raises(ValueError):
            pipeline.imwrite("unused.jpg", ok, 0)
        torch.cuda.synchronize()
        report = _lib.prof_report()                    # every launch of the library is bracketed while the profiler is on
    finally:
        lib.ocrvi_prof_enable(0)
        lib.ocrvi_prof_reset()
    assert not report, report
    assert not os.path.exists("unused.jpg")
