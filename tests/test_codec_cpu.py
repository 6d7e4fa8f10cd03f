"""What ocr_vi_invoice_amd/codec.py shares between its two formats and no other test reaches without a GPU: the encode jobs' common page
validation, the header pass of ``imdecode`` and the dispatch of the generic decode wrappers.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases  # noqa: E402

from ocr_vi_invoice_amd import _lib, codec, pipeline  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def good_jpeg() -> bytes:
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    name = next(str(n) for n, k in zip(z["names"], z["kinds"]) if str(k) != "bad")
    return z["j_" + name].tobytes()


@pytest.fixture(scope="module")
def good_png() -> bytes:
    samples = png_cases.random_samples(np.random.default_rng(7), 9, 11, 2, 8)
    return png_cases.write_png(samples, 2, 8, [y % 5 for y in range(9)])


GOOD = np.zeros((8, 8, 3), np.uint8)
BAD_PAGES = [
    ([[[0, 0, 0]]], "w: page 0: expected a numpy array or a tensor, got list"),
    ([np.zeros((8, 8, 3), np.float32)], "w: page 0: dtype float32 (uint8 expected)"),
    ([np.zeros((8, 8, 4), np.uint8)], "w: page 0: shape (8, 8, 4) (H x W x 3 RGB or H x W grey expected)"),
    ([np.zeros((8,), np.uint8)], "w: page 0: shape (8,) (H x W x 3 RGB or H x W grey expected)"),
    ([np.zeros((0, 8), np.uint8)], "w: page 0: sides 0 x 8 outside 1..65500"),
    ([GOOD, np.broadcast_to(np.uint8(0), (8, 65501))], "w: page 1: sides 8 x 65501 outside 1..65500"),
]


@pytest.mark.parametrize("job", [pipeline.JpegEncodeJob, pipeline.PngEncodeJob], ids=["jpeg", "png"])
@pytest.mark.parametrize("pages, message", BAD_PAGES, ids=["type", "dtype", "channels", "rank", "empty", "second-page"])
def test_both_jobs_refuse_a_bad_page_with_the_same_text(job, pages, message):
    with pytest.raises(ValueError) as e:
        job(pages, what="w")
    assert str(e.value) == message


def test_a_page_the_sizes_entry_refuses_is_named_in_both_formats():
    """Sides within 1..65500 do not guarantee that ``ocrvi_jpeg_encode_sizes`` accepts the page: it needs 208 bytes x blocks < 2^32,
    about 20.6 million blocks, and a 40000 x 40000 grey page has 5000 x 5000 = 25 million.  The job names the refused page, as the
    PNG job does for a page past its IDAT bound."""
    big = np.broadcast_to(np.uint8(0), (40000, 40000))        # (no memory behind it; the constructor reads only its shape)
    with pytest.raises(ValueError, match=r"^w: page 1: jpeg_encode_sizes: 40000 x 40000 has 25000000 blocks"):
        pipeline.JpegEncodeJob([GOOD, big], what="w")
    with pytest.raises(ValueError, match=r"^w: page 1: png_encode_sizes: "):
        pipeline.PngEncodeJob([GOOD, np.broadcast_to(np.uint8(0), (65500, 65500, 3))], what="w")


def test_constructors_lay_out_good_pages_without_a_device():
    pages = [GOOD, np.zeros((5, 9), np.uint8)]
    j, p = pipeline.JpegEncodeJob(pages, quality=[90, 50]), pipeline.PngEncodeJob(pages)
    assert j.geom == [(8, 8, 3, 2), (5, 9, 1, 1)] and p.geom == [(8, 8, 3), (5, 9, 1)]
    for job in (j, p):
        assert len(job.caps) == 2 and len(job.w_off) == len(job.o_off) == 3 and job.o_off[2] == sum(job.caps)
        assert job.lengths is None and job.out is None
    assert [o[9] for o in p.offsets] == [p.w_off[1], p.w_off[2] - p.w_off[1]]


def test_imdecode_reads_every_header_in_the_callers_order_first(good_png):
    bad_jpeg, bad_png = b"no SOI here", good_png[:20]
    with pytest.raises(ValueError, match=r"^imdecode: file 1: "):      # (still in the header pass: nothing here has a device)
        pipeline.imdecode([good_png, bad_jpeg, bad_png])
    with pytest.raises(ValueError, match=r"^imdecode: file 0: "):
        pipeline.imdecode([bad_png, bad_jpeg])
    with pytest.raises(ValueError, match=r"^imdecode: "):
        pipeline.imdecode(bad_png)
    assert pipeline.imdecode([]) == []


def _fields(info):
    return {name: bytes(getattr(info, name)) if isinstance(getattr(info, name), C.Array) else getattr(info, name) for name, _ in info._fields_}


def test_generic_wrappers_dispatch_by_signature_and_by_info(good_jpeg, good_png):
    for data, fmt, cls, info_of, parse in ((good_jpeg, codec.JPEG, _lib.JpegInfo, pipeline.jpeg_info_struct, pipeline.jpeg_parse),
                                           (good_png, codec.PNG, _lib.PngInfo, pipeline.png_info_struct, pipeline.png_parse)):
        assert codec.format_of(data) is fmt and codec.format_of(memoryview(data)) is fmt
        info = codec.info_struct(data, "x")
        assert type(info) is cls and codec.format_of_info(info) is fmt
        assert _fields(info) == _fields(info_of(data))
        want = parse(data)
        buf = np.full(info.stream_bytes + 8, 0xA5, np.uint8)
        used = codec.parse_into(info, data, buf.ctypes.data, info.stream_bytes, "x")
        assert used == want.nbytes and buf[:used].tobytes() == want.tobytes() and (buf[info.stream_bytes:] == 0xA5).all()
        entry, same = np.zeros(fmt.entry_width, np.int64), np.zeros(fmt.entry_width, np.int64)
        codec.table_entry(info, used, 256, 512, 3 * info.out_width, 0, entry)
        fmt.table_entry(info, used, 256, 512, 3 * info.out_width, 0, same)
        assert entry.any() and (entry == same).all()
    assert codec.format_of(b"") is codec.JPEG and codec.format_of(None) is codec.JPEG and not pipeline.is_png(None)
    with pytest.raises(ValueError, match=r"^jpeg: .*SOI"):            # the JPEG binding stays the JPEG parser, whatever the signature
        pipeline.jpeg_info_struct(good_png)
    with pytest.raises(ValueError, match=r"^: "):                     # an empty ``what`` is used as given, only a missing one is the name
        pipeline.png_info_struct(good_png[:20], "")
    assert pipeline.jpeg_parse(good_jpeg).dtype == np.uint32 and pipeline.png_parse(good_png).dtype == np.uint8
