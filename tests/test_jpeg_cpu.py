"""The host half of the JPEG decoder (ocrvi_jpeg_info, ocrvi_jpeg_parse) and its NumPy reference (tests/jpeg_ref.py) against
tests/golden/jpeg_cases.npz (PIL / libjpeg-turbo's decode of PIL-encoded files; tests/golden/make_jpeg_golden.py).  No GPU."""
import ctypes as C
import hashlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402

from ocr_vi_invoice_amd import _lib, pipeline  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
Z = np.load(GOLD)
NAMES = [str(n) for n in Z["names"]]
KIND = {str(n): str(k) for n, k in zip(Z["names"], Z["kinds"])}
DECODABLE = [n for n in NAMES if KIND[n] != "bad"]
PINNED = [n for n in NAMES if KIND[n] in ("pil", "sha")]


def data(name) -> bytes:
    return Z["j_" + name].tobytes()


_REF = {}


def ref_parse(name):
    if name not in _REF:
        _REF[name] = jpeg_ref.parse(data(name))
    return _REF[name]


def expand(words: np.ndarray, n_blocks: int) -> np.ndarray:
    """The sparse stream -> int32 [n_blocks, 64], after the format's own consistency check."""
    check_stream(words, n_blocks)
    off = words[:n_blocks + 1].astype(np.int64)
    rec = words[n_blocks + 1:]
    out = np.zeros((n_blocks, 64), np.int32)
    blk = np.repeat(np.arange(n_blocks), np.diff(off))
    out[blk, rec >> 16] = (rec & 0xFFFF).astype(np.uint16).view(np.int16)
    return out


def check_stream(words: np.ndarray, n_blocks: int):
    assert words.size >= n_blocks + 1
    off = words[:n_blocks + 1].astype(np.int64)
    rec = words[n_blocks + 1:]
    assert off[0] == 0 and off[-1] == rec.size
    d = np.diff(off)
    assert (d >= 0).all() and (d <= 64).all(), "offsets not monotone"
    assert ((rec >> 16) < 64).all(), "position >= 64"


def raw_parse(buf: bytes, cap: int = None):
    """(rc, words, used, cap) of ocrvi_jpeg_parse, with the cap ocrvi_jpeg_info reports unless one is given."""
    lib = _lib.load()
    a = np.frombuffer(buf, np.uint8)
    info = _lib.JpegInfo()
    rc = lib.ocrvi_jpeg_info(a.ctypes.data if a.size else None, a.size, C.byref(info))
    if rc != 0:
        return rc, None, 0, 0, info
    cap = int(info.stream_bytes) if cap is None else cap
    out = np.full(cap // 4 + 8, 0xDEADBEEF, np.uint32)          # eight guard words behind the buffer
    used = C.c_size_t()
    rc = lib.ocrvi_jpeg_parse(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(used))
    assert (out[cap // 4:] == 0xDEADBEEF).all(), "ocrvi_jpeg_parse wrote past cap"
    assert used.value <= cap
    return rc, out[:used.value // 4], used.value, cap, info


@pytest.mark.parametrize("name", PINNED)
def test_reference_equals_pil(name):
    out = jpeg_ref.decode(data(name))
    assert hashlib.sha256(out.tobytes()).digest() == Z["h_" + name].tobytes()
    if KIND[name] == "pil":
        assert out.shape == Z["p_" + name].shape and np.array_equal(out, Z["p_" + name])


def test_stored_outputs_equal_a_fresh_pil_decode():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    for name in PINNED:
        rgb = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data(name)))).convert("RGB"))
        assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).digest() == Z["h_" + name].tobytes(), name


def test_fixture_covers_what_it_claims():
    infos = {n: jpeg_ref.info(data(n)) for n in DECODABLE}
    assert {(i["h_samp"][0], i["v_samp"][0]) for i in infos.values() if i["components"] == 3} == {(1, 1), (2, 1), (2, 2)}
    assert any(i["components"] == 1 for i in infos.values())
    assert sorted(infos[f"orient{k}_33x17"]["orientation"] for k in range(1, 9)) == list(range(1, 9))
    assert {infos[n]["restart_interval"] for n in ("rst1_33x17", "rst3_33x17", "rstrow_33x17")} == {1, 3, 2}
    d = data("q16_33x17")
    assert d[d.index(b"\xff\xdb") + 4] >> 4 == 1                                    # a 16-bit DQT
    seen = np.zeros(64, bool)
    for n in ("s97x131_444_q100", "s97x131_420_q85"):
        seen |= (ref_parse(n).blocks != 0).any(axis=0)
    assert seen.all(), "a coefficient position never occurs"


@pytest.mark.parametrize("name", DECODABLE)
def test_info_equals_reference(name):
    got, want = pipeline.jpeg_info(data(name)), jpeg_ref.info(data(name))
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    h = ref_parse(name)
    assert np.array_equal(got["quant"].astype(np.int64), np.stack(h.quant))
    assert got["workspace_bytes"] % 256 == 0
    hs, vs = want["h_samp"][0], want["v_samp"][0]
    planes = 64 * h.mcus_x * hs * h.mcus_y * vs + (2 * 64 * h.mcus_x * h.mcus_y if want["components"] == 3 else 0)
    assert planes <= got["workspace_bytes"] < planes + 256


@pytest.mark.parametrize("name", DECODABLE)
def test_parse_equals_reference_coefficients(name):
    h = ref_parse(name)
    rc, words, used, cap, info = raw_parse(data(name))
    assert rc == 0, _lib.last_error()
    assert info.blocks == h.n_blocks
    assert np.array_equal(expand(words, h.n_blocks), h.blocks)
    assert (words[h.n_blocks + 1:] & 0xFFFF != 0).all(), "a zero coefficient was stored"
    assert np.array_equal(pipeline.jpeg_parse(data(name)), words)
    if name == "s97x131_420_q85":                      # sparse: well under the 3 bytes per pixel of raw RGB
        assert used < 3 * 97 * 131


def _refused(buf, *words):
    lib = _lib.load()
    a = np.frombuffer(buf, np.uint8)
    info = _lib.JpegInfo()
    assert lib.ocrvi_jpeg_info(a.ctypes.data, a.size, C.byref(info)) == -1
    msg = info.reason.decode()
    assert "unsupported" in msg and any(w in msg for w in words), msg
    out = np.zeros(1 << 16, np.uint32)
    used = C.c_size_t()
    assert lib.ocrvi_jpeg_parse(a.ctypes.data, a.size, out.ctypes.data, out.nbytes, C.byref(used)) == -1
    assert any(w in _lib.last_error() for w in words)
    with pytest.raises(ValueError, match="|".join(words)):
        pipeline.jpeg_info(buf)
    with pytest.raises(jpeg_ref.Unsupported):
        jpeg_ref.parse(buf)


def test_unsupported_files_are_refused_by_name():
    _refused(data("progressive_33x17"), "progressive")
    _refused(data("cmyk_16x16"), "4 components")
    buf = bytearray(data("s16x16_420_q85"))            # 4:4:0: luma 1 x 2
    sof = buf.index(b"\xff\xc0")
    assert buf[sof + 11] == 0x22
    buf[sof + 11] = 0x12
    _refused(bytes(buf), "sampling factors")


def test_every_truncation_is_einval():
    buf = data("s17x33_420_q85")
    assert raw_parse(buf)[0] == 0
    for n in range(len(buf)):
        rc = raw_parse(buf[:n])[0]
        assert rc == -1, (n, rc)
        with pytest.raises(jpeg_ref.JpegError):
            jpeg_ref.parse(buf[:n])


def test_single_byte_corruptions_fail_cleanly_or_stay_consistent():
    buf = data("rst3_33x17")
    rng = np.random.default_rng(20261019)
    ok = bad = 0
    for _ in range(2000):
        b = bytearray(buf)
        p = int(rng.integers(0, len(b)))
        b[p] ^= int(rng.integers(1, 256))
        rc, words, used, cap, info = raw_parse(bytes(b))
        assert rc in (0, -1), rc
        if rc == 0:
            check_stream(words, int(info.blocks))
            ok += 1
        else:
            bad += 1
    assert ok > 0 and bad > 0, (ok, bad)


def test_short_cap_is_enomem():
    buf = data("s33x17_420_q85")
    rc, words, used, cap, info = raw_parse(buf)
    assert rc == 0
    for short in (0, 4 * int(info.blocks), used - 4):
        assert raw_parse(buf, cap=short)[0] == -3, short
    rc2, words2, used2, _, _ = raw_parse(buf, cap=used)
    assert rc2 == 0 and used2 == used and np.array_equal(words2, words)


def test_python_entry_points_raise_valueerror():
    with pytest.raises(ValueError, match="truncated|EOI|marker|Huffman"):
        pipeline.jpeg_parse(data("s33x17_420_q85")[:-40])
    with pytest.raises(ValueError, match="SOI"):
        pipeline.jpeg_info(b"not a jpeg at all")
    with pytest.raises(ValueError, match="JPEG bytes"):
        pipeline.jpeg_info(np.zeros(4, np.uint8))


def test_out_of_range_stream_saturates_in_the_reference():
    """Every quantisation entry patched to 255: dequantised coefficients leave [-16384, 16383] and the reference's two saturating steps
    (include/ocrvi.h) apply; the result is defined and not PIL's."""
    h = ref_parse("oor_33x17")
    comp = jpeg_ref.block_comp(h)
    dq = h.blocks.astype(np.int64) * np.stack(h.quant)[comp]
    assert np.abs(dq).max() >= jpeg_ref.SAT
    out = jpeg_ref.decode(data("oor_33x17"))
    assert out.shape == (33, 17, 3)


def _one_bit_dc_file(n_blocks: int) -> bytes:
    """A grey 8 x (8 n_blocks) file whose DC table codes category 0 in one bit and whose AC table codes (run 0, size 1) in one bit: after
    the first block a block costs 1 + 63 * 2 bits and yields 64 records, the densest stream the format allows."""
    import struct
    bits = ["10", "1"]                                 # block 0: DC category 1, difference +1
    for b in range(n_blocks):
        if b:
            bits.append("0")                           # DC category 0: the prediction stays 1, so DC is a record
        bits.append("01" * 63)                         # 63 coefficients of +1
    s = "".join(bits)
    s += "1" * (-len(s) % 8)
    scan = bytearray()
    for k in range(0, len(s), 8):
        v = int(s[k:k + 8], 2)
        scan.append(v)
        if v == 0xFF:
            scan.append(0)

    def seg(marker, body):
        return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body

    dht_dc = bytes([0x00, 1, 1] + [0] * 14 + [0, 1])                  # '0' -> category 0, '10' -> category 1
    dht_ac = bytes([0x10, 1, 1] + [0] * 14 + [0x01, 0x00])            # '0' -> (0, 1), '10' -> EOB
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([1] * 64)) + seg(0xC0, struct.pack(">BHHB", 8, 8, 8 * n_blocks, 1) + bytes([1, 0x11, 0]))
            + seg(0xC4, dht_dc) + seg(0xC4, dht_ac) + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + bytes(scan) + b"\xff\xd9")


def test_densest_stream_fits_the_cap_info_reports():
    """One record per coefficient at less than two bits of scan data per record: ocrvi_jpeg_parse must still fit info.stream_bytes."""
    buf = _one_bit_dc_file(64)
    h = jpeg_ref.parse(buf)
    assert (h.blocks == 1).all() and h.n_blocks == 64
    rc, words, used, cap, info = raw_parse(buf)
    assert rc == 0, _lib.last_error()
    assert words.size == 65 + 64 * 64 and used <= cap == info.stream_bytes
    assert 8 * (len(buf) - buf.index(b"\xff\xda") - 10) < 2 * 64 * 64          # fewer than two bits of scan data per record
    assert np.array_equal(expand(words, 64), h.blocks)
