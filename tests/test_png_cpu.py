"""The host half of the PNG decoder (ocrvi_png_info, ocrvi_png_parse, ocrvi_png_plan: chunks, CRC-32, the library's own inflate) against
the NumPy reference (tests/png_ref.py, inflate by zlib) on files from tests/png_cases.py, and the reference against
tests/golden/png_cases.npz (PIL's decode; tests/golden/make_png_golden.py).  No GPU."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as cases  # noqa: E402
import png_ref  # noqa: E402

from ocr_vi_invoice_amd import _lib, pipeline  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "png_cases.npz"))
NAMES = [str(n) for n in Z["names"]]
KIND = {str(n): str(k) for n, k in zip(Z["names"], Z["kinds"])}
INFO_KEYS = ("width", "height", "bit_depth", "colour_type", "channels", "row_bytes", "out_height", "out_width", "palette_entries", "idat_bytes",
             "stream_bytes", "workspace_bytes")


def host(data: bytes) -> bytes:
    """ocrvi_png_info + ocrvi_png_parse: the stream, of exactly stream_bytes bytes."""
    info = pipeline.png_info(data)
    out = pipeline.png_parse(data)
    assert out.size == info["stream_bytes"]
    return out.tobytes()


def one_file(colour, depth, seed=0, h=29, w=37, **kw):
    rng = np.random.default_rng(1000 * colour + depth + seed)
    samples = cases.random_samples(rng, h, w, colour, depth) * rng.integers(0, 2, (h, w, 1)) * rng.integers(0, 2, (h, w, 1))
    if kw.get("fixed"):                                      # runs, so that zlib prefers a fixed-Huffman block to a stored one
        samples = np.repeat(samples[:, :1], w, axis=1)
    palette = rng.integers(0, 256, (min(1 << depth, 200), 3)).astype(np.uint8) if colour == 3 else None
    filters = [cases.FILTER_PAIRS[(y + seed) % 25] for y in range(h)]
    return cases.write_png(samples, colour, depth, filters, palette, **kw)


VARIANTS = {"stored": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9), "fixed": dict(fixed=True),
            "split1": dict(split=1, empty_between=True), "split7": dict(split=7)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("colour,depth", cases.PAIRS)
def test_info_and_stream_equal_reference(colour, depth, variant):
    data = one_file(colour, depth, **VARIANTS[variant])
    got, want = pipeline.png_info(data), png_ref.info(data)
    assert {k: got[k] for k in INFO_KEYS} == want
    assert host(data) == png_ref.stream(data)


def test_stored_and_fixed_files_hold_such_blocks():
    """Level 0 gives stored blocks (the stream is longer than its data), Z_FIXED a first block of type 1, skewed samples one of type 2."""
    data = one_file(2, 8, level=0)
    z = b"".join(b for t, b in png_ref.chunks(data) if t == b"IDAT")
    assert (z[2] >> 1) & 3 == 0 and len(z) > 29 * (1 + 37 * 3)
    z = b"".join(b for t, b in png_ref.chunks(one_file(2, 8, fixed=True)) if t == b"IDAT")
    assert (z[2] >> 1) & 3 == 1
    skewed = cases.write_png(np.random.default_rng(5).integers(0, 4, (29, 37, 3)), 2, 8, [0] * 29, level=9)    # two bits of entropy per byte
    z = b"".join(b for t, b in png_ref.chunks(skewed) if t == b"IDAT")
    assert (z[2] >> 1) & 3 == 2 and host(skewed) == png_ref.stream(skewed)


@pytest.mark.parametrize("name", NAMES)
def test_golden_files(name):
    """The library's stream equals the reference's for every golden file; the reference's pixels equal PIL's wherever PIL is the claim."""
    data = Z["f_" + name].tobytes()
    assert host(data) == png_ref.stream(data)
    if KIND[name] == "pil":
        assert np.array_equal(png_ref.decode(data), Z["p_" + name])


def test_ancillary_chunks_are_skipped_without_their_crc():
    extra = b"".join(cases.chunk(t, b"\x01\x02\x03\x04", crc=0xDEADBEEF) for t in (b"tRNS", b"gAMA", b"cHRM", b"sRGB", b"iCCP", b"bKGD", b"pHYs",
                                                                                   b"eXIf", b"tEXt", b"acTL", b"fcTL"))
    plain = one_file(2, 8)
    data = one_file(2, 8, before_idat=extra, after_idat=cases.chunk(b"fdAT", bytes(9), crc=1) + cases.chunk(b"tIME", bytes(7), crc=2))
    assert host(data) == host(plain) == png_ref.stream(plain)
    # a PLTE in a truecolour file is a suggested palette: read past, palette_entries stays 0
    sug = one_file(2, 8, before_idat=cases.chunk(b"PLTE", bytes(12)))
    assert host(sug) == host(plain) and pipeline.png_info(sug)["palette_entries"] == 0


def test_bytes_after_the_zlib_stream_are_ignored():
    rows = cases.filter_rows(cases.pack_rows(np.arange(12).reshape(3, 4, 1), 8), 1, [0, 1, 2])
    data = raw_png(zlib.compress(rows.tobytes()) + b"trailing bytes", 4, 3, 0, 8)
    assert host(data) == rows.tobytes()


# ---------------------------------------------------------------------------------------------- refusals
def raw_png(z: bytes, w, h, colour, depth, plte: bytes = None) -> bytes:
    return (cases.SIGNATURE + cases.ihdr(w, h, depth, colour) + (cases.chunk(b"PLTE", plte) if plte is not None else b"")
            + cases.chunk(b"IDAT", z) + cases.chunk(b"IEND"))


def refused(data: bytes, word: str):
    with pytest.raises(ValueError, match=word):
        host(data)


def test_refused_features():
    rows = bytes(2 * 3)                                      # 2 x 2 grey 8-bit, filter 0
    z = zlib.compress(rows)
    idat = cases.chunk(b"IDAT", z)
    end = cases.chunk(b"IEND")
    S = cases.SIGNATURE
    refused(S + cases.ihdr(2, 2, 8, 0, interlace=1) + idat + end, "Adam7")
    refused(S + cases.ihdr(2, 2, 8, 0, compression=1) + idat + end, "compression method 1")
    refused(S + cases.ihdr(2, 2, 8, 0, filter_method=1) + idat + end, "filter method 1")
    for colour, depth in ((2, 4), (3, 16), (4, 2), (6, 1), (0, 3), (1, 8), (5, 8), (0, 0)):
        refused(S + cases.ihdr(2, 2, depth, colour) + idat + end, f"illegal pair of colour type {colour} and bit depth {depth}")
    for w, h in ((0, 2), (2, 0), (65501, 2), (2, 65501), (2 ** 31, 2)):
        refused(S + cases.ihdr(w, h, 8, 0) + idat + end, "a side of 0 or above 65500")
    refused(S + cases.ihdr(2, 2, 8, 3) + idat + end, "without PLTE")
    refused(S + cases.ihdr(2, 2, 8, 3) + idat + cases.chunk(b"PLTE", bytes(6)) + end, "without PLTE")       # PLTE after IDAT
    refused(S + cases.ihdr(2, 2, 8, 3) + cases.chunk(b"PLTE", bytes(4)) + idat + end, "not a multiple of 3")
    refused(S + cases.ihdr(2, 2, 8, 3) + cases.chunk(b"PLTE", bytes(771)) + idat + end, "above 256")
    refused(S + cases.ihdr(2, 2, 8, 0) + cases.chunk(b"ABCD", b"x") + idat + end, "unknown critical chunk ABCD")
    refused(S + cases.chunk(b"CgBI", bytes(4)) + cases.ihdr(2, 2, 8, 0) + idat + end, "unknown critical chunk CgBI")
    half = len(z) // 2
    refused(S + cases.ihdr(2, 2, 8, 0) + cases.chunk(b"IDAT", z[:half]) + cases.chunk(b"tEXt", b"k\0v") + cases.chunk(b"IDAT", z[half:]) + end,
            "not consecutive")
    refused(S + cases.ihdr(2, 2, 8, 0) + idat, "no IEND")
    refused(S + cases.ihdr(2, 2, 8, 0) + end, "no IDAT")
    refused(b"not a png at all", "signature")
    refused(b"", "signature")
    # the same file, untouched, parses
    assert host(S + cases.ihdr(2, 2, 8, 0) + idat + end) == rows


def test_wrong_crc_and_flipped_bytes():
    data = one_file(3, 8)
    pos, where = 8, {}
    for typ, body in png_ref.chunks(data):
        where.setdefault(typ, (pos, len(body)))
        pos += 12 + len(body)
    for typ in (b"IHDR", b"PLTE", b"IDAT", b"IEND"):
        p, n = where[typ]
        crc_at = p + 8 + n
        bad = bytearray(data)
        bad[crc_at + 3] ^= 1                                  # the CRC itself
        refused(bytes(bad), f"wrong CRC on the {typ.decode()} chunk")
        if n:                                                 # a byte of the body: the CRC no longer matches (or the field is refused)
            bad = bytearray(data)
            bad[p + 8 + n // 2] ^= 0x10
            with pytest.raises(ValueError):
                host(bytes(bad))


@pytest.mark.parametrize("name", ["t2_d8", "pil_P_std"])
def test_every_prefix_is_refused(name):
    data = Z["f_" + name].tobytes()
    lib = _lib.load()
    info = _lib.PngInfo()
    out = np.empty(pipeline.png_info(data)["stream_bytes"], np.uint8)
    used = C.c_size_t()
    for n in range(len(data)):
        buf = np.frombuffer(data[:n], np.uint8)
        ptr = buf.ctypes.data if n else None
        assert lib.ocrvi_png_info(ptr, n, C.byref(info)) == -1, n
        assert info.reason, n
        assert lib.ocrvi_png_parse(ptr, n, out.ctypes.data, out.nbytes, C.byref(used)) == -1 and used.value == 0, n


class BitWriter:
    """Deflate's bit order: fields least significant bit first, Huffman codes most significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, k):
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):
        for i in range(k - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def canonical(lengths: dict) -> dict:
    """{symbol: length} -> {symbol: (code, length)}, RFC 1951's assignment."""
    out, code = {}, 0
    for ln in range(1, 16):
        for sym in sorted(s for s, v in lengths.items() if v == ln):
            out[sym] = (code, ln)
            code += 1
        code <<= 1
    return out


ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(w: BitWriter, cl_lengths: dict, symbols, nlen: int, ndist: int) -> None:
    """A final dynamic block's header: the code-length code, then ``symbols`` [(code-length symbol, extra bits value)]."""
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(nlen - 257, 5)
    w.bits(ndist - 1, 5)
    w.bits(15, 4)
    for s in ORDER:
        w.bits(cl_lengths.get(s, 0), 3)
    cl = canonical(cl_lengths)
    for sym, extra in symbols:
        w.code(*cl[sym])
        if sym == 16:
            w.bits(extra, 2)
        elif sym == 17:
            w.bits(extra, 3)
        elif sym == 18:
            w.bits(extra, 7)


def zwrap(deflate: bytes, output: bytes) -> bytes:
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(output))


CL = {1: 2, 2: 2, 18: 1}                                     # a complete code-length code over the symbols 1, 2 and 18


def single_distance_code_block(distance_bit: int) -> bytes:
    """Literal/length code {0: 2 bits, 256: 2 bits, 257: 1 bit} (complete), one distance code of one bit (the incomplete set zlib
    accepts).  Data: literal 0, then length 3 with the distance bit given: 0 is distance 1, 1 is the code that has no symbol."""
    w = BitWriter()
    dynamic_header(w, CL, [(2, 0), (18, 127), (18, 106), (2, 0), (1, 0), (1, 0)], 258, 1)
    lit = canonical({0: 2, 256: 2, 257: 1})
    w.code(*lit[0])
    w.code(*lit[257])
    w.bits(distance_bit, 1)
    w.code(*lit[256])
    return w.done()


def test_untrusted_deflate_streams():
    rows = bytes(4)                                          # 1 x 2 grey 8-bit: two rows of (filter 0, sample 0)
    good = zlib.compress(rows)

    def png(z):
        return raw_png(z, 1, 2, 0, 8)

    assert host(png(good)) == rows
    refused(png(bytes([0x79, 0x01]) + good[2:]), "compression method 9")
    refused(png(bytes([0x88, 0x1C]) + good[2:]), "window")                     # CINFO 8: 64 K
    refused(png(bytes([0x78, 0x02]) + good[2:]), "FCHECK")
    refused(png(bytes([0x78, 0x20 | (31 - (0x7820 % 31))]) + good[2:]), "preset dictionary")
    refused(png(b"\x78\x01" + b"\x07"), "reserved deflate block type")
    refused(png(b"\x78\x01" + b"\x01\x04\x00\x00\x00" + rows), "does not match its complement")
    assert host(png(zwrap(b"\x01\x04\x00\xfb\xff" + rows, rows))) == rows                       # the same stored block, well-formed
    w = BitWriter()                                          # three code-length codes of one bit
    dynamic_header(w, {0: 1, 1: 1, 2: 1}, [], 257, 1)
    refused(png(zwrap(w.done(), rows)), "over-subscribed")
    w = BitWriter()                                          # literals 0, 1 and 256 all of one bit
    dynamic_header(w, CL, [(1, 0), (1, 0), (18, 127), (18, 105), (1, 0), (1, 0)], 257, 1)
    refused(png(zwrap(w.done(), rows)), "over-subscribed literal/length")
    w = BitWriter()                                          # literals 0 and 256 of two bits each and nothing else
    dynamic_header(w, CL, [(2, 0), (18, 127), (18, 106), (2, 0), (1, 0)], 257, 1)
    refused(png(zwrap(w.done(), rows)), "incomplete literal/length")
    assert host(png(zwrap(single_distance_code_block(0), rows))) == rows       # the single-code set zlib accepts, and a distance of 1
    assert zlib.decompress(zwrap(single_distance_code_block(0), rows)) == rows
    refused(png(zwrap(single_distance_code_block(1), rows)), "distance code with no symbol")
    w = BitWriter()                                          # a fixed block that opens with length 3, distance 1: nothing to copy from
    w.bits(1, 1)
    w.bits(1, 2)
    w.code(1, 7)
    w.code(0, 5)
    w.code(0, 7)
    refused(png(zwrap(w.done(), rows)), "before the start of the output")
    refused(png(good[:-1] + bytes([good[-1] ^ 1])), "Adler-32")
    refused(png(good[:-2]), "Adler-32")
    refused(png(zlib.compress(rows[:-1])), "shorter")
    refused(png(zlib.compress(rows + b"\0")), "longer")
    refused(png(zlib.compress(rows + b"\0", 0)), "longer")
    refused(png(zlib.compress(b"\0\0\5\0")), "filter byte 5")
    refused(png(good[:6]), "truncated")


def test_short_cap_is_enomem_and_nothing_is_written():
    data = one_file(2, 8)
    info = pipeline.png_info(data)
    buf = np.full(info["stream_bytes"] + 64, 0xA5, np.uint8)
    used = C.c_size_t(7)
    rc = _lib.load().ocrvi_png_parse(np.frombuffer(data, np.uint8).ctypes.data, len(data), buf.ctypes.data, info["stream_bytes"] - 1, C.byref(used))
    assert rc == -3 and used.value == 0 and (buf == 0xA5).all()
    with pytest.raises(MemoryError):
        pipeline.png_parse_into(data, buf.ctypes.data, 10)
    assert pipeline.png_parse_into(data, buf.ctypes.data, info["stream_bytes"]) == info["stream_bytes"]
    assert (buf[info["stream_bytes"]:] == 0xA5).all()                           # exact: nothing past the stream


def test_jpeg_messages_are_unchanged():
    with pytest.raises(ValueError, match="SOI"):
        pipeline.jpeg_info(b"not a jpeg at all")
    assert pipeline.IMAGE_BYTES == pipeline.JPEG_BYTES == (bytes, bytearray, memoryview)
    assert pipeline.is_png(memoryview(one_file(0, 8))) and not pipeline.is_png(b"\xff\xd8\xff") and not pipeline.is_png(np.zeros(8, np.uint8))


def test_exports_match_the_header():
    hdr = open(os.path.join(HERE, "..", "include", "ocrvi.h")).read()
    lib = _lib.load()
    for name in ("ocrvi_png_info", "ocrvi_png_parse", "ocrvi_png_table_entry", "ocrvi_png_plan", "ocrvi_png_decode_pages"):
        assert f"int {name}(" in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
    assert f"#define OCRVI_PNG_ENTRY {_lib.PNG_ENTRY}\n" in hdr
    assert C.sizeof(_lib.PngInfo) == 10 * 4 + 3 * 8 + 160
    assert lib.ocrvi_abi_version() == _lib.ABI_VERSION == 5                      # exports were added, nothing changed


@pytest.mark.parametrize("h,row_bytes", [(1, 1), (7, 24), (255, 25), (256, 48), (257, 49), (513, 7), (1280, 3840)])
def test_plan(h, row_bytes):
    """One band, a band's edge, several bands; the line between bands is there from the second band on."""
    data = cases.SIGNATURE + cases.ihdr(row_bytes, h, 8, 0) + cases.chunk(b"IDAT", b"") + cases.chunk(b"IEND")
    info = pipeline.png_info_struct(data)
    plan = pipeline.png_plan(info)
    assert plan == png_ref.plan(h, row_bytes)
    chunks = -(-row_bytes // 24)
    assert plan["band_rows"] == 256 and plan["chunk_bytes"] == 24 and plan["bands"] == -(-h // 256)
    assert plan["steps"] == plan["bands"] * (chunks - 1) + h
    assert info.workspace_bytes == (0 if h <= 256 else -(-chunks * 24 // 256) * 256) and info.workspace_bytes % 256 == 0
    entry = np.zeros(_lib.PNG_ENTRY, np.int64)
    pipeline.png_table_entry(info, info.stream_bytes, 256, -512, 3 * row_bytes + 5, 1024, entry)
    assert entry.tolist() == [256, h * (1 + row_bytes), row_bytes, h, 8, 0, 0, -512, 3 * row_bytes + 5, 1024] + [0] * 6
    with pytest.raises(ValueError, match="stride"):
        pipeline.png_table_entry(info, info.stream_bytes, 0, 0, 3 * row_bytes - 1, 0, entry)
    with pytest.raises(ValueError, match="used"):
        pipeline.png_table_entry(info, info.stream_bytes - 1, 0, 0, 3 * row_bytes, 0, entry)
