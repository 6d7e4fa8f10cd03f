"""The PNG encoder's arithmetic and host entries without a GPU: tests/pngenc_ref.py's file for every case checked by independent
readers (tests/png_ref.py, zlib, PIL when present, the library's own host inflate), its codes checked for completeness, the bound, the
stored digests, the library's host entries against the reference, and a table of mutants -- each rule changed, each change seen in
the bytes of at least one case."""
import hashlib
import io
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
import pngenc_ref  # noqa: E402
from pngenc_cases import B, BIG, NAMES, PAGE, RUNS, code_histograms, filters, golden, image, ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("ocrvi_png_encode_sizes", "ocrvi_png_encode_table_entry", "ocrvi_png_encode_pages", "ocrvi_test_png_code_lengths")


def rgb(img):
    return img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)


def idat(data: bytes) -> bytes:
    ch = png_ref.chunks(data)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    return ch[1][1]


def test_exports_match_the_header_and_the_abi_is_still_5():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    with open(os.path.join(HERE, "..", "include", "ocrvi.h")) as f:
        header = f.read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and hasattr(lib, n) and re.search(r"\bint " + n + r"\(", header), n
    assert f"#define OCRVI_PNG_ENC_ENTRY {_lib.PNG_ENC_ENTRY}\n" in header
    assert f"#define OCRVI_PNG_ENC_BLOCK {_lib.PNG_ENC_BLOCK}\n" in header and _lib.PNG_ENC_BLOCK == B <= 65535
    assert lib.ocrvi_abi_version() == 5 == _lib.ABI_VERSION


@pytest.mark.parametrize("name", NAMES)
def test_reference_file_is_read_back_four_ways(name):
    from ocr_vi_invoice_amd import pipeline
    e, img = ref(name), image(name)
    assert np.array_equal(png_ref.decode(e.data), rgb(img))
    z = idat(e.data)
    assert zlib.decompress(z) == e.stream.tobytes()
    assert z[:2] == b"\x78\x01" and z[2:-4] == e.deflate
    assert zlib.adler32(e.stream.tobytes()) == e.adler and zlib.crc32(b"IDAT" + z) == e.crc
    assert pipeline.png_parse(e.data).tobytes() == e.stream.tobytes()          # the library's own inflate, on this encoder's blocks
    info = pipeline.png_info(e.data)
    assert (info["height"], info["width"], info["bit_depth"], info["colour_type"]) == (img.shape[0], img.shape[1], 8, 2 if img.ndim == 3 else 0)
    assert hashlib.sha256(e.data).digest() == golden()["h_" + name].tobytes()
    assert e.data[:33] == pngenc_ref.header(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3)


@pytest.mark.parametrize("name", NAMES)
def test_reference_file_decodes_under_pil(name):
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(ref(name).data))), image(name))


def test_reference_on_the_page():
    """One 960 x 1280 synth.make_invoice page: 226 blocks, all dynamic; the digest the GPU test compares with."""
    from ocr_vi_invoice_amd import pipeline
    e, g = ref(PAGE), golden()
    assert (len(e.data), hashlib.sha256(e.data).digest()) == (int(g["n_" + PAGE]), g["h_" + PAGE].tobytes())
    assert zlib.decompress(idat(e.data)) == e.stream.tobytes()
    assert pipeline.png_parse(e.data).tobytes() == e.stream.tobytes()
    assert len(e.blocks) == 226 > 128


def test_reference_on_the_many_block_case():
    """265 blocks: the per-page scan walks them in chunks of 256, and the blocks of the second chunk are stored ones, whose padding
    depends on the position carried over from the first."""
    e, g = ref(BIG), golden()
    assert (len(e.data), hashlib.sha256(e.data).digest()) == (int(g["n_" + BIG]), g["h_" + BIG].tobytes())
    assert zlib.decompress(idat(e.data)) == e.stream.tobytes()
    types = [b.type for b in e.blocks]
    assert len(types) == 265 and set(types[:256]) == {2} and types[257:] == [0] * 8
    assert e.bit_offsets[257] % 8 != 0 or e.bit_offsets[256] % 8 != 0


def test_the_cases_reach_the_rules_they_are_there_for():
    assert list(ref("tie_5x9").filters) == [1, 2, 2, 2, 2]
    assert set(ref("walk_26x20_adaptive").filters) == {0, 1, 2, 3, 4}
    assert (1 + image("rgb_7x6").shape[1] * 3) % 4 != 0
    want = {1: [], 2: [], 3: [], 4: [3], 258: [257], 259: [258], 260: [258], 261: [258], 262: [258, 3], 517: [258, 258]}
    for n in RUNS:
        b = ref(f"run_{n}").blocks[0]
        assert [int(v) for v in b.length if v] == want[n], n
        assert int((b.length == 0).sum()) + sum(want[n]) == n + 3
    b = ref("zeros_40x50").blocks[0]                                          # the run goes through the filter bytes
    assert int((b.length == 0).sum()) == 1 and int(b.length.sum()) == 40 * 51 - 1
    assert [len(ref(n).stream) - B for n in ("exact_B", "B_minus_1", "B_plus_1")] == [0, -1, 1]
    assert [len(ref(n).blocks) for n in ("exact_B", "B_minus_1", "B_plus_1")] == [1, 1, 2]
    e = ref("cross_130x127")
    assert len(e.blocks) == 2 and list(e.blocks[1].length) == [256] and e.blocks[1].pos[0] == 0     # block 1 is one match
    assert int(e.blocks[0].length.sum()) + int((e.blocks[0].length == 0).sum()) == B            # and no match crosses the block's end
    assert [b.type for b in ref("noise_64x64").blocks] == [pngenc_ref.STORED]
    e = ref("mix_385x127")
    assert [b.type for b in e.blocks] == [0, 2, 0, 1] and e.bit_offsets[2] % 8 != 0
    b = ref("tie_types_1x40").blocks[0]
    assert pngenc_ref.stored_bits(0, 41) == b.fixed_bits < b.dynamic_bits and b.type == pngenc_ref.STORED
    assert max(int(b.lens.max()) for n in NAMES for b in ref(n).blocks) <= 15


def test_every_code_is_complete_and_within_its_limit():
    def kraft(lens, limit):
        return sum(1 << (limit - int(v)) for v in lens if v)
    for n in NAMES + [PAGE]:
        for b in ref(n).blocks:
            assert kraft(b.lens, 15) == 1 << 15 and int(b.lens.max()) <= 15, n
            assert kraft(b.cl_lens, 7) == 1 << 7 and int(b.cl_lens.max()) <= 7, n
            assert b.lens[256] > 0
    hit = {}
    for label, counts, limit in code_histograms():
        for row in counts:
            lens = pngenc_ref.code_lengths(row, limit)
            assert kraft(lens, limit) == 1 << limit and int(lens.max()) <= limit, (label, row)
            assert all(lens[k] > 0 for k in np.flatnonzero(row))
            hit[label] = max(hit.get(label, 0), int(lens.max()))
        # an optimal code where the limit does not bind: more frequent symbols never get longer codes
        order = np.argsort(counts[-1], kind="stable")
        used = [k for k in order if counts[-1][k]]
        lens = pngenc_ref.code_lengths(counts[-1], limit)
        assert all(lens[a] >= lens[b] for a, b in zip(used[:-1], used[1:]))
    assert hit == {"literal/length": 15, "code-length": 7}                      # the Fibonacci counts reach both limits


def test_sizes_and_the_bound():
    from ocr_vi_invoice_amd import pipeline
    for n in NAMES + [PAGE]:
        img, e = image(n), ref(n)
        nc = 1 if img.ndim == 2 else 3
        s, want = pipeline.png_encode_sizes(img.shape[0], img.shape[1], nc), pngenc_ref.sizes(img.shape[0], img.shape[1], nc)
        assert (s["stream_bytes"], s["blocks"], s["out_capacity"]) == (want["stream_bytes"], want["blocks"], want["capacity"]) == (
            len(e.stream), len(e.blocks), 63 + 5 * len(e.blocks) + len(e.stream)), n
        assert len(e.data) <= s["out_capacity"], n
        o = s["offsets"]
        assert s["workspace_bytes"] % 256 == 0 and s["workspace_bytes"] >= o[8] + 32 and all(v % 16 == 0 for v in o)
        sizes = [img.shape[0], len(e.stream) + 16, 1152 * s["blocks"], 320 * s["blocks"], 640 * s["blocks"], 32 * s["blocks"], 8 * (s["blocks"] + 1),
                 4 * (len(e.data) // 4096 + 1)]
        assert all(o[k + 1] - o[k] >= sizes[k] for k in range(8)), n
    e = ref("noise_64x64")                                                      # stored: the bound is reached but for the padding
    assert len(e.data) == 63 + 5 + len(e.stream)


def test_host_entries_refuse_bad_arguments():
    from ocr_vi_invoice_amd import _lib, pipeline
    lib = _lib.load()
    entry = np.full(_lib.PNG_ENC_ENTRY, -1, np.int64)
    cap = pipeline.png_encode_sizes(33, 50, 3)["out_capacity"]
    _lib.check(lib.ocrvi_png_encode_table_entry(50, 33, 3, 5, -4096, 157, 512, cap, 256, entry.ctypes.data))
    assert list(entry[:9]) == [-4096, 157, 50, 33, 3, 5, 512, cap, 256] and not entry[9:].any()
    for args in ((0, 33, 3, 5, 0, 150, 0, cap, 0), (50, 65501, 3, 5, 0, 150, 0, cap, 0), (50, 33, 2, 5, 0, 150, 0, cap, 0),
                 (50, 33, 3, 6, 0, 150, 0, cap, 0), (50, 33, 3, -1, 0, 150, 0, cap, 0), (50, 33, 3, 5, 0, 149, 0, cap, 0),
                 (50, 33, 3, 5, 0, 150, 0, cap - 1, 0), (50, 33, 3, 5, 0, 150, 0, cap, 8), (50, 33, 3, 5, 0, 150, 8, cap, 0)):
        assert lib.ocrvi_png_encode_table_entry(*args, entry.ctypes.data) == -1, args
    assert lib.ocrvi_png_encode_table_entry(50, 33, 3, 5, 0, 150, 0, cap, 0, None) == -1
    for h, w, nc in ((0, 5, 3), (5, 65501, 1), (5, 5, 4), (65500, 65500, 1)):   # the last: an IDAT that could pass 2^31 - 1 bytes
        with pytest.raises(ValueError):
            pipeline.png_encode_sizes(h, w, nc)
    assert pipeline.png_encode_sizes(32000, 65500, 1)["out_capacity"] < 2 ** 31


def test_job_refuses_before_the_device_is_touched():
    """Every refusal is a ValueError raised by the constructor, which has no device code in it (this test runs without a GPU)."""
    from ocr_vi_invoice_amd import pipeline
    ok = np.zeros((8, 8, 3), np.uint8)
    bad = [dict(images=[np.zeros((8, 8, 3), np.float32)]), dict(images=[np.zeros((8, 8, 4), np.uint8)]), dict(images=[np.zeros((8,), np.uint8)]),
           dict(images=[np.zeros((0, 8, 3), np.uint8)]), dict(images=[np.zeros((8, 65501), np.uint8)]), dict(images=[[1, 2, 3]]),
           dict(images=[ok], filters="best"), dict(images=[ok], filters=5), dict(images=[np.broadcast_to(np.uint8(0), (65500, 65500))])]     # an IDAT that could pass 2^31 - 1 bytes
    for kw in bad:
        with pytest.raises(ValueError):
            pipeline.PngEncodeJob(**kw)
    job = pipeline.PngEncodeJob([ok, np.zeros((5, 9), np.uint8)], "paeth")
    assert job.geom == [(8, 8, 3), (5, 9, 1)]
    with pytest.raises(ValueError):
        pipeline.imwrite("unused.png", ok, format="jpg")
    with pytest.raises(ValueError):
        pipeline.save_result("unused.png", ok, [], format="PNG")
    assert not os.path.exists("unused.png")


MUTANTS = {"the adaptive tie goes to the higher filter": dict(tie_lower=False),
           "matches are split at 257": dict(split=257),
           "a remainder of 3 is written as literals": dict(min_rem=4),
           "a remainder of 2 is written as a match": dict(min_rem=2),
           "a run does not continue from the previous block": dict(cross_block=False),
           "the block-type tie goes to the later type": dict(type_tie_earlier=False),
           "a stored block's padding ignores its header bits": dict(pad_counts_header=False)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_changes_the_bytes_of_some_case(mutant):
    rules = pngenc_ref.Rules(**MUTANTS[mutant])
    changed = [n for n in NAMES if pngenc_ref.encode(image(n), filters(n), rules).data != ref(n).data]
    assert changed, mutant


SIZE_MARGIN_PER_BLOCK = 16      # bytes


def test_size_against_zlib_rle():
    """The tokens are Z_RLE's kind, so the IDAT stays within zlib's Z_RLE (level 6) output of the same filtered stream plus what cutting
    the stream into independent blocks costs: one dynamic header per 16 KiB.  Measured with stdlib zlib on one 960 x 1280
    synth.make_invoice page (profiles/r21_png_encode.md): 0.9998 x Z_RLE on the noisy page, RGB and grey (the per-block codes fit better
    than zlib's, which outweighs the headers); 48 873 against 46 107 bytes on the page thresholded to clean paper as RGB, 25 289 against
    24 410 as grey -- 12.2 and 11.6 bytes a block, which is the header itself (17 bits, 3 HCLEN, some twenty code-length symbols).  The
    margin is that measured cost rounded up to 16 bytes a block; Huffman-only coding of the clean RGB page is 474 907 bytes and zlib
    level 1 58 179, so a matcher that stopped working, or codes that stopped adapting, would not fit."""
    page = image(PAGE)
    for name, img in (("noisy rgb", page), ("noisy grey", np.ascontiguousarray(page[:, :, 1])),
                      ("clean rgb", ((page >= 128) * 255).astype(np.uint8)), ("clean grey", ((page[:, :, 1] >= 128) * 255).astype(np.uint8))):
        e = ref(PAGE) if name == "noisy rgb" else pngenc_ref.encode(img)
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        rle = len(co.compress(e.stream.tobytes()) + co.flush())
        ours = len(e.deflate) + 6
        print(name, "idat", ours, "z_rle", rle, "blocks", len(e.blocks))
        assert ours <= rle + SIZE_MARGIN_PER_BLOCK * len(e.blocks), (name, ours, rle, len(e.blocks))
