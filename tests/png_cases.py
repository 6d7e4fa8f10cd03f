"""A small PNG writer for the tests (stdlib ``zlib`` + NumPy) that takes the filter of every row explicitly, can split IDAT at chosen
sizes, pick the zlib level (0 gives stored blocks) or fixed Huffman codes, and add ancillary chunks; plus the hand-built streams the
kernel tests feed to ``ocrvi_png_decode_pages`` without any zlib in the way."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# all 15 legal pairs of (colour type, bit depth)
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
# a cyclic sequence over 0..4 in which every ordered pair (previous row's filter, this row's filter) occurs once: 25 + 1 rows
FILTER_PAIRS = [0, 0, 1, 0, 2, 0, 3, 0, 4, 1, 1, 2, 1, 3, 1, 4, 2, 2, 3, 2, 4, 3, 3, 4, 4, 0]


def chunk(typ: bytes, body: bytes = b"", crc: int = None) -> bytes:
    c = zlib.crc32(typ + body) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", c)


def ihdr(width, height, depth, colour, compression=0, filter_method=0, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, compression, filter_method, interlace))


def random_samples(rng, height, width, colour, depth) -> np.ndarray:
    """Random samples [H, W, channels], each below 2 ** depth."""
    return rng.integers(0, 1 << depth, (height, width, CHANNELS[colour]), dtype=np.int64)


def pack_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """Samples [H, W, channels] -> the unfiltered bytes of each row, uint8 [H, row_bytes]: most significant bit first, pad bits 0."""
    h = samples.shape[0]
    flat = samples.reshape(h, -1)
    if depth == 16:
        return np.stack([flat >> 8, flat & 255], axis=2).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    bits = ((flat[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8)
    return np.packbits(bits, axis=1)


def filter_rows(rows: np.ndarray, bpp: int, filters) -> np.ndarray:
    """Unfiltered bytes [H, row_bytes] -> filtered rows with their filter bytes, uint8 [H, 1 + row_bytes] (the PNG specification's
    forward filters: the inverse of tests/png_ref.py's ``unfilter``)."""
    h, n = rows.shape
    r = np.zeros((h + 1, n + bpp), np.int64)
    r[1:, bpp:] = rows
    out = np.zeros((h, 1 + n), np.uint8)
    for y in range(h):
        ft = int(filters[y])
        x, a, b, c = r[y + 1, bpp:], r[y + 1, :n], r[y, bpp:], r[y, :n]
        if ft == 0:
            p = 0
        elif ft == 1:
            p = a
        elif ft == 2:
            p = b
        elif ft == 3:
            p = (a + b) >> 1
        else:
            q = a + b - c
            pa, pb, pc = np.abs(q - a), np.abs(q - b), np.abs(q - c)
            p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[y, 0] = ft
        out[y, 1:] = (x - p) & 255
    return out


def deflate(raw: bytes, level: int = 6, fixed: bool = False) -> bytes:
    if fixed:
        co = zlib.compressobj(level or 6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        return co.compress(raw) + co.flush()
    return zlib.compress(raw, level)


def idat_chunks(z: bytes, split=None, empty_between: bool = False) -> bytes:
    """The zlib stream as IDAT chunks of ``split`` bytes each (None: one chunk), optionally with an empty IDAT after every one."""
    parts = [z] if not split else [z[i:i + split] for i in range(0, len(z), split)]
    out = b""
    for p in parts:
        out += chunk(b"IDAT", p)
        if empty_between:
            out += chunk(b"IDAT", b"")
    return out


def write_png(samples: np.ndarray, colour: int, depth: int, filters, palette: np.ndarray = None, level: int = 6, fixed: bool = False,
              split=None, empty_between: bool = False, before_idat: bytes = b"", after_idat: bytes = b"") -> bytes:
    """Samples [H, W, channels] -> a PNG file with row y filtered by ``filters[y]``.  palette: uint8 [n, 3] for colour type 3.
    ``before_idat`` / ``after_idat``: ready-made chunks (ancillary ones, say) placed there."""
    h, w = samples.shape[:2]
    bpp = max(1, CHANNELS[colour] * depth // 8)
    rows = filter_rows(pack_rows(samples, depth), bpp, filters)
    plte = chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()) if colour == 3 else b""
    return (SIGNATURE + ihdr(w, h, depth, colour) + plte + before_idat + idat_chunks(deflate(rows.tobytes(), level, fixed), split, empty_between)
            + after_idat + chunk(b"IEND"))


def hand_stream(rows: np.ndarray, palette: np.ndarray = None) -> bytes:
    """Filtered rows [H, 1 + row_bytes] (+ a palette [n, 3]) -> the page's stream of include/ocrvi.h, no zlib involved."""
    head = b""
    if palette is not None:
        pal = np.zeros((256, 4), np.uint8)
        pal[:len(palette), :3] = palette
        head = pal.tobytes()
    return head + np.ascontiguousarray(rows, np.uint8).tobytes()


# (a, b, c) = (left, above, above-left) that Paeth resolves as: the outcome a, the outcome b, the outcome c, the tie |q-a| == |q-c| (a wins
# over c) and the tie |q-b| == |q-c| (b wins over c)
PAETH_TRIPLES = np.array([(150, 101, 100), (101, 150, 100), (120, 80, 100), (80, 110, 100), (110, 80, 100)])


def paeth_rows():
    """-> (grey 8-bit samples [2 * 5, 2, 1], filters): for each (a, b, c) of ``PAETH_TRIPLES`` two rows [c, b] / [a, x], the second one
    Paeth-filtered, so its second byte is predicted from exactly that triple."""
    samples = np.zeros((2 * len(PAETH_TRIPLES), 2, 1), np.int64)
    filters = []
    for k, (a, b, c) in enumerate(PAETH_TRIPLES):
        samples[2 * k, :, 0] = (c, b)
        samples[2 * k + 1, :, 0] = (a, (37 * k + 11) & 255)
        filters += [0, 4]
    return samples, filters
