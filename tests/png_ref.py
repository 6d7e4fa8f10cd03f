"""An independent reference PNG decoder for the tests: chunks parsed here, inflate by ``zlib.decompress``, the row filters undone and the
samples converted in NumPy, with the arithmetic include/ocrvi.h states ("PNG decode"):

  unfilter  bpp = max(1, channels * bit_depth / 8); a = the reconstructed byte bpp to the left, b = the byte above, c = the byte
            above-left (each 0 outside the row or the image); every reconstructed byte is (x + p) & 255 with p = 0, a, b, (a + b) >> 1 or
            Paeth for filter bytes 0 .. 4 (a filter byte above 4 counts as 0: the device's rule for a rewritten stream)
  Paeth     q = a + b - c; a if |q - a| <= |q - b| and |q - a| <= |q - c|; else b if |q - b| <= |q - c|; else c
  samples   packed most significant bit first; grey samples of depth 1, 2, 4 scale by 255, 85, 17; a 16-bit sample gives its high byte;
            grey goes to all three channels; palette index i gives palette row i, rows beyond the file's PLTE are (0, 0, 0); alpha is
            dropped; tRNS, gamma, colour profiles and the eXIf orientation are ignored
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
BAND_ROWS, CHUNK_BYTES = 256, 24


def chunks(data: bytes):
    """[(type, body)] up to IEND."""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while True:
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        out.append((typ, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
        if typ == b"IEND":
            return out


def info(data: bytes) -> dict:
    ch = chunks(data)
    w, h, depth, colour = struct.unpack(">IIBB", ch[0][1][:10])
    channels = CHANNELS[colour]
    row_bytes = (w * channels * depth + 7) // 8
    plte = [b for t, b in ch if t == b"PLTE"]
    idat = sum(len(b) for t, b in ch if t == b"IDAT")
    chunks_per_row = -(-row_bytes // CHUNK_BYTES)
    return {"width": w, "height": h, "bit_depth": depth, "colour_type": colour, "channels": channels, "row_bytes": row_bytes,
            "out_height": h, "out_width": w, "palette_entries": len(plte[0]) // 3 if colour == 3 and plte else 0, "idat_bytes": idat,
            "stream_bytes": (1024 if colour == 3 else 0) + h * (1 + row_bytes),
            "workspace_bytes": 0 if h <= BAND_ROWS else -(-chunks_per_row * CHUNK_BYTES // 256) * 256}


def plan(height: int, row_bytes: int) -> dict:
    """What ``ocrvi_png_plan`` reports: a band of r rows and c chunks takes c + r - 1 steps."""
    c = -(-row_bytes // CHUNK_BYTES)
    bands = -(-height // BAND_ROWS)
    steps = sum(c + min(BAND_ROWS, height - b * BAND_ROWS) - 1 for b in range(bands))
    return {"band_rows": BAND_ROWS, "chunk_bytes": CHUNK_BYTES, "bands": bands, "steps": steps}


def palette_block(plte: bytes) -> bytes:
    pal = np.zeros((256, 4), np.uint8)
    e = np.frombuffer(plte, np.uint8).reshape(-1, 3)
    pal[:len(e), :3] = e
    return pal.tobytes()


def stream(data: bytes) -> bytes:
    """The page's stream as ``ocrvi_png_parse`` writes it: [palette] + the inflated scanlines."""
    ch = chunks(data)
    i = info(data)
    z = b"".join(b for t, b in ch if t == b"IDAT")
    rows = zlib.decompressobj().decompress(z)
    assert len(rows) == i["height"] * (1 + i["row_bytes"])
    head = palette_block([b for t, b in ch if t == b"PLTE"][0]) if i["colour_type"] == 3 else b""
    return head + rows


def unfilter(rows: np.ndarray, bpp: int) -> np.ndarray:
    """rows: uint8 [H, 1 + row_bytes] (filter byte first) -> the reconstructed bytes, uint8 [H, row_bytes]."""
    h, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h + 1, n + bpp), np.int64)             # a row of zeros above, bpp zeros to the left
    for y in range(h):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        cur, up = out[y + 1], out[y]
        if ft == 0 or ft > 4:
            cur[bpp:] = x
        elif ft == 2:
            cur[bpp:] = (x + up[bpp:]) & 255
        elif ft == 1:                                       # a running sum along each of the bpp interleaved lanes
            for lane in range(bpp):
                cur[bpp + lane::bpp] = np.cumsum(x[lane::bpp]) & 255
        else:
            for i in range(n):
                a, b, c = int(cur[i]), int(up[bpp + i]), int(up[i])
                if ft == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[bpp + i] = (int(x[i]) + p) & 255
    return out[1:, bpp:].astype(np.uint8)


def convert(recon: np.ndarray, width: int, colour: int, depth: int, palette: np.ndarray = None) -> np.ndarray:
    """Reconstructed bytes [H, row_bytes] -> uint8 RGB [H, W, 3].  palette: uint8 [256, 4] (colour type 3)."""
    h = recon.shape[0]
    channels = CHANNELS[colour]
    if depth < 8:
        bits = np.unpackbits(recon, axis=1)[:, :width * depth].reshape(h, width, depth)      # most significant bit first
        v = np.zeros((h, width), np.int64)
        for k in range(depth):
            v = (v << 1) | bits[:, :, k]
        s = v[:, :, None]
        if colour == 0:
            s = s * {1: 255, 2: 85, 4: 17}[depth]
    elif depth == 8:
        s = recon[:, :width * channels].reshape(h, width, channels).astype(np.int64)
    else:
        s = recon[:, :width * channels * 2].reshape(h, width, channels, 2)[..., 0].astype(np.int64)   # the high byte
    if colour == 3:
        return palette[s[:, :, 0], :3].astype(np.uint8)
    if colour in (0, 4):
        return np.repeat(s[:, :, :1], 3, axis=2).astype(np.uint8)
    return s[:, :, :3].astype(np.uint8)


def decode_stream(stream_bytes: bytes, width: int, height: int, colour: int, depth: int) -> np.ndarray:
    """A page's stream (include/ocrvi.h) -> uint8 RGB [H, W, 3]: what ``ocrvi_png_decode_pages`` must write."""
    channels = CHANNELS[colour]
    row_bytes = (width * channels * depth + 7) // 8
    buf = np.frombuffer(stream_bytes, np.uint8)
    palette = None
    if colour == 3:
        palette, buf = buf[:1024].reshape(256, 4), buf[1024:]
    rows = buf.reshape(height, 1 + row_bytes)
    return convert(unfilter(rows, max(1, channels * depth // 8)), width, colour, depth, palette)


def decode(data: bytes) -> np.ndarray:
    i = info(data)
    return decode_stream(stream(data), i["width"], i["height"], i["colour_type"], i["bit_depth"])
