"""Baseline JPEG in NumPy / plain Python, written from the rules of include/ocrvi.h ("JPEG decode"): marker parse, Huffman decode,
dequantisation, the 8 x 8 slow-integer inverse DCT, chroma upsampling, colour conversion, EXIF orientation.  It is the reference of
tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py and shares no code with the C++ parser or the kernels.  Slow (the entropy decoder is a
Python loop): meant for files of a few hundred pixels a side.

    info(data)    -> dict of what ocrvi_jpeg_info reports
    parse(data)   -> Parsed: header fields, per-component quantisation tables, `blocks` int32 [n_blocks, 64] -- the quantised
                     coefficients of every 8 x 8 block in the order the scan codes them, natural (row-major) positions
    decode(data)  -> uint8 [H', W', 3] RGB after the EXIF orientation
"""
from __future__ import annotations

import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SAT = 16384       # dequantised coefficients and pass-1 results are saturated to [-SAT, SAT - 1]


class JpegError(ValueError):
    """A corrupt or truncated file."""


class Unsupported(JpegError):
    """A well-formed file of a kind the library does not decode; str(e) names the feature."""


class Parsed:
    pass


def _exif_orientation(seg: bytes) -> int:
    if len(seg) < 14 or seg[:6] != b"Exif\0\0":
        return 1
    t = seg[6:]
    if t[:2] == b"II":
        e = "<"
    elif t[:2] == b"MM":
        e = ">"
    else:
        return 1
    if struct.unpack(e + "H", t[2:4])[0] != 42:
        return 1
    ifd = struct.unpack(e + "I", t[4:8])[0]
    if ifd + 2 > len(t):
        return 1
    n = struct.unpack(e + "H", t[ifd:ifd + 2])[0]
    for i in range(n):
        o = ifd + 2 + 12 * i
        if o + 12 > len(t):
            return 1
        tag, typ, cnt = struct.unpack(e + "HHI", t[o:o + 8])
        if tag == 0x0112:
            if typ != 3 or cnt != 1:
                return 1
            v = struct.unpack(e + "H", t[o + 8:o + 10])[0]
            return v if 1 <= v <= 8 else 1
    return 1


def _headers(data: bytes) -> Parsed:
    d = bytes(data)
    n = len(d)
    if n < 4 or d[:2] != b"\xff\xd8":
        raise JpegError("no SOI marker")
    h = Parsed()
    h.orientation, h.restart_interval = 1, 0
    h.qt, h.huff = {}, {}
    sof = None
    jfif, adobe = False, None
    p = 2
    while True:
        if p >= n or d[p] != 0xFF:
            raise JpegError("expected a marker")
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            raise JpegError("truncated marker")
        m = d[p]
        p += 1
        if m in (0xD8, 0xD9, 0x01, 0x00) or 0xD0 <= m <= 0xD7:
            raise JpegError(f"marker FF{m:02X} before SOS")
        if p + 2 > n:
            raise JpegError("truncated length")
        ln = (d[p] << 8) | d[p + 1]
        if ln < 2 or p + ln > n:
            raise JpegError("bad segment length")
        s = d[p + 2:p + ln]
        p += ln
        if m in (0xC0, 0xC1):
            if sof is not None or len(s) < 6:
                raise JpegError("bad SOF")
            if s[0] != 8:
                raise Unsupported(f"{s[0]}-bit precision")
            h.height, h.width, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if not (1 <= h.height <= 65500 and 1 <= h.width <= 65500):
                raise JpegError("bad dimensions")
            if nc == 4:
                raise Unsupported("4 components")
            if nc not in (1, 3) or len(s) != 6 + 3 * nc:
                raise JpegError("bad SOF")
            sof = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nc)]
            for _, hs, vs, tq in sof:
                if not (1 <= hs <= 4 and 1 <= vs <= 4) or tq > 3:
                    raise JpegError("bad SOF component")
            if nc == 1:
                sof = [(sof[0][0], 1, 1, sof[0][3])]
            elif (sof[0][1], sof[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any(c[1] != 1 or c[2] != 1 for c in sof[1:]):
                raise Unsupported("sampling factors")
        elif m == 0xC2:
            raise Unsupported("progressive")
        elif m in (0xC3, 0xC7, 0xCB, 0xCF):
            raise Unsupported("lossless")
        elif m in (0xC9, 0xCA, 0xCC, 0xCD, 0xCE):
            raise Unsupported("arithmetic coding")
        elif m in (0xC5, 0xC6):
            raise Unsupported("hierarchical")
        elif m == 0xDC:
            raise Unsupported("DNL")
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if len(s) - q < 17:
                    raise JpegError("bad DHT")
                tc, th = s[q] >> 4, s[q] & 15
                counts = list(s[q + 1:q + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or q + 17 + tot > len(s):
                    raise JpegError("bad DHT")
                codes, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        if code >= (1 << length):
                            raise JpegError("bad Huffman table")
                        codes[(length, code)] = s[q + 17 + k]
                        code += 1
                        k += 1
                    code <<= 1
                h.huff[(tc, th)] = codes
                q += 17 + tot
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tid = s[q] >> 4, s[q] & 15
                need = 1 + (128 if pq else 64)
                if pq > 1 or tid > 3 or len(s) - q < need:
                    raise JpegError("bad DQT")
                raw = np.frombuffer(s[q + 1:q + need], dtype=">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = raw
                h.qt[tid] = nat
                q += need
        elif m == 0xDD:
            if len(s) != 2:
                raise JpegError("bad DRI")
            h.restart_interval = (s[0] << 8) | s[1]
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xE1:
            if s[:6] == b"Exif\0\0":
                h.orientation = _exif_orientation(s)
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
        elif m == 0xDA:
            if sof is None or len(s) < 1:
                raise JpegError("bad SOS")
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) != 4 + 2 * ns:
                raise JpegError("bad SOS")
            if ns != len(sof):
                raise Unsupported("several scans")
            h.tabs = []
            for c in range(ns):
                if s[1 + 2 * c] != sof[c][0]:
                    raise JpegError("scan component mismatch")
                td, ta = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if (0, td) not in h.huff or (1, ta) not in h.huff or sof[c][3] not in h.qt:
                    raise JpegError("missing table")
                h.tabs.append((h.huff[(0, td)], h.huff[(1, ta)]))
            if tuple(s[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise JpegError("bad spectral selection")
            if ns == 3:
                if adobe == 0:
                    raise Unsupported("Adobe transform 0 (RGB)")
                if not jfif and bytes(c[0] for c in sof) == b"RGB":
                    raise Unsupported("component ids R, G, B without JFIF (RGB)")
            break
    h.ncomp = len(sof)
    h.hs, h.vs = sof[0][1], sof[0][2]
    h.h_samp = [c[1] for c in sof]
    h.v_samp = [c[2] for c in sof]
    h.quant = [h.qt[c[3]] for c in sof]
    h.mcus_x = -(-h.width // (8 * h.hs))
    h.mcus_y = -(-h.height // (8 * h.vs))
    h.blocks_per_mcu = 1 if h.ncomp == 1 else h.hs * h.vs + 2
    h.n_blocks = h.mcus_x * h.mcus_y * h.blocks_per_mcu
    if h.n_blocks > 4 * (n - p):
        raise JpegError("truncated")
    h.scan_pos = p
    swap = h.orientation >= 5
    h.out_height, h.out_width = (h.width, h.height) if swap else (h.height, h.width)
    return h


def info(data) -> dict:
    h = _headers(data)
    return {"width": h.width, "height": h.height, "components": h.ncomp, "h_samp": h.h_samp, "v_samp": h.v_samp,
            "restart_interval": h.restart_interval, "orientation": h.orientation, "out_height": h.out_height, "out_width": h.out_width,
            "blocks": h.n_blocks}


class _Bits:
    """The entropy-coded segment as a bit string, byte-unstuffed, up to the next marker."""

    def __init__(self, d: bytes, p: int):
        self.d, self.p = d, p
        self.acc, self.n = 0, 0

    def _byte(self) -> bool:
        d, p = self.d, self.p
        if p >= len(d):
            return False
        b = d[p]
        if b == 0xFF:
            if p + 1 >= len(d) or d[p + 1] != 0:
                return False
            self.p = p + 2
        else:
            self.p = p + 1
        self.acc = ((self.acc << 8) | b) & 0xFFFFFFFFFF
        self.n += 8
        return True

    def bit(self) -> int:
        if self.n == 0 and not self._byte():
            raise JpegError("truncated data")
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k: int) -> int:
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, codes) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = codes.get((length, code))
            if s is not None:
                return s
        raise JpegError("bad Huffman code")


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def parse(data) -> Parsed:
    d = bytes(data)
    h = _headers(d)
    blocks = np.zeros((h.n_blocks, 64), np.int32)
    br = _Bits(d, h.scan_pos)
    pred = [0, 0, 0]
    nl = 1 if h.ncomp == 1 else h.hs * h.vs
    b, rst = 0, 0
    for mcu in range(h.mcus_x * h.mcus_y):
        if h.restart_interval and mcu and mcu % h.restart_interval == 0:
            if br.n >= 8:
                raise JpegError("data where RSTn was expected")
            br.n = 0
            p = br.p
            if p >= len(d) or d[p] != 0xFF:
                raise JpegError("missing RSTn")
            while p < len(d) and d[p] == 0xFF:
                p += 1
            if p >= len(d) or d[p] != 0xD0 + rst:
                raise JpegError("misnumbered RSTn")
            br.p = p + 1
            rst = (rst + 1) & 7
            pred = [0, 0, 0]
        for k in range(h.blocks_per_mcu):
            c = 0 if k < nl else k - nl + 1
            dc_codes, ac_codes = h.tabs[c]
            s = br.symbol(dc_codes)
            if s > 15:
                raise JpegError("bad DC category")
            pred[c] += _extend(br.bits(s), s) if s else 0
            if not -32768 <= pred[c] <= 32767:
                raise JpegError("DC outside 16 bits")
            blocks[b, 0] = pred[c]
            i = 1
            while i < 64:
                rs = br.symbol(ac_codes)
                r, sz = rs >> 4, rs & 15
                if sz == 0:
                    if r == 15:
                        i += 16
                        if i > 63:
                            raise JpegError("run past 63")
                        continue
                    if r:
                        raise JpegError("EOBn in a sequential scan")
                    break
                i += r
                if i > 63:
                    raise JpegError("run past 63")
                blocks[b, ZIGZAG[i]] = _extend(br.bits(sz), sz)
                i += 1
            b += 1
    if br.n >= 8:
        raise JpegError("data after the last MCU")
    p = br.p
    if p >= len(d) or d[p] != 0xFF:
        raise JpegError("no EOI")
    while p < len(d) and d[p] == 0xFF:
        p += 1
    if p >= len(d):
        raise JpegError("no EOI")
    if d[p] != 0xD9:
        if d[p] in (0xDA, 0xC4, 0xDB, 0xDD):
            raise Unsupported("several scans")
        raise JpegError("expected EOI")
    h.blocks = blocks
    return h


def block_comp(h: Parsed) -> np.ndarray:
    """The component of every block of ``h.blocks``."""
    k = np.arange(h.n_blocks) % h.blocks_per_mcu
    nl = 1 if h.ncomp == 1 else h.hs * h.vs
    return np.where(k < nl, 0, k - nl + 1)


def _idct_pass(x, shift):
    """One pass of the slow-integer inverse DCT along axis -2 ... of eight inputs x[..., 0..7] (Python-width integers: object arrays are
    avoided by the saturation, every true value fits int64 with room to spare)."""
    x = x.astype(np.int64)
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """coef int [n, 64] quantised (natural order), quant int [n, 64] or [64] -> uint8 [n, 8, 8] samples."""
    dq = np.clip(coef.astype(np.int64) * quant.astype(np.int64), -SAT, SAT - 1).reshape(-1, 8, 8)
    # pass 1 down the columns: the eight inputs of column c are dq[:, 0..7, c]
    ws = np.clip(_idct_pass(dq.transpose(0, 2, 1), 11), -SAT, SAT - 1).transpose(0, 2, 1)      # [n, row, col]
    out = _idct_pass(ws, 18) + 128                                                             # along the rows
    return np.clip(out, 0, 255).astype(np.uint8)


def planes(h: Parsed):
    """The component planes, padded to whole MCUs, from h.blocks."""
    comp = block_comp(h)
    out = []
    for c in range(h.ncomp):
        hs, vs = (h.hs, h.vs) if c == 0 and h.ncomp == 3 else (1, 1)
        bw, bh = h.mcus_x * hs, h.mcus_y * vs
        idx = np.nonzero(comp == c)[0]
        px = idct_blocks(h.blocks[idx], h.quant[c])
        k = np.arange(len(idx))
        if h.ncomp == 1:
            bx, by = k % bw, k // bw
        else:
            mcu, r = k // (hs * vs), k % (hs * vs)
            bx, by = (mcu % h.mcus_x) * hs + r % hs, (mcu // h.mcus_x) * vs + r // hs
        plane = np.zeros((bh * 8, bw * 8), np.uint8)
        for j in range(len(idx)):
            plane[by[j] * 8:by[j] * 8 + 8, bx[j] * 8:bx[j] * 8 + 8] = px[j]
        out.append(plane)
    return out


def _up_h2(c: np.ndarray) -> np.ndarray:
    """4:2:2 rows: c int [rows, cw] -> [rows, 2 cw]."""
    c = c.astype(np.int64)
    cw = c.shape[1]
    out = np.empty((c.shape[0], 2 * cw), np.int64)
    if cw <= 2:                       # too narrow for the triangle filter: every sample twice
        out[:, 0::2] = c
        out[:, 1::2] = c
        return out
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0] = c[:, 0]
    out[:, -1] = c[:, -1]
    return out


def _up_h2v2(c: np.ndarray) -> np.ndarray:
    """4:2:0: c int [ch, cw] -> [2 ch, 2 cw]."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    t = np.empty((2 * ch, cw), np.int64)
    t[0::2] = 3 * c + above
    t[1::2] = 3 * c + below
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * t + left + 8) >> 4
    out[:, 1::2] = (3 * t + right + 7) >> 4
    out[:, 0] = (4 * t[:, 0] + 8) >> 4
    out[:, -1] = (4 * t[:, -1] + 7) >> 4
    return out


def orient(img: np.ndarray, k: int) -> np.ndarray:
    """EXIF orientation k as PIL.ImageOps.exif_transpose applies it."""
    if k == 2:
        return img[:, ::-1]
    if k == 3:
        return img[::-1, ::-1]
    if k == 4:
        return img[::-1]
    if k == 5:
        return img.transpose(1, 0, 2)
    if k == 6:
        return np.rot90(img, -1)
    if k == 7:
        return img[::-1, ::-1].transpose(1, 0, 2)
    if k == 8:
        return np.rot90(img, 1)
    return img


def decode(data) -> np.ndarray:
    h = parse(data)
    pl = planes(h)
    H, W = h.height, h.width
    y = pl[0][:H, :W].astype(np.int64)
    if h.ncomp == 1:
        rgb = np.stack([y, y, y], axis=-1)
    else:
        cw, ch = -(-W // h.hs), -(-H // h.vs)
        cc = []
        for c in (1, 2):
            p = pl[c][:ch, :cw]
            if (h.hs, h.vs) == (2, 1):
                p = _up_h2(p)
            elif (h.hs, h.vs) == (2, 2):
                p = _up_h2v2(p)
            cc.append(p[:H, :W].astype(np.int64) - 128)
        cb, cr = cc
        r = y + ((91881 * cr + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        rgb = np.stack([r, g, b], axis=-1)
    return np.ascontiguousarray(orient(np.clip(rgb, 0, 255).astype(np.uint8), h.orientation))
