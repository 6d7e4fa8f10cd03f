"""Baseline JPEG encoding in NumPy / plain Python, written from the rules of include/ocrvi.h ("JPEG encode"): quantisation tables for a
quality, colour conversion, 4:2:0 down-sampling, the 8 x 8 slow-integer forward DCT, quantisation, dummy blocks, Huffman coding with the
four Annex K tables, byte stuffing and the file header.  It is the reference of tests/test_jpeg_encode_cpu.py and
tests/test_gpu_jpeg_encode.py and shares no code with the C++ entries or the kernels.  Slow (the entropy coder is a Python loop).

    quant_tables(q)                     -> (luma, chroma) int64 [64], natural (row-major) order
    header(h, w, nc, sub, q)            -> the bytes SOI .. SOS
    encode(image, q, sub)               -> Encoded: .data (the whole file), .scan (the stuffed scan), .unstuffed (before stuffing),
                                           .coef int32 [blocks, 64] (quantised, zigzag order, scan block order; the DC is the absolute value,
                                           for a dummy block the value it inherits), .dummy bool [blocks], .bits int64 [blocks]
                                           (the bits each block adds to the scan), .comp int [blocks]
"""
from __future__ import annotations

import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                     72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                      + [99] * 32, np.int64)
# Annex K.3: (the number of codes of each length 1..16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
            0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
            0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
            0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
            0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
            0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
            0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
              0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
              0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
              0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
              0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
              0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
              0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
              0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
SUBSAMPLINGS = ("4:2:0", "4:4:4")


class Encoded:
    pass


def quant_tables(q: int):
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA))


def _codes(spec):
    """symbol -> (code, length), Annex C."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def header(h: int, w: int, nc: int, sub: str, q: int) -> bytes:
    ql, qc = quant_tables(q)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, t in enumerate((ql, qc)[:1 if nc == 1 else 2]):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(v) for v in t[ZIGZAG])
    comps = [(1, 0x22 if (nc == 3 and sub == "4:2:0") else 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)][:nc]
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * nc, 8, h, w, nc) + b"".join(bytes(c) for c in comps)
    for cls_id, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))[:2 if nc == 1 else 4]:
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(spec[1]), cls_id) + bytes(spec[0]) + bytes(spec[1])
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc) + b"".join(bytes([i + 1, 0x00 if i == 0 else 0x11]) for i in range(nc)) + b"\x00\x3f\x00"
    return out


def _fdct_pass(d, first: bool):
    """One pass over the LAST axis of int64 [..., 8]."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15
    r = 1 << (sh - 1)
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o[2] = (z1 + t13 * 6270 + r) >> sh
    o[6] = (z1 - t12 * 15137 + r) >> sh
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7] = (t4 + z1 + z3 + r) >> sh
    o[5] = (t5 + z2 + z4 + r) >> sh
    o[3] = (t6 + z2 + z3 + r) >> sh
    o[1] = (t7 + z1 + z4 + r) >> sh
    return np.stack(o, axis=-1)


def fdct_quant(blocks, table):
    """uint8-valued [..., 8, 8] samples, table int64 [64] natural order -> int64 [..., 64] quantised coefficients, natural order."""
    a = _fdct_pass(blocks.astype(np.int64) - 128, True)                   # along rows
    c = np.swapaxes(_fdct_pass(np.swapaxes(a, -1, -2), False), -1, -2)    # down columns
    c = c.reshape(c.shape[:-2] + (64,))
    d = 8 * table
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def _planes(image, sub):
    """The component planes, each padded by replication to whole blocks (only real blocks)."""
    img = np.asarray(image)
    if img.ndim == 2:
        comps = [img.astype(np.int64)]
    else:
        r, g, b = (img[..., i].astype(np.int64) for i in range(3))
        comps = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                 (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                 (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16]
    h, w = img.shape[:2]
    out = []
    for i, p in enumerate(comps):
        if i > 0 and sub == "4:2:0":
            ch, cw = (h + 1) // 2, (w + 1) // 2
            bh, bw = (ch + 7) // 8 * 8, (cw + 7) // 8 * 8
            # columns are replicated at full resolution, then down-sampled; of the rows only the one an odd height lacks is replicated at
            # full resolution, and the chroma rows below the last real one repeat that down-sampled row
            full = np.pad(p, ((0, 2 * ch - h), (0, 2 * bw - w)), mode="edge")
            bias = np.where(np.arange(bw) % 2 == 0, 1, 2)[None, :]
            p = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
            p = np.pad(p, ((0, bh - ch), (0, 0)), mode="edge")
        else:
            p = np.pad(p, ((0, -h % 8), (0, -w % 8)), mode="edge")
        out.append(p)
    return out


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def encode(image, quality: int = 95, sub: str = "4:2:0") -> Encoded:
    img = np.asarray(image)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)) and sub in SUBSAMPLINGS
    h, w = img.shape[:2]
    nc = 1 if img.ndim == 2 else 3
    ql, qc = quant_tables(quality)
    planes = _planes(img, sub)
    hs = 2 if (nc == 3 and sub == "4:2:0") else 1
    mx, my = -(-w // (8 * hs)), -(-h // (8 * hs))
    coefs, comp_of, dummy = [], [], []
    # every real block of every plane at once: [block rows, block columns, 64] in zigzag order
    zz = [fdct_quant(p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2), ql if c == 0 else qc)[..., ZIGZAG] for c, p in enumerate(planes)]

    def real(c, by, bx):
        return zz[c][by, bx] if by < zz[c].shape[0] and bx < zz[c].shape[1] else None

    for y in range(my):
        for x in range(mx):
            order = [(0, y * hs + j, x * hs + i) for j in range(hs) for i in range(hs)] + ([(1, y, x), (2, y, x)] if nc == 3 else [])
            for c, by, bx in order:
                v = real(c, by, bx)
                if v is None:                          # a dummy block: no AC, the DC of the block coded just before it in this MCU
                    v = np.zeros(64, np.int64)
                    v[0] = coefs[-1][0]
                    dummy.append(True)
                else:
                    dummy.append(False)
                coefs.append(v)
                comp_of.append(c)
    dc_t = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac_t = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    acc, held, nbits, bits_per_block = 0, 0, 0, []      # `held` bits wait in `acc` for a whole byte
    stream = bytearray()
    pred = [0, 0, 0]

    def put(code, ln):
        nonlocal acc, held, nbits
        acc = (acc << ln) | code
        held += ln
        nbits += ln
        while held >= 8:
            held -= 8
            stream.append(acc >> held)
            acc &= (1 << held) - 1

    for v, c in zip((b.tolist() for b in coefs), comp_of):
        start = nbits
        t = 0 if c == 0 else 1
        diff = int(v[0]) - pred[c]
        pred[c] = int(v[0])
        s = _category(diff)
        put(*dc_t[t][s])
        if s:
            put((diff if diff > 0 else diff - 1) & ((1 << s) - 1), s)
        run = 0
        for k in range(1, 64):
            x = int(v[k])
            if x == 0:
                run += 1
                continue
            while run > 15:
                put(*ac_t[t][0xF0])
                run -= 16
            s = _category(x)
            assert s <= 10
            put(*ac_t[t][(run << 4) | s])
            put((x if x > 0 else x - 1) & ((1 << s) - 1), s)
            run = 0
        if run:
            put(*ac_t[t][0x00])
        bits_per_block.append(nbits - start)
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    e = Encoded()
    assert held == 0 and len(stream) * 8 == nbits
    e.unstuffed = bytes(stream)
    e.scan = e.unstuffed.replace(b"\xff", b"\xff\x00")
    e.header = header(h, w, nc, sub, quality)
    e.data = e.header + e.scan + b"\xff\xd9"
    e.coef = np.array(coefs, np.int32).reshape(-1, 64)
    e.dummy = np.array(dummy, bool)
    e.bits = np.array(bits_per_block, np.int64)
    e.comp = np.array(comp_of)
    e.mcus = (my, mx)
    return e
