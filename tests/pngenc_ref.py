"""An independent NumPy / Python restatement of the PNG encoder's arithmetic (include/ocrvi.h, "PNG encode"), stage by stage: filter
bytes and filtered stream, tokens and histograms, code lengths, block types, bit offsets, Adler-32, CRC-32 and the file.  Nothing here
calls zlib: the tests use zlib to check what this module writes.

  filters     bpp = components; x = the raw byte, a = the raw byte bpp to the left, b = the raw byte above, c = the raw byte above-left
              (each 0 outside the row or the image); filtered byte = (x - p) & 255 with p = 0, a, b, (a + b) >> 1 or Paeth(a, b, c) for
              filters 0 .. 4.  Paeth: q = a + b - c; a if |q - a| <= |q - b| and |q - a| <= |q - c|; else b if |q - b| <= |q - c|; else c
  adaptive    cost of a filter = the sum of min(v, 256 - v) over the row's filtered bytes (the filter byte is not counted); the smallest
              cost wins, ties go to the lower filter number
  stream      h x (1 + row_bytes) bytes, every row led by its filter byte; row_bytes = width x components
  blocks      the stream is cut into deflate blocks of BLOCK = 16384 bytes (the last may be shorter)
  eq          eq[i] = i > 0 and s[i] == s[i - 1] over the whole stream; inside a block a RUN is a maximal set of consecutive positions
              with eq = 1 (it ends at the block's end; a block whose first byte has eq = 1 begins with a run)
  tokens      a byte with eq = 0 is a literal.  A run of L bytes is floor(L / 258) matches of length 258 at distance 1, then its
              remainder r = L mod 258: one match of length r when r >= 3, else r literals
  codes       per block, counts of the literal / length symbols 0..285 (the end-of-block symbol 256 counted once).  Code lengths from
              counts: a symbol of count 0 gets length 0; when fewer than two symbols have a count, the lowest-numbered symbols of count 0
              are given count 1 until two have; the m used symbols are sorted by (count, symbol) ascending; a Huffman tree is built from
              two queues (the sorted leaves, and the internal nodes in the order they are made), always taking the lighter head, the
              leaf on a tie; n[l] = the leaves at depth l, depths above the limit counted at the limit; while the sum of n[l] 2^(limit - l)
              exceeds 2^limit: n[limit] -= 1, then for the largest l < limit with n[l] > 0: n[l] -= 1, n[l + 1] += 2; finally lengths are
              dealt out along the sorted list, n[limit] symbols get the limit, the next n[limit - 1] get limit - 1, and so on.  The codes
              are canonical (RFC 1951, 3.2.2).  Limit 15 for literal / length codes, 7 for the code-length code
  dynamic     HLIT = max(257, 1 + the last literal / length symbol used); HDIST = 2, both distance lengths 1; the HLIT + 2 lengths,
              taken as one sequence, are cut into maximal runs of equal values.  A run of zeros: repeatedly take c = min(left, 138): symbol
              18 (c - 11 in 7 bits) when c >= 11, symbol 17 (c - 3 in 3 bits) when c >= 3, else c symbols 0.  A run of v > 0: symbol v,
              then repeatedly c = min(left, 6): symbol 16 (c - 3 in 2 bits) while left >= 3, then the rest as symbols v.  HCLEN = max(4,
              1 + the last position used in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15)
  block type  bits of a block as stored (3 + padding to a byte at its position + 32 + 8 n), fixed (3 + RFC 1951's fixed codes; a
              match costs its length code, extra bits and 5) and dynamic (3 + 14 + 3 HCLEN + the code-length symbols + the tokens; a
              match costs its length code, extra bits and 1); the smallest wins, ties go to the earlier of stored, fixed, dynamic
  file        signature, IHDR (depth 8, colour type 2 or 0, no interlace), one IDAT = 78 01 + the blocks + Adler-32 of the stream, IEND
"""
import struct
from dataclasses import dataclass, field

import numpy as np

BLOCK = 16384
ADLER = 65521
POLY = 0xEDB88320
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2

# length 3..258 -> (symbol, extra bits, extra value)
LEN_SYM = np.zeros((259, 3), np.int64)
for _k, (_b, _e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
    for _l in range(_b, min(_b + (1 << _e), 259)):
        if _l < 258 or _k == 28:
            LEN_SYM[_l] = (257 + _k, _e, _l - _b)
FIXED_LEN = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, np.int64)


@dataclass
class Rules:
    """The rules a mutant changes (tests/test_png_encode_cpu.py); the defaults are the library's."""
    tie_lower: bool = True           # adaptive: ties go to the lower filter number
    split: int = 258                 # the longest match
    min_rem: int = 3                 # the shortest remainder coded as a match
    cross_block: bool = True         # a run continues from the previous block
    type_tie_earlier: bool = True    # block type: ties go to the earlier of stored, fixed, dynamic
    pad_counts_header: bool = True   # a stored block's padding follows its 3 header bits


DEFAULT = Rules()


def paeth(a, b, c):
    q = a + b - c
    pa, pb, pc = np.abs(q - a), np.abs(q - b), np.abs(q - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_stream(img: np.ndarray, mode: str = "adaptive", rules: Rules = DEFAULT):
    """uint8 [h, w] or [h, w, 3] -> (filter of every row uint8 [h], the filtered stream uint8 [h, 1 + row_bytes])."""
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else 3
    n = w * bpp
    r = np.zeros((h + 1, n + bpp), np.int64)
    r[1:, bpp:] = img.reshape(h, n)
    x, a, b, c = r[1:, bpp:], r[1:, :n], r[:-1, bpp:], r[:-1, :n]
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth(a, b, c)]) & 255           # [5, h, n]
    if FILTERS[mode] < 5:
        ft = np.full(h, FILTERS[mode], np.int64)
    else:
        cost = np.minimum(cand, 256 - cand).sum(axis=2)                                         # [5, h]
        ft = np.argmin(cost, axis=0) if rules.tie_lower else 4 - np.argmin(cost[::-1], axis=0)
    out = np.zeros((h, 1 + n), np.uint8)
    out[:, 0] = ft
    out[:, 1:] = cand[ft, np.arange(h)]
    return ft.astype(np.uint8), out


def block_tokens(s: np.ndarray, lo: int, hi: int, rules: Rules = DEFAULT):
    """The tokens of block s[lo:hi] -> (positions inside the block, lengths): length 0 is the literal at that position, otherwise a
    match of that length at distance 1."""
    n = hi - lo
    blk = s[lo:hi]
    eq = np.zeros(n, bool)
    eq[1:] = blk[1:] == blk[:-1]
    eq[0] = rules.cross_block and lo > 0 and s[lo] == s[lo - 1]
    idx = np.arange(n)
    a = np.maximum.accumulate(np.where(~eq, idx, -1)) + 1                     # where the run a position lies in starts
    e = np.minimum.accumulate(np.where(~eq, idx, n)[::-1])[::-1]              # where it ends
    j, run = idx - a, e - a
    full = run // rules.split * rules.split
    rem = run - full
    m258 = eq & (j < full) & (j % rules.split == 0)
    mrem = eq & (j == full) & (rem >= rules.min_rem)
    lit = ~eq | (eq & (j >= full) & (rem < rules.min_rem))
    length = np.where(m258, rules.split, np.where(mrem, rem, 0))
    keep = m258 | mrem | lit
    return idx[keep], length[keep]


def histogram(blk: np.ndarray, pos: np.ndarray, length: np.ndarray) -> np.ndarray:
    """Counts of symbols 0..285, then [286] the matches (= the count of distance symbol 0) and [287] zero."""
    hist = np.zeros(288, np.int64)
    lit = length == 0
    hist[:256] = np.bincount(blk[pos[lit]], minlength=256)
    hist[256] = 1
    hist[:286] += np.bincount(LEN_SYM[length[~lit], 0], minlength=286)[:286] if (~lit).any() else 0
    hist[286] = int((~lit).sum())
    return hist


def code_lengths(counts, limit: int) -> np.ndarray:
    """The length-limited code of the module's docstring: counts [n] -> lengths uint8 [n]."""
    cnt = [int(v) for v in counts]
    n = len(cnt)
    s = 0
    while sum(1 for v in cnt if v) < 2:
        if cnt[s] == 0:
            cnt[s] = 1
        s += 1
    order = sorted((v, i) for i, v in enumerate(cnt) if v)
    m = len(order)
    weight = [v for v, _ in order]
    parent = [0] * (2 * m - 1)
    li, ni = 0, m
    for node in range(m, 2 * m - 1):
        picks = []
        for _ in range(2):
            if li < m and (ni >= node or weight[li] <= weight[ni]):
                picks.append(li)
                li += 1
            else:
                picks.append(ni)
                ni += 1
        weight.append(weight[picks[0]] + weight[picks[1]])
        parent[picks[0]] = parent[picks[1]] = node
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    nl = [0] * (limit + 1)
    for leaf in range(m):
        nl[min(depth[leaf], limit)] += 1
    total = sum(nl[k] << (limit - k) for k in range(1, limit + 1))
    while total > (1 << limit):
        nl[limit] -= 1
        for k in range(limit - 1, 0, -1):
            if nl[k]:
                nl[k] -= 1
                nl[k + 1] += 2
                break
        total -= 1
    out = np.zeros(n, np.uint8)
    k = 0
    for bits in range(limit, 0, -1):
        for _ in range(nl[bits]):
            out[order[k][1]] = bits
            k += 1
    return out


def canonical_codes(lengths) -> np.ndarray:
    """RFC 1951 3.2.2, each code bit-reversed (deflate sends Huffman codes most significant bit first into an LSB-first stream)."""
    lengths = [int(v) for v in lengths]
    count = [0] * 17
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = np.zeros(len(lengths), np.int64)
    for i, v in enumerate(lengths):
        if v:
            out[i] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


def cl_tokens(seq):
    """The run-length coding of a sequence of code lengths -> [(symbol, extra value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, k = seq[i], i
        while k < n and seq[k] == v:
            k += 1
        left = k - i
        i = k
        if v == 0:
            while left:
                c = min(left, 138)
                if c >= 11:
                    out.append((18, c - 11))
                elif c >= 3:
                    out.append((17, c - 3))
                else:
                    out += [(0, 0)] * c
                left -= c
        else:
            out.append((v, 0))
            left -= 1
            while left >= 3:
                c = min(left, 6)
                out.append((16, c - 3))
                left -= c
            out += [(v, 0)] * left
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


@dataclass
class Block:
    lo: int
    hi: int
    pos: np.ndarray
    length: np.ndarray
    hist: np.ndarray
    lens: np.ndarray                 # 286 literal / length code lengths
    cl_lens: np.ndarray              # 19 code-length code lengths
    cl_tok: list
    hlit: int
    hclen: int
    fixed_bits: int
    dynamic_bits: int
    adler_a: int                     # sum of the block's bytes mod 65521
    adler_b: int                     # sum of (n - i) x byte i mod 65521
    type: int = -1
    bit_offset: int = 0


@dataclass
class Encoded:
    filters: np.ndarray
    stream: np.ndarray               # uint8, flat
    blocks: list = field(default_factory=list)
    bit_offsets: list = field(default_factory=list)     # of every block, and the end
    adler: int = 1
    crc: int = 0
    deflate: bytes = b""
    data: bytes = b""


def analyse_block(s, lo, hi, rules=DEFAULT) -> Block:
    pos, length = block_tokens(s, lo, hi, rules)
    blk = s[lo:hi]
    hist = histogram(blk, pos, length)
    lens = code_lengths(hist[:286], 15)
    hlit = max(257, int(np.flatnonzero(lens)[-1]) + 1)
    tok = cl_tokens([int(v) for v in lens[:hlit]] + [1, 1])
    cl_hist = np.bincount([t[0] for t in tok], minlength=19)
    cl_lens = code_lengths(cl_hist, 7)
    hclen = max(4, max(k for k, sym in enumerate(CL_ORDER) if cl_lens[sym]) + 1)
    extra = np.zeros(286, np.int64)
    extra[257:286] = LEN_EXTRA
    body = hist[:286]
    fixed_bits = 3 + int((body * (FIXED_LEN[:286] + extra)).sum()) + 5 * int(hist[286])
    dynamic_bits = (3 + 14 + 3 * hclen + sum(int(cl_lens[t]) + CL_EXTRA.get(t, 0) for t, _ in tok)
                    + int((body * (lens.astype(np.int64) + extra)).sum()) + int(hist[286]))
    n = hi - lo
    b64 = blk.astype(np.int64)
    return Block(lo, hi, pos, length, hist, lens, cl_lens, tok, hlit, hclen, fixed_bits, dynamic_bits, int(b64.sum() % ADLER),
                 int((b64 * (n - np.arange(n))).sum() % ADLER))


def stored_bits(pos: int, n: int, rules=DEFAULT) -> int:
    pad = (-(pos + 3)) % 8 if rules.pad_counts_header else (-pos) % 8
    return 3 + pad + 32 + 8 * n


def pack_fields(vals, nbits) -> np.ndarray:
    """Fields (value, bits), each least significant bit first -> the bits, uint8 0 / 1."""
    vals, nbits = np.asarray(vals, np.int64), np.asarray(nbits, np.int64)
    keep = nbits > 0
    vals, nbits = vals[keep], nbits[keep]
    offs = np.cumsum(nbits) - nbits
    total = int(nbits.sum())
    k = np.arange(total) - np.repeat(offs, nbits)
    return ((np.repeat(vals, nbits) >> k) & 1).astype(np.uint8)


def block_bits(s, b: Block, final: bool, rules=DEFAULT) -> np.ndarray:
    n = b.hi - b.lo
    if b.type == STORED:
        pad = stored_bits(b.bit_offset, n, rules) - 35 - 8 * n
        head = pack_fields([int(final), 0, 0, n, n ^ 0xFFFF], [1, 2, pad, 16, 16])
        return np.concatenate([head, np.unpackbits(s[b.lo:b.hi], bitorder="little")])
    if b.type == FIXED:
        lens, head_v, head_n = FIXED_LEN, [int(final), 1], [1, 2]
        dist_v, dist_n = 0, 5
    else:
        lens = np.concatenate([b.lens, [0, 0]]).astype(np.int64)
        cl_codes = canonical_codes(b.cl_lens)
        head_v, head_n = [int(final), 2, b.hlit - 257, 1, b.hclen - 4], [1, 2, 5, 5, 4]
        for sym in CL_ORDER[:b.hclen]:
            head_v.append(int(b.cl_lens[sym]))
            head_n.append(3)
        for sym, ev in b.cl_tok:
            head_v += [int(cl_codes[sym]), ev]
            head_n += [int(b.cl_lens[sym]), CL_EXTRA.get(sym, 0)]
        dist_v, dist_n = 0, 1
    codes = canonical_codes(lens)
    blk = s[b.lo:b.hi]
    lit = b.length == 0
    sym = np.where(lit, blk[b.pos], LEN_SYM[b.length, 0])
    t = len(sym)
    vals, bits = np.zeros((t, 3), np.int64), np.zeros((t, 3), np.int64)
    vals[:, 0], bits[:, 0] = codes[sym], lens[sym]
    vals[:, 1], bits[:, 1] = np.where(lit, 0, LEN_SYM[b.length, 2]), np.where(lit, 0, LEN_SYM[b.length, 1])
    vals[:, 2], bits[:, 2] = dist_v, np.where(lit, 0, dist_n)
    return np.concatenate([pack_fields(head_v, head_n), pack_fields(vals.reshape(-1), bits.reshape(-1)),
                           pack_fields([codes[256]], [lens[256]])])


def crc_table():
    t = np.zeros(256, np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        t[i] = c
    return t


_CRC_TABLE = crc_table()


def crc_raw(data: bytes, crc: int = 0) -> int:
    """The CRC register after ``data``, no initial or final inversion."""
    for v in data:
        crc = int(_CRC_TABLE[(crc ^ v) & 255]) ^ (crc >> 8)
    return crc


def crc_mul(a: int, b: int) -> int:
    """The product of two polynomials mod the CRC polynomial, reflected: bit 31 is x^0."""
    r = 0
    for i in range(32):
        if a & (1 << (31 - i)):
            r ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return r


def crc_xpow8(n: int) -> int:
    """x^(8 n) mod the CRC polynomial."""
    r, base = 0x80000000, 0x00800000
    while n:
        if n & 1:
            r = crc_mul(r, base)
        base = crc_mul(base, base)
        n >>= 1
    return r


def crc32_segments(data: bytes, first: int = 0, seg: int = 4096):
    """CRC-32 the way the device computes it: raw partials of the segments [k seg, (k + 1) seg) of the FILE (``data`` starts at file
    offset ``first``), the first four bytes inverted, each partial multiplied by x^(8 x the bytes after it), XORed, inverted."""
    d = bytearray(data)
    for k in range(4):
        d[k] ^= 0xFF
    cuts = [0] + list(range(seg - first % seg, len(d), seg)) + [len(d)]
    parts = [crc_raw(bytes(d[a:b])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    ends = [b for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    total = 0
    for p, e in zip(parts, ends):
        total ^= crc_mul(p, crc_xpow8(len(d) - e))
    return total ^ 0xFFFFFFFF, parts


def chunk(typ: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", crc32_segments(typ + body)[0])


def header(h: int, w: int, components: int) -> bytes:
    """The 33 constant bytes: signature and IHDR."""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if components == 3 else 0, 0, 0, 0))


def sizes(h: int, w: int, components: int) -> dict:
    stream = h * (1 + w * components)
    blocks = -(-stream // BLOCK)
    return {"stream_bytes": stream, "blocks": blocks, "capacity": 33 + 12 + 2 + 5 * blocks + stream + 4 + 12}


def encode(img: np.ndarray, mode: str = "adaptive", rules: Rules = DEFAULT) -> Encoded:
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    h, w = img.shape[:2]
    ft, rows = filter_stream(img, mode, rules)
    s = rows.reshape(-1)
    e = Encoded(ft, s)
    pos, a1, a2, bits = 0, 1, 0, []
    nb = -(-len(s) // BLOCK)
    for k in range(nb):
        lo, hi = k * BLOCK, min(len(s), (k + 1) * BLOCK)
        b = analyse_block(s, lo, hi, rules)
        cost = [stored_bits(pos, hi - lo, rules), b.fixed_bits, b.dynamic_bits]
        b.type = int(np.argmin(cost)) if rules.type_tie_earlier else 2 - int(np.argmin(cost[::-1]))
        b.bit_offset = pos
        e.bit_offsets.append(pos)
        bb = block_bits(s, b, k == nb - 1, rules)
        assert len(bb) == cost[b.type] or not rules.pad_counts_header, (k, len(bb), cost)
        bits.append(bb)
        pos += len(bb)
        a2 = (a2 + (hi - lo) * a1 + b.adler_b) % ADLER
        a1 = (a1 + b.adler_a) % ADLER
        e.blocks.append(b)
    e.bit_offsets.append(pos)
    e.adler = (a2 << 16) | a1
    e.deflate = np.packbits(np.concatenate(bits), bitorder="little").tobytes()
    body = b"\x78\x01" + e.deflate + struct.pack(">I", e.adler)
    e.crc = crc32_segments(b"IDAT" + body, 37)[0]
    e.data = header(h, w, 1 if img.ndim == 2 else 3) + struct.pack(">I", len(body)) + b"IDAT" + body + struct.pack(">I", e.crc) + chunk(b"IEND", b"")
    return e
