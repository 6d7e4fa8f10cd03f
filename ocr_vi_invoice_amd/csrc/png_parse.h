// PNG on the host: chunk walker, CRC-32, zlib header, inflate (stored, fixed and dynamic blocks), Adler-32 -> the page's stream of
// include/ocrvi.h ("PNG decode": an optional 1024-byte palette, then the filtered scanlines as the file holds them).  Plain C++17, no
// HIP, no zlib, no libpng: tools/png_parse_check.cpp includes this file alone.  The input is untrusted: every read goes through a bounds
// check, every loop consumes input or ends, and nothing is written outside the caller's buffer.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace ocrvi {
namespace png {

enum { P_OK = 0, P_EINVAL = -1, P_ENOMEM = -3 };   // the values of OCRVI_OK / OCRVI_EINVAL / OCRVI_ENOMEM
enum { kBandRows = 256, kChunkBytes = 24, kMaxSide = 65500, kPaletteBytes = 1024 };   // the kernel's plan (csrc/png.hip)

struct Header {
    int width = 0, height = 0, depth = 0, colour = 0, channels = 0;
    int palette_entries = 0;
    bool have_ihdr = false;
    uint8_t palette[kPaletteBytes];   // 256 x (R, G, B, 0)
    size_t first_idat = 0;            // offset of the first IDAT chunk (its length field)
    int idat_chunks = 0;
    uint64_t idat_bytes = 0;
    uint64_t row_bytes = 0, stream_bytes = 0, workspace_bytes = 0;
    char msg[160] = "";
};

static inline int fail(Header& h, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h.msg, sizeof(h.msg), fmt, ap);
    va_end(ap);
    return P_EINVAL;
}

static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct CrcTable {
    uint32_t t[4][256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 4; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255];
    }
};

static inline uint32_t crc32(const uint8_t* p, size_t n) {
    static const CrcTable T;
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 4; n -= 4, p += 4) {
        c ^= (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        c = T.t[3][c & 255] ^ T.t[2][(c >> 8) & 255] ^ T.t[1][(c >> 16) & 255] ^ T.t[0][c >> 24];
    }
    for (; n; --n, ++p) c = T.t[0][(c ^ *p) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

static inline uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;   // the longest run whose sums stay below 2^32
        for (size_t i = 0; i < k; ++i) { a += p[i]; b += a; }
        a %= 65521; b %= 65521;
        p += k; n -= k;
    }
    return (b << 16) | a;
}

static inline int channels_of(int colour) { return colour == 0 || colour == 3 ? 1 : colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 0; }

static inline bool legal_pair(int colour, int depth) {
    switch (colour) {
        case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
        case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
        case 2: case 4: case 6: return depth == 8 || depth == 16;
        default: return false;
    }
}

// What the kernel does for a page of `height` rows of `row_bytes` bytes: bands of kBandRows rows (thread = row) walked in skewed steps,
// a step reconstructing one kChunkBytes chunk per row; a band of r rows and c chunks takes c + r - 1 steps.
static inline void plan(int height, uint64_t row_bytes, int* band_rows, int* chunk_bytes, int* bands, int* steps) {
    const int64_t chunks = (int64_t)((row_bytes + kChunkBytes - 1) / kChunkBytes);
    const int nb = (height + kBandRows - 1) / kBandRows;
    int64_t st = 0;
    for (int b = 0; b < nb; ++b) {
        const int rows = height - b * kBandRows < kBandRows ? height - b * kBandRows : kBandRows;
        st += chunks + rows - 1;
    }
    if (band_rows) *band_rows = kBandRows;
    if (chunk_bytes) *chunk_bytes = kChunkBytes;
    if (bands) *bands = nb;
    if (steps) *steps = (int)st;
}

// The line a page of more than one band keeps its band's last reconstructed row in: whole chunks, a multiple of 256 bytes.
static inline uint64_t line_bytes(int height, uint64_t row_bytes) {
    if (height <= kBandRows) return 0;
    const uint64_t chunks = (row_bytes + kChunkBytes - 1) / kChunkBytes;
    return (chunks * kChunkBytes + 255) / 256 * 256;
}

// Signature, IHDR and the chunk list up to IEND.  The CRC of IHDR, PLTE and IEND is checked here; that of the IDAT chunks too when
// `idat_crc` (ocrvi_png_parse; ocrvi_png_info leaves the bulk of the file unread).
static inline int parse_headers(const uint8_t* d, size_t n, Header& h, bool idat_crc) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    memset(h.palette, 0, sizeof(h.palette));
    if (!d || n < 8 || memcmp(d, sig, 8) != 0) return fail(h, "not a PNG file (no PNG signature)");
    size_t pos = 8;
    int idat_state = 0;            // 0 before, 1 inside, 2 after the run of IDAT chunks
    bool have_plte = false;
    for (;;) {
        if (n - pos < 12) return fail(h, "truncated file: no IEND chunk (the file ends at byte %zu)", n);
        const uint32_t len = be32(d + pos);
        const uint8_t* type = d + pos + 4;
        if (len > 0x7FFFFFFFu || (size_t)len > n - pos - 12) {
            char name[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 4; ++i) name[i] = type[i] >= 32 && type[i] < 127 ? (char)type[i] : '?';
            return fail(h, "truncated file: chunk %s at byte %zu claims %u bytes, the file has %zu left", name, pos, len, n - pos - 12);
        }
        const uint8_t* body = type + 4;
        const bool is_ihdr = memcmp(type, "IHDR", 4) == 0, is_plte = memcmp(type, "PLTE", 4) == 0, is_idat = memcmp(type, "IDAT", 4) == 0,
                   is_iend = memcmp(type, "IEND", 4) == 0;
        if (!h.have_ihdr && !is_ihdr) {
            if (!(type[0] & 0x20)) {
                char name[5] = {0, 0, 0, 0, 0};
                for (int i = 0; i < 4; ++i) name[i] = type[i] >= 32 && type[i] < 127 ? (char)type[i] : '?';
                return fail(h, "unknown critical chunk %s before IHDR%s", name, memcmp(type, "CgBI", 4) == 0 ? " (an Apple CgBI file)" : "");
            }
            return fail(h, "IHDR is not the first chunk");
        }
        if (is_ihdr || is_plte || is_iend || (is_idat && idat_crc)) {
            if (crc32(type, (size_t)len + 4) != be32(body + len)) {
                return fail(h, "wrong CRC on the %.4s chunk at byte %zu", (const char*)type, pos);
            }
        }
        if (is_ihdr) {
            if (h.have_ihdr) return fail(h, "a second IHDR chunk");
            if (len != 13) return fail(h, "IHDR of %u bytes instead of 13", len);
            const uint32_t w = be32(body), ht = be32(body + 4);
            h.depth = body[8]; h.colour = body[9];
            if (w == 0 || ht == 0 || w > (uint32_t)kMaxSide || ht > (uint32_t)kMaxSide)
                return fail(h, "image size %u x %u: a side of 0 or above %d is not supported", w, ht, (int)kMaxSide);
            h.width = (int)w; h.height = (int)ht;
            h.have_ihdr = true;
            if (!legal_pair(h.colour, h.depth)) return fail(h, "illegal pair of colour type %d and bit depth %d", h.colour, h.depth);
            h.channels = channels_of(h.colour);
            if (body[10] != 0) return fail(h, "compression method %d is not supported (only 0, deflate)", body[10]);
            if (body[11] != 0) return fail(h, "filter method %d is not supported (only 0)", body[11]);
            if (body[12] == 1) return fail(h, "Adam7 interlace is not supported");
            if (body[12] != 0) return fail(h, "interlace method %d is not supported", body[12]);
            h.row_bytes = ((uint64_t)h.width * h.channels * h.depth + 7) / 8;
            h.stream_bytes = (h.colour == 3 ? (uint64_t)kPaletteBytes : 0) + (uint64_t)h.height * (1 + h.row_bytes);
            h.workspace_bytes = line_bytes(h.height, h.row_bytes);
        } else if (is_plte) {
            if (have_plte) return fail(h, "a second PLTE chunk");
            if (idat_state) return fail(h, "PLTE after IDAT");
            if (len % 3 != 0) return fail(h, "PLTE length %u is not a multiple of 3", len);
            if (len > 768) return fail(h, "PLTE with %u entries (above 256)", len / 3);
            if (len == 0) return fail(h, "PLTE with no entries");
            have_plte = true;
            h.palette_entries = (int)(len / 3);
            for (uint32_t i = 0; i < len / 3; ++i) {
                h.palette[4 * i] = body[3 * i]; h.palette[4 * i + 1] = body[3 * i + 1]; h.palette[4 * i + 2] = body[3 * i + 2];
            }
        } else if (is_idat) {
            if (idat_state == 2) return fail(h, "IDAT chunks are not consecutive (another chunk lies between them)");
            if (h.colour == 3 && !have_plte) return fail(h, "a palette image (colour type 3) without PLTE before IDAT");
            if (idat_state == 0) h.first_idat = pos;
            idat_state = 1;
            ++h.idat_chunks;
            h.idat_bytes += len;
        } else if (is_iend) {
            if (!idat_state) return fail(h, "no IDAT chunk before IEND");
            if (h.colour != 3) h.palette_entries = 0;      // a suggested palette (PLTE in a truecolour file) is not used
            return P_OK;
        } else {
            if (!(type[0] & 0x20)) {
                char name[5] = {0, 0, 0, 0, 0};
                for (int i = 0; i < 4; ++i) name[i] = type[i] >= 32 && type[i] < 127 ? (char)type[i] : '?';
                return fail(h, "unknown critical chunk %s", name);
            }
        }                                                  // (ancillary: skipped by its length, its CRC unread)
        if (!is_idat && idat_state == 1) idat_state = 2;
        pos += (size_t)len + 12;
    }
}

// ---- inflate (RFC 1951) ------------------------------------------------------------------------------------------------------------

struct Bits {
    const uint8_t* p;
    size_t n, pos = 0;
    uint64_t acc = 0;
    int cnt = 0;
    Bits(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
    // at least `need` (<= 32) bits in acc, or false at the end of the input
    inline bool fill(int need) {
        while (cnt <= 56 && pos < n) { acc |= (uint64_t)p[pos++] << cnt; cnt += 8; }
        return cnt >= need;
    }
    inline uint32_t peek(int k) const { return (uint32_t)(acc & ((1ull << k) - 1)); }
    inline void drop(int k) { acc >>= k; cnt -= k; }
};

// A canonical Huffman code: a 9-bit lookup for the short codes, the count / symbol walk of the RFC for the long ones.
struct Huff {
    enum { kFast = 9 };
    uint16_t count[16], symbol[288];
    uint16_t fast[1 << kFast];        // (symbol << 4) | length, 0 = not a short code
};

// 0 ok; -1 over-subscribed; -2 incomplete (the caller decides whether the single-code case applies)
static inline int build(Huff& t, const uint8_t* lengths, int n) {
    memset(t.count, 0, sizeof(t.count));
    for (int i = 0; i < n; ++i) ++t.count[lengths[i]];
    memset(t.fast, 0, sizeof(t.fast));
    int left = 1;
    for (int len = 1; len < 16; ++len) {
        left <<= 1;
        left -= t.count[len];
        if (left < 0) return -1;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int len = 1; len < 15; ++len) offs[len + 1] = (uint16_t)(offs[len] + t.count[len]);
    for (int i = 0; i < n; ++i)
        if (lengths[i]) t.symbol[offs[lengths[i]]++] = (uint16_t)i;
    // the short codes, bit-reversed as the stream presents them
    int code = 0, index = 0;
    for (int len = 1; len <= Huff::kFast; ++len) {
        for (int k = 0; k < t.count[len]; ++k, ++code, ++index) {
            int rev = 0;
            for (int b = 0; b < len; ++b) rev |= ((code >> b) & 1) << (len - 1 - b);
            for (int f = rev; f < (1 << Huff::kFast); f += 1 << len) t.fast[f] = (uint16_t)((t.symbol[index] << 4) | len);
        }
        code <<= 1;
    }
    return left > 0 ? -2 : 0;
}

// -> symbol, or -1 at the end of the input, or -2 for a code with no symbol
static inline int decode(Bits& b, const Huff& t) {
    b.fill(15);
    if (b.cnt == 0) return -1;
    const uint16_t f = t.fast[b.peek(Huff::kFast)];
    if (f) {
        if ((f & 15) > b.cnt) return -1;
        b.drop(f & 15);
        return f >> 4;
    }
    int code = 0, first = 0, index = 0;
    uint64_t acc = b.acc;
    for (int len = 1; len < 16; ++len) {
        if (len > b.cnt) return -1;
        code |= (int)(acc & 1);
        acc >>= 1;
        const int count = t.count[len];
        if (code - count < first) {
            b.drop(len);
            return t.symbol[index + (code - first)];
        }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -2;
}

static const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                       8193, 12289, 16385, 24577};
static const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// Inflates the zlib stream z[0 .. zn) into exactly `want` bytes at out; bytes after the end of the zlib stream are ignored.
static inline int inflate_zlib(const uint8_t* z, size_t zn, uint8_t* out, uint64_t want, Header& h) {
    if (zn < 2) return fail(h, "truncated zlib stream: no header");
    if ((z[0] & 15) != 8) return fail(h, "bad zlib header: compression method %d is not 8 (deflate)", z[0] & 15);
    if ((z[0] >> 4) > 7) return fail(h, "bad zlib header: window of 2^%d bytes is above 32 K", (z[0] >> 4) + 8);
    if (((z[0] << 8) | z[1]) % 31 != 0) return fail(h, "bad zlib header: FCHECK does not match");
    if (z[1] & 0x20) return fail(h, "bad zlib header: a preset dictionary is not allowed in PNG");
    Bits b(z + 2, zn - 2);
    uint64_t o = 0;
    Huff lit, dist;
    for (bool last = false; !last;) {
        if (!b.fill(3)) return fail(h, "truncated deflate stream: no block header");
        last = b.peek(1) != 0;
        const int btype = (int)(b.peek(3) >> 1);
        b.drop(3);
        if (btype == 3) return fail(h, "reserved deflate block type 3");
        if (btype == 0) {
            b.drop(b.cnt & 7);                                      // to the byte boundary; the accumulator holds whole bytes from here
            if (!b.fill(32)) return fail(h, "truncated deflate stream: no stored-block length");
            const uint32_t len = b.peek(16), nlen = b.peek(32) >> 16;
            b.drop(32);
            if ((len ^ 0xFFFFu) != nlen) return fail(h, "stored-block length %u does not match its complement", len);
            if (len > want - o) return fail(h, "the inflated data are longer than the %llu bytes the header implies", (unsigned long long)want);
            uint32_t k = 0;
            for (; k < len && b.cnt >= 8; ++k) { out[o++] = (uint8_t)b.peek(8); b.drop(8); }
            if (len - k > b.n - b.pos) return fail(h, "truncated deflate stream: a stored block of %u bytes ends past the data", len);
            memcpy(out + o, b.p + b.pos, len - k);
            b.pos += len - k; o += len - k;
            continue;
        }
        if (btype == 1) {
            uint8_t lengths[288 + 30];
            for (int i = 0; i < 144; ++i) lengths[i] = 8;
            for (int i = 144; i < 256; ++i) lengths[i] = 9;
            for (int i = 256; i < 280; ++i) lengths[i] = 7;
            for (int i = 280; i < 288; ++i) lengths[i] = 8;
            for (int i = 0; i < 30; ++i) lengths[288 + i] = 5;
            build(lit, lengths, 288);
            build(dist, lengths + 288, 30);                         // (incomplete by two codes, as the format defines it)
        } else {
            if (!b.fill(14)) return fail(h, "truncated deflate stream: no code counts");
            const int nlen = (int)b.peek(5) + 257, ndist = (int)(b.peek(10) >> 5) + 1, ncode = (int)(b.peek(14) >> 10) + 4;
            b.drop(14);
            if (nlen > 286 || ndist > 30) return fail(h, "bad deflate block: %d literal/length and %d distance codes", nlen, ndist);
            static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t lengths[288 + 32];
            memset(lengths, 0, sizeof(lengths));
            for (int i = 0; i < ncode; ++i) {
                if (!b.fill(3)) return fail(h, "truncated deflate stream: code-length code lengths");
                lengths[order[i]] = (uint8_t)b.peek(3);
                b.drop(3);
            }
            Huff cl;
            if (build(cl, lengths, 19) != 0) return fail(h, "bad deflate block: the code-length code is over-subscribed or incomplete");
            uint8_t ll[288 + 32];
            memset(ll, 0, sizeof(ll));
            for (int i = 0; i < nlen + ndist;) {
                const int sym = decode(b, cl);
                if (sym == -1) return fail(h, "truncated deflate stream: code lengths");
                if (sym < 0) return fail(h, "bad deflate block: a code-length code with no symbol");
                if (sym < 16) { ll[i++] = (uint8_t)sym; continue; }
                int prev = 0, rep;
                if (sym == 16) {
                    if (i == 0) return fail(h, "bad deflate block: a repeat with no length before it");
                    prev = ll[i - 1];
                    if (!b.fill(2)) return fail(h, "truncated deflate stream: code lengths");
                    rep = 3 + (int)b.peek(2); b.drop(2);
                } else if (sym == 17) {
                    if (!b.fill(3)) return fail(h, "truncated deflate stream: code lengths");
                    rep = 3 + (int)b.peek(3); b.drop(3);
                } else {
                    if (!b.fill(7)) return fail(h, "truncated deflate stream: code lengths");
                    rep = 11 + (int)b.peek(7); b.drop(7);
                }
                if (i + rep > nlen + ndist) return fail(h, "bad deflate block: a repeat runs past the code lengths");
                while (rep--) ll[i++] = (uint8_t)prev;
            }
            if (ll[256] == 0) return fail(h, "bad deflate block: no end-of-block code");
            int rc = build(lit, ll, nlen);
            if (rc == -1) return fail(h, "bad deflate block: over-subscribed literal/length code");
            // (an incomplete set passes only as zlib lets it: a single code of one bit; or, for distances, no code at all)
            if (rc == -2 && !(nlen - lit.count[0] == 1 && lit.count[1] == 1)) return fail(h, "bad deflate block: incomplete literal/length code");
            rc = build(dist, ll + nlen, ndist);
            if (rc == -1) return fail(h, "bad deflate block: over-subscribed distance code");
            if (rc == -2 && !(ndist - dist.count[0] == 1 && dist.count[1] == 1) && ndist != dist.count[0])
                return fail(h, "bad deflate block: incomplete distance code");
        }
        for (;;) {
            int sym = decode(b, lit);
            if (sym == -1) return fail(h, "truncated deflate stream: the data end inside a block");
            if (sym < 0) return fail(h, "bad deflate stream: a literal/length code with no symbol");
            if (sym < 256) {
                if (o >= want) return fail(h, "the inflated data are longer than the %llu bytes the header implies", (unsigned long long)want);
                out[o++] = (uint8_t)sym;
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return fail(h, "bad deflate stream: length symbol %d", sym + 257);
            if (!b.fill(kLenExtra[sym])) return fail(h, "truncated deflate stream: length bits");
            const uint32_t len = kLenBase[sym] + b.peek(kLenExtra[sym]);
            b.drop(kLenExtra[sym]);
            const int ds = decode(b, dist);
            if (ds == -1) return fail(h, "truncated deflate stream: the data end inside a block");
            if (ds < 0) return fail(h, "bad deflate stream: a distance code with no symbol");
            if (ds >= 30) return fail(h, "bad deflate stream: distance symbol %d", ds);
            if (!b.fill(kDistExtra[ds])) return fail(h, "truncated deflate stream: distance bits");
            const uint64_t dd = kDistBase[ds] + b.peek(kDistExtra[ds]);
            b.drop(kDistExtra[ds]);
            if (dd > o) return fail(h, "bad deflate stream: a distance of %llu reaches before the start of the output", (unsigned long long)dd);
            if (len > want - o) return fail(h, "the inflated data are longer than the %llu bytes the header implies", (unsigned long long)want);
            const uint8_t* s = out + o - dd;
            uint8_t* q = out + o;
            if (dd >= len) memcpy(q, s, len);
            else for (uint32_t i = 0; i < len; ++i) q[i] = s[i];    // an overlapping run repeats itself
            o += len;
        }
    }
    if (o != want)
        return fail(h, "the inflated data are %llu bytes, shorter than the %llu the header implies", (unsigned long long)o, (unsigned long long)want);
    // the Adler-32 follows at the next byte boundary; whole bytes still in the accumulator come first
    b.drop(b.cnt & 7);
    uint8_t ad[4];
    for (int i = 0; i < 4; ++i) {
        if (b.cnt >= 8) { ad[i] = (uint8_t)b.peek(8); b.drop(8); }
        else if (b.pos < b.n) ad[i] = b.p[b.pos++];
        else return fail(h, "truncated zlib stream: no Adler-32");
    }
    if (be32(ad) != adler32(out, (size_t)want)) return fail(h, "wrong Adler-32 on the inflated data");
    return P_OK;
}

// The page's stream into out[0 .. cap): P_ENOMEM when cap < h.stream_bytes, otherwise exactly h.stream_bytes bytes.
static inline int parse_stream(const uint8_t* d, size_t n, Header& h, void* out, size_t cap, size_t* used) {
    *used = 0;
    if ((uint64_t)cap < h.stream_bytes) {
        snprintf(h.msg, sizeof(h.msg), "png_parse: cap = %zu is below the stream's %llu bytes", cap, (unsigned long long)h.stream_bytes);
        return P_ENOMEM;
    }
    uint8_t* o = (uint8_t*)out;
    if (h.colour == 3) { memcpy(o, h.palette, kPaletteBytes); o += kPaletteBytes; }
    const uint64_t want = (uint64_t)h.height * (1 + h.row_bytes);
    int rc;
    if (h.idat_chunks == 1) {
        rc = inflate_zlib(d + h.first_idat + 8, (size_t)h.idat_bytes, o, want, h);
    } else {                                                        // the chunks' data, joined (parse_headers has checked every length)
        uint8_t* z = (uint8_t*)malloc(h.idat_bytes ? (size_t)h.idat_bytes : 1);
        if (!z) { snprintf(h.msg, sizeof(h.msg), "png_parse: out of host memory joining %d IDAT chunks", h.idat_chunks); return P_ENOMEM; }
        size_t pos = h.first_idat, zn = 0;
        for (int k = 0; k < h.idat_chunks; ++k) {
            const uint32_t len = be32(d + pos);
            memcpy(z + zn, d + pos + 8, len);
            zn += len; pos += (size_t)len + 12;
        }
        rc = inflate_zlib(z, zn, o, want, h);
        free(z);
    }
    if (rc != P_OK) return rc;
    for (int y = 0; y < h.height; ++y) {
        const uint8_t f = o[(uint64_t)y * (1 + h.row_bytes)];
        if (f > 4) return fail(h, "row %d has filter byte %d (above 4)", y, f);
    }
    *used = (size_t)h.stream_bytes;
    return P_OK;
}

}  // namespace png
}  // namespace ocrvi
