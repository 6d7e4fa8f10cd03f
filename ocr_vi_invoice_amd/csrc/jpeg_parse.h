// Baseline JPEG on the host: marker parser, EXIF orientation, Huffman decoder -> the sparse coefficient stream of include/ocrvi.h
// ("JPEG decode").  Plain C++17, no HIP: tools/jpeg_parse_check.cpp includes this file alone.  The input is untrusted: every read goes
// through a bounds check, every loop consumes input or ends, and nothing is written outside the caller's buffer.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace ocrvi {
namespace jpeg {

enum { J_OK = 0, J_EINVAL = -1, J_ENOMEM = -3 };   // the values of OCRVI_OK / OCRVI_EINVAL / OCRVI_ENOMEM

struct Header {
    int width = 0, height = 0, ncomp = 0;
    int comp_id[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int restart_interval = 0, orientation = 1;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    uint16_t quant[4][64];            // natural (row-major) order
    bool have_quant[4] = {false, false, false, false};
    uint8_t bits[2][4][17];           // [class][id][length] = number of codes of that length
    uint8_t vals[2][4][256];
    bool have_huff[2][4] = {{false, false, false, false}, {false, false, false, false}};
    size_t scan_pos = 0;              // first byte of entropy-coded data
    // derived
    int mcus_x = 0, mcus_y = 0, blocks_per_mcu = 0;
    int64_t blocks = 0;
    char msg[160] = "";
};

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static inline int fail(Header& h, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h.msg, sizeof(h.msg), fmt, ap);
    va_end(ap);
    return J_EINVAL;
}

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// EXIF: only tag 0x0112 of IFD0 is read; anything malformed leaves the orientation at 1.
static inline int exif_orientation(const uint8_t* p, size_t n) {
    if (n < 14 || memcmp(p, "Exif\0\0", 6) != 0) return 1;
    const uint8_t* t = p + 6;
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 1;
    auto u16 = [&](size_t o) -> uint32_t { return le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1]); };
    auto u32 = [&](size_t o) -> uint32_t {
        return le ? ((uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
                  : (((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]);
    };
    if (u16(2) != 42) return 1;
    const size_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 1;
    const size_t cnt = u16(ifd);
    for (size_t i = 0; i < cnt; ++i) {
        const size_t e = ifd + 2 + 12 * i;
        if (e > tn || tn - e < 12) return 1;
        if (u16(e) == 0x0112) {
            if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;
            const uint32_t v = u16(e + 8);
            return (v >= 1 && v <= 8) ? (int)v : 1;
        }
    }
    return 1;
}

// Markers from SOI up to and including the SOS header.  J_EINVAL with h.msg for a corrupt or unsupported file.
static inline int parse_headers(const uint8_t* d, size_t n, Header& h) {
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(h, "jpeg: no SOI marker (not a JPEG file)");
    size_t p = 2;
    for (;;) {
        if (p >= n) return fail(h, "jpeg: truncated before SOS");
        if (d[p] != 0xFF) return fail(h, "jpeg: expected a marker at byte %zu", p);
        while (p < n && d[p] == 0xFF) ++p;          // fill bytes
        if (p >= n) return fail(h, "jpeg: truncated marker");
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00)
            return fail(h, "jpeg: marker FF%02X before SOS", m);
        if (m == 0xD9) return fail(h, "jpeg: EOI before SOS (no image data)");
        if (n - p < 2) return fail(h, "jpeg: truncated segment length");
        const size_t len = (size_t)be16(d + p);
        if (len < 2 || len > n - p) return fail(h, "jpeg: bad length %zu of segment FF%02X", len, m);
        const uint8_t* s = d + p + 2;
        const size_t sn = len - 2;
        p += len;
        if (m == 0xC0 || m == 0xC1) {
            if (h.have_sof) return fail(h, "jpeg: two frame headers");
            if (sn < 6) return fail(h, "jpeg: bad SOF length");
            const int prec = s[0];
            if (prec != 8) return fail(h, "jpeg: unsupported: %d-bit precision (only 8-bit)", prec);
            h.height = be16(s + 1);
            h.width = be16(s + 3);
            h.ncomp = s[5];
            if (h.height == 0 || h.width == 0 || h.height > 65500 || h.width > 65500)
                return fail(h, "jpeg: bad dimensions %dx%d (1 .. 65500)", h.height, h.width);
            if (h.ncomp == 4) return fail(h, "jpeg: unsupported: 4 components (CMYK / YCCK)");
            if (h.ncomp != 1 && h.ncomp != 3) return fail(h, "jpeg: bad number of components %d", h.ncomp);
            if (sn != (size_t)(6 + 3 * h.ncomp)) return fail(h, "jpeg: bad SOF length");
            for (int c = 0; c < h.ncomp; ++c) {
                h.comp_id[c] = s[6 + 3 * c];
                h.hs[c] = s[7 + 3 * c] >> 4;
                h.vs[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
                if (h.hs[c] < 1 || h.hs[c] > 4 || h.vs[c] < 1 || h.vs[c] > 4) return fail(h, "jpeg: bad sampling factors %dx%d", h.hs[c], h.vs[c]);
                if (h.tq[c] > 3) return fail(h, "jpeg: bad quantisation table id %d", h.tq[c]);
            }
            if (h.ncomp == 1) {
                h.hs[0] = h.vs[0] = 1;               // a single-component scan is not interleaved: the factors have no effect
            } else {
                const bool luma_ok = (h.hs[0] == 1 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 2);
                if (!luma_ok || h.hs[1] != 1 || h.vs[1] != 1 || h.hs[2] != 1 || h.vs[2] != 1)
                    return fail(h, "jpeg: unsupported: sampling factors %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 only)", h.hs[0], h.vs[0], h.hs[1],
                                h.vs[1], h.hs[2], h.vs[2]);
            }
            h.have_sof = true;
        } else if (m == 0xC2) {
            return fail(h, "jpeg: unsupported: progressive (SOF2)");
        } else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
            return fail(h, "jpeg: unsupported: lossless (SOF%d)", m - 0xC0);
        } else if (m == 0xC9 || m == 0xCA || m == 0xCD || m == 0xCE || m == 0xCC) {
            return fail(h, "jpeg: unsupported: arithmetic coding (FF%02X)", m);
        } else if (m == 0xC5 || m == 0xC6) {
            return fail(h, "jpeg: unsupported: hierarchical (SOF%d)", m - 0xC0);
        } else if (m == 0xDC) {
            return fail(h, "jpeg: unsupported: DNL marker");
        } else if (m == 0xC4) {              // DHT
            size_t q = 0;
            while (q < sn) {
                if (sn - q < 17) return fail(h, "jpeg: bad DHT length");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return fail(h, "jpeg: bad Huffman table id %02X", s[q]);
                int total = 0;
                h.bits[tc][th][0] = 0;
                for (int i = 1; i <= 16; ++i) { h.bits[tc][th][i] = s[q + i]; total += s[q + i]; }
                if (total > 256 || (size_t)total > sn - q - 17) return fail(h, "jpeg: bad DHT length");
                // the code space must not overflow (Kraft): otherwise two symbols would share a code
                int code = 0;
                for (int i = 1; i <= 16; ++i) {
                    code += h.bits[tc][th][i];
                    if (code > (1 << i)) return fail(h, "jpeg: bad Huffman table (over-subscribed)");
                    code <<= 1;
                }
                memcpy(h.vals[tc][th], s + q + 17, (size_t)total);
                h.have_huff[tc][th] = true;
                q += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {              // DQT
            size_t q = 0;
            while (q < sn) {
                const int pq = s[q] >> 4, id = s[q] & 15;
                if (pq > 1 || id > 3) return fail(h, "jpeg: bad quantisation table %02X", s[q]);
                const size_t need = 1 + (pq ? 128 : 64);
                if (sn - q < need) return fail(h, "jpeg: bad DQT length");
                for (int i = 0; i < 64; ++i)
                    h.quant[id][kZigzag[i]] = pq ? (uint16_t)be16(s + q + 1 + 2 * i) : (uint16_t)s[q + 1 + i];
                h.have_quant[id] = true;
                q += need;
            }
        } else if (m == 0xDD) {              // DRI
            if (sn != 2) return fail(h, "jpeg: bad DRI length");
            h.restart_interval = be16(s);
        } else if (m == 0xE0) {
            if (sn >= 5 && memcmp(s, "JFIF\0", 5) == 0) h.jfif = true;
        } else if (m == 0xE1) {
            if (sn >= 6 && memcmp(s, "Exif\0\0", 6) == 0) h.orientation = exif_orientation(s, sn);
        } else if (m == 0xEE) {
            if (sn >= 12 && memcmp(s, "Adobe", 5) == 0) { h.adobe = true; h.adobe_transform = s[11]; }
        } else if (m == 0xDA) {              // SOS
            if (!h.have_sof) return fail(h, "jpeg: SOS before the frame header");
            if (sn < 1) return fail(h, "jpeg: bad SOS length");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sn != (size_t)(4 + 2 * ns)) return fail(h, "jpeg: bad SOS length");
            if (ns != h.ncomp) return fail(h, "jpeg: unsupported: several scans (a scan of %d of %d components)", ns, h.ncomp);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.comp_id[c]) return fail(h, "jpeg: scan component %d does not match the frame", c);
                h.td[c] = s[2 + 2 * c] >> 4;
                h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return fail(h, "jpeg: bad Huffman table selector");
                if (!h.have_huff[0][h.td[c]] || !h.have_huff[1][h.ta[c]]) return fail(h, "jpeg: missing Huffman table");
                if (!h.have_quant[h.tq[c]]) return fail(h, "jpeg: missing quantisation table %d", h.tq[c]);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return fail(h, "jpeg: bad spectral selection in a sequential scan");
            if (h.ncomp == 3) {
                if (h.adobe && h.adobe_transform == 0) return fail(h, "jpeg: unsupported: Adobe transform 0 (RGB-coded)");
                if (!h.jfif && h.comp_id[0] == 'R' && h.comp_id[1] == 'G' && h.comp_id[2] == 'B')
                    return fail(h, "jpeg: unsupported: component ids R, G, B without JFIF (RGB-coded)");
            }
            h.scan_pos = p;
            const int mw = 8 * h.hs[0], mh = 8 * h.vs[0];
            h.mcus_x = (h.width + mw - 1) / mw;
            h.mcus_y = (h.height + mh - 1) / mh;
            h.blocks_per_mcu = h.ncomp == 1 ? 1 : h.hs[0] * h.vs[0] + 2;
            h.blocks = (int64_t)h.mcus_x * h.mcus_y * h.blocks_per_mcu;
            // a block takes at least two bits (a DC code and an EOB code): a file too short for its size is refused before anything is sized by it
            if (h.blocks > 4 * (int64_t)(n - p)) return fail(h, "jpeg: truncated (%lld blocks, %zu bytes of scan data)", (long long)h.blocks, n - p);
            return J_OK;
        }
        // other APPn / COM / reserved segments are skipped
    }
}

// Upper bound of the stream's size: nblocks + 1 offsets and one word per non-zero coefficient.  An AC record takes at least two bits of
// scan data (a code and one magnitude bit); a DC record can cost a single bit (a one-bit code for a zero difference on a non-zero
// prediction), so each block adds one record to what the bits allow.  A block holds at most 64.
static inline uint64_t stream_bound(const Header& h, size_t n) {
    const uint64_t by_bits = 4ull * (uint64_t)(n - h.scan_pos) + (uint64_t)h.blocks, by_blocks = 64ull * (uint64_t)h.blocks;
    return 4ull * ((uint64_t)h.blocks + 1 + (by_bits < by_blocks ? by_bits : by_blocks));
}
// Bytes of the component planes, each padded to whole blocks of whole MCUs.
static inline uint64_t plane_bytes(const Header& h) {
    const uint64_t luma = 64ull * h.mcus_x * h.hs[0] * h.mcus_y * h.vs[0];
    return h.ncomp == 1 ? luma : luma + 2 * 64ull * h.mcus_x * h.mcus_y;
}

struct HuffLut {
    enum { FAST = 10 };
    uint16_t fast[1 << FAST];      // (length << 8) | symbol, 0 = longer than FAST bits or not a code
    int32_t maxcode[18];           // largest code of each length, -1 when none
    int32_t valptr[17], mincode[17];
    const uint8_t* vals;
};

static inline void build_lut(const uint8_t* bits, const uint8_t* vals, HuffLut& t) {
    memset(t.fast, 0, sizeof(t.fast));
    t.vals = vals;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
            if (l <= HuffLut::FAST) {
                const int lo = code << (HuffLut::FAST - l), cnt = 1 << (HuffLut::FAST - l);
                for (int j = 0; j < cnt; ++j) t.fast[lo + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t.maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
}

struct BitReader {
    const uint8_t* d;
    size_t p, n;
    uint64_t acc = 0;     // the low `nbits` bits are valid, the oldest bit highest
    int nbits = 0;
    bool stopped = false;  // a marker or the end of the file: no more data bytes
    BitReader(const uint8_t* d_, size_t p_, size_t n_) : d(d_), p(p_), n(n_) {}
    void fill() {
        while (nbits <= 56 && !stopped) {
            if (p >= n) { stopped = true; break; }
            const uint8_t b = d[p];
            if (b == 0xFF) {
                if (p + 1 >= n) { stopped = true; break; }
                if (d[p + 1] != 0x00) { stopped = true; break; }   // a marker: p stays on its FF
                p += 2;
            } else {
                p += 1;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    // the next k bits (k <= 16) without consuming them, zero-padded when fewer remain
    uint32_t peek(int k) {
        if (nbits < k) fill();
        if (nbits >= k) return (uint32_t)(acc >> (nbits - k)) & ((1u << k) - 1);
        return (uint32_t)(acc << (k - nbits)) & ((1u << k) - 1);
    }
    bool skip(int k) {
        if (nbits < k) return false;
        nbits -= k;
        return true;
    }
    bool get(int k, uint32_t& v) {
        if (k == 0) { v = 0; return true; }
        if (nbits < k) fill();
        if (nbits < k) return false;
        v = (uint32_t)(acc >> (nbits - k)) & ((1u << k) - 1);
        nbits -= k;
        return true;
    }
};

// One Huffman symbol, or -1 (no such code / out of data).
static inline int decode_symbol(BitReader& br, const HuffLut& t) {
    const uint32_t look = br.peek(HuffLut::FAST);
    const uint16_t f = t.fast[look];
    if (f) return br.skip(f >> 8) ? (f & 255) : -1;
    const uint32_t w = br.peek(16);
    for (int l = HuffLut::FAST + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(w >> (16 - l));
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l])
            return br.skip(l) ? t.vals[t.valptr[l] + code - t.mincode[l]] : -1;
    }
    return -1;
}

static inline int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// The scan -> out: uint32 [blocks + 1] record offsets (block d, in the order the scan codes them, owns records off[d] .. off[d+1]) followed
// by the records, (natural position << 16) | (coefficient & 0xffff), DC first and then in zigzag order, non-zero coefficients only.
static inline int parse_scan(const uint8_t* d, size_t n, Header& h, void* out, size_t cap, size_t* used) {
    const uint64_t nb = (uint64_t)h.blocks;
    if ((uint64_t)cap / 4 < nb + 1) { snprintf(h.msg, sizeof(h.msg), "jpeg_parse: cap %zu is below the %llu bytes of the block offsets", cap, (unsigned long long)(4 * (nb + 1))); return J_ENOMEM; }
    uint32_t* off = (uint32_t*)out;
    uint32_t* rec = off + nb + 1;
    const uint64_t rec_cap = (uint64_t)cap / 4 - (nb + 1);
    uint64_t nrec = 0;
    if (rec_cap > 0xffffffffull) return fail(h, "jpeg_parse: cap above the 2^32 records an offset can address");
    HuffLut dc[3], ac[3];
    for (int c = 0; c < h.ncomp; ++c) {
        build_lut(h.bits[0][h.td[c]], h.vals[0][h.td[c]], dc[c]);
        build_lut(h.bits[1][h.ta[c]], h.vals[1][h.ta[c]], ac[c]);
    }
    BitReader br(d, h.scan_pos, n);
    int pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)h.mcus_x * h.mcus_y;
    const int nluma = h.ncomp == 1 ? 1 : h.hs[0] * h.vs[0];
    uint64_t blk = 0;
    int rst = 0;
    for (int64_t mcu = 0; mcu < mcus; ++mcu) {
        if (h.restart_interval && mcu && mcu % h.restart_interval == 0) {
            if (br.nbits >= 8) return fail(h, "jpeg: data where RST%d was expected (MCU %lld)", rst, (long long)mcu);
            br.nbits = 0;
            br.acc = 0;
            size_t p = br.p;
            if (p >= n || d[p] != 0xFF) return fail(h, "jpeg: missing RST%d (MCU %lld)", rst, (long long)mcu);
            while (p < n && d[p] == 0xFF) ++p;
            if (p >= n) return fail(h, "jpeg: truncated at RST%d", rst);
            if (d[p] != 0xD0 + rst) return fail(h, "jpeg: expected RST%d, found FF%02X (MCU %lld)", rst, d[p], (long long)mcu);
            br.p = p + 1;
            br.stopped = false;
            rst = (rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int b = 0; b < h.blocks_per_mcu; ++b, ++blk) {
            const int c = b < nluma ? 0 : b - nluma + 1;
            off[blk] = (uint32_t)nrec;
            const int s = decode_symbol(br, dc[c]);
            if (s < 0) return fail(h, "jpeg: bad Huffman code or truncated data (DC, block %llu)", (unsigned long long)blk);
            if (s > 15) return fail(h, "jpeg: bad DC category %d (block %llu)", s, (unsigned long long)blk);
            uint32_t v;
            if (!br.get(s, v)) return fail(h, "jpeg: truncated data (block %llu)", (unsigned long long)blk);
            const int dcv = pred[c] + (s ? extend(v, s) : 0);
            if (dcv < -32768 || dcv > 32767) return fail(h, "jpeg: DC coefficient %d outside 16 bits (block %llu)", dcv, (unsigned long long)blk);
            pred[c] = dcv;
            if (dcv) {
                if (nrec >= rec_cap) { snprintf(h.msg, sizeof(h.msg), "jpeg_parse: cap %zu is too small", cap); return J_ENOMEM; }
                rec[nrec++] = (uint32_t)(uint16_t)dcv;
            }
            for (int k = 1; k < 64;) {
                const int rs = decode_symbol(br, ac[c]);
                if (rs < 0) return fail(h, "jpeg: bad Huffman code or truncated data (AC, block %llu)", (unsigned long long)blk);
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    if (r != 15) {
                        if (r != 0) return fail(h, "jpeg: EOBn code in a sequential scan (block %llu)", (unsigned long long)blk);
                        break;
                    }
                    k += 16;
                    if (k > 63) return fail(h, "jpeg: zero run past coefficient 63 (block %llu)", (unsigned long long)blk);
                    continue;
                }
                k += r;
                if (k > 63) return fail(h, "jpeg: run past coefficient 63 (block %llu)", (unsigned long long)blk);
                if (!br.get(sz, v)) return fail(h, "jpeg: truncated data (block %llu)", (unsigned long long)blk);
                if (nrec >= rec_cap) { snprintf(h.msg, sizeof(h.msg), "jpeg_parse: cap %zu is too small", cap); return J_ENOMEM; }
                rec[nrec++] = ((uint32_t)kZigzag[k] << 16) | (uint32_t)(uint16_t)extend(v, sz);
                ++k;
            }
        }
    }
    off[nb] = (uint32_t)nrec;
    // after the last MCU: padding bits, then EOI
    if (br.nbits >= 8) return fail(h, "jpeg: data after the last MCU");
    size_t p = br.p;
    if (p >= n || d[p] != 0xFF) return fail(h, "jpeg: truncated (no EOI)");
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n) return fail(h, "jpeg: truncated (no EOI)");
    if (d[p] != 0xD9) {
        if (d[p] == 0xDA || d[p] == 0xC4 || d[p] == 0xDB || d[p] == 0xDD) return fail(h, "jpeg: unsupported: several scans");
        return fail(h, "jpeg: expected EOI, found FF%02X", d[p]);
    }
    *used = (size_t)(4 * (nb + 1 + nrec));
    return J_OK;
}

// The format's own consistency check (tests, tools/jpeg_parse_check.cpp): offsets monotone and inside the records, positions below 64.
static inline bool stream_consistent(const void* out, size_t used, uint64_t blocks) {
    if (used % 4 || used / 4 < blocks + 1) return false;
    const uint32_t* off = (const uint32_t*)out;
    const uint64_t nrec = used / 4 - (blocks + 1);
    if (off[0] != 0 || off[blocks] != nrec) return false;
    for (uint64_t b = 0; b < blocks; ++b)
        if (off[b] > off[b + 1] || off[b + 1] - off[b] > 64) return false;
    const uint32_t* rec = off + blocks + 1;
    for (uint64_t i = 0; i < nrec; ++i)
        if ((rec[i] >> 16) >= 64) return false;
    return true;
}

}  // namespace jpeg
}  // namespace ocrvi
