// Stand-alone robustness check of the host PNG parser (ocr_vi_invoice_amd/csrc/png_parse.h, included alone: no HIP, no library, no zlib).
// For every file on the command line: the whole file must parse; every prefix must be refused; 2000 seeded single-byte corruptions
// must be refused or give a stream of exactly stream_bytes bytes with legal filter bytes, and so must 2000 more whose chunk CRC is put
// right after the corruption (so that the chunk parser and inflate see the bad byte, not only the CRC check).  Inputs and outputs live
// in heap blocks of their exact size, so that a sanitizer build sees any read or write outside them:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/png_parse_check.cpp -o png_parse_check
//   ./png_parse_check file.png ...
//
// Exit status 0 when every expectation held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ocr_vi_invoice_amd/csrc/png_parse.h"

using namespace ocrvi::png;

struct Result { int rc; bool consistent; };

static Result run(const uint8_t* src, size_t n, size_t cap_override = (size_t)-1) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);       // exact size: an over-read is a heap-buffer-overflow
    if (n) memcpy(in, src, n);
    Header h;
    Result r = {parse_headers(n ? in : nullptr, n, h, true), false};
    if (r.rc == P_OK) {
        const size_t cap = cap_override != (size_t)-1 ? cap_override : (size_t)h.stream_bytes;
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        size_t used = 0;
        r.rc = parse_stream(in, n, h, out, cap, &used);
        if (r.rc == P_OK) {
            r.consistent = used == h.stream_bytes && used <= cap;
            const uint8_t* rows = out + (h.colour == 3 ? (size_t)kPaletteBytes : 0);
            for (int y = 0; y < h.height && r.consistent; ++y)
                if (rows[(size_t)y * (1 + h.row_bytes)] > 4) r.consistent = false;
        }
        free(out);
    }
    free(in);
    return r;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s file.png ...\n", argv[0]); return 2; }
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + got);
        fclose(f);
        const Result whole = run(d.data(), d.size());
        if (whole.rc != P_OK || !whole.consistent) { printf("%s: the whole file does not parse (rc %d)\n", argv[a], whole.rc); ++failures; continue; }
        size_t trunc_bad = 0;
        for (size_t n = 0; n < d.size(); ++n)
            if (run(d.data(), n).rc != P_EINVAL) ++trunc_bad;
        size_t ok = 0, refused = 0, corrupt_bad = 0;
        uint64_t s = 0x9E3779B97F4A7C15ull ^ d.size();
        std::vector<uint8_t> c(d);
        for (int i = 0; i < 2000; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            const size_t p = (size_t)(s % d.size());
            const uint8_t x = (uint8_t)(1 + (s >> 32) % 255);
            c[p] ^= x;
            const Result r = run(c.data(), c.size());
            if (r.rc == P_EINVAL) ++refused;
            else if (r.rc == P_OK && r.consistent) ++ok;
            else ++corrupt_bad;
            c[p] ^= x;
        }
        // the same with the CRC of the chunk that holds the byte recomputed
        size_t ok2 = 0, refused2 = 0;
        for (int i = 0; i < 2000; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            const size_t p = (size_t)(s % d.size());
            const uint8_t x = (uint8_t)(1 + (s >> 32) % 255);
            c[p] ^= x;
            size_t at = 8, crc_at = 0;
            uint8_t saved[4] = {0, 0, 0, 0};
            while (at + 12 <= d.size()) {                          // the chunk list of the intact file
                const size_t len = be32(d.data() + at);
                if (len > d.size() - at - 12) break;
                if (p >= at + 4 && p < at + 8 + len) { crc_at = at + 8 + len; break; }
                at += len + 12;
            }
            if (crc_at) {
                memcpy(saved, &c[crc_at], 4);
                const uint32_t v = crc32(&c[at + 4], crc_at - at - 4);
                c[crc_at] = (uint8_t)(v >> 24); c[crc_at + 1] = (uint8_t)(v >> 16); c[crc_at + 2] = (uint8_t)(v >> 8); c[crc_at + 3] = (uint8_t)v;
            }
            const Result r = run(c.data(), c.size());
            if (r.rc == P_EINVAL) ++refused2;
            else if (r.rc == P_OK && r.consistent) ++ok2;
            else ++corrupt_bad;
            if (crc_at) memcpy(&c[crc_at], saved, 4);
            c[p] ^= x;
        }
        const int short_rc = run(d.data(), d.size(), 8).rc;      // a cap below the stream
        printf("%s: %zu bytes; %zu prefixes, %zu not refused; 2000 corruptions: %zu refused, %zu parsed consistently; 2000 with the CRC put right: "
               "%zu refused, %zu parsed consistently; %zu inconsistent; short cap rc %d\n",
               argv[a], d.size(), d.size(), trunc_bad, refused, ok, refused2, ok2, corrupt_bad, short_rc);
        if (trunc_bad || corrupt_bad || short_rc != P_ENOMEM) ++failures;
    }
    printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
