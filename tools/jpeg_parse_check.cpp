// Stand-alone robustness check of the host JPEG parser (ocr_vi_invoice_amd/csrc/jpeg_parse.h, included alone: no HIP, no library).
// For every file on the command line: the whole file must parse; every prefix must be refused; 2000 seeded single-byte corruptions
// must be refused or give a stream that passes the format's own consistency check.  Inputs and outputs live in heap blocks of their
// exact size, so that a sanitizer build sees any read or write outside them:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_parse_check.cpp -o jpeg_parse_check
//   ./jpeg_parse_check file.jpg ...
//
// Exit status 0 when every expectation held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ocr_vi_invoice_amd/csrc/jpeg_parse.h"

using namespace ocrvi::jpeg;

struct Result { int rc; bool consistent; };

static Result run(const uint8_t* src, size_t n, size_t cap_override = (size_t)-1) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);       // exact size: an over-read is a heap-buffer-overflow
    if (n) memcpy(in, src, n);
    Header h;
    Result r = {parse_headers(n ? in : nullptr, n, h), false};
    if (r.rc == J_OK) {
        const size_t cap = cap_override != (size_t)-1 ? cap_override : (size_t)stream_bound(h, n);
        void* out = malloc(cap ? cap : 1);
        size_t used = 0;
        r.rc = parse_scan(in, n, h, out, cap, &used);
        if (r.rc == J_OK) r.consistent = used <= cap && stream_consistent(out, used, (uint64_t)h.blocks);
        free(out);
    }
    free(in);
    return r;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]); return 2; }
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
        if (whole.rc != J_OK || !whole.consistent) { printf("%s: the whole file does not parse (rc %d)\n", argv[a], whole.rc); ++failures; continue; }
        size_t trunc_bad = 0;
        for (size_t n = 0; n < d.size(); ++n)
            if (run(d.data(), n).rc != J_EINVAL) ++trunc_bad;
        size_t ok = 0, refused = 0, corrupt_bad = 0;
        uint64_t s = 0x9E3779B97F4A7C15ull ^ d.size();
        std::vector<uint8_t> c(d);
        for (int i = 0; i < 2000; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            const size_t p = (size_t)(s % d.size());
            const uint8_t x = (uint8_t)(1 + (s >> 32) % 255);
            c[p] ^= x;
            const Result r = run(c.data(), c.size());
            if (r.rc == J_EINVAL) ++refused;
            else if (r.rc == J_OK && r.consistent) ++ok;
            else ++corrupt_bad;
            c[p] ^= x;
        }
        const int short_rc = run(d.data(), d.size(), 8).rc;      // a cap that cannot hold the offsets
        printf("%s: %zu bytes; %zu prefixes, %zu not refused; 2000 corruptions: %zu refused, %zu parsed consistently, %zu inconsistent; short cap rc %d\n",
               argv[a], d.size(), d.size(), trunc_bad, refused, ok, corrupt_bad, short_rc);
        if (trunc_bad || corrupt_bad || short_rc != J_ENOMEM) ++failures;
    }
    printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
