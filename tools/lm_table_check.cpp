// Stand-alone check of ocr_vi_invoice_amd/csrc/lm_table.h, the host half of the character n-gram model: builds tables, probes present and
// absent keys, scores strings by hand, and feeds truncated and corrupted blobs to the validator.  No HIP, no libocrvi: meant to run under
// the host sanitizers on a CPU box:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/lm_table_check.cpp -o lm_table_check && ./lm_table_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>

#include "../ocr_vi_invoice_amd/csrc/lm_table.h"

using namespace ocrvi::lm;

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct Grams {
    std::vector<int32_t> ids, lens;
    std::vector<float> lp, bo;
    void add(std::initializer_list<int32_t> g, float l, float b) {
        int32_t row[MAX_ORDER] = {-1, -1, -1, -1, -1, -1};
        int k = 0;
        for (int32_t v : g)
            if (k < MAX_ORDER) row[k++] = v;
        ids.insert(ids.end(), row, row + MAX_ORDER);
        lens.push_back((int32_t)g.size());
        lp.push_back(l);
        bo.push_back(b);
    }
    bool build(int order, int C, int bos, double unk, std::vector<unsigned char>* blob, std::string* err) const {
        return lm_build(ids.data(), lens.data(), lp.data(), bo.data(), lens.size(), order, C, bos, unk, blob, err);
    }
};

// the validator on an exact-size heap copy, so that a read past the end is the sanitizer's to see
static bool valid(const std::vector<unsigned char>& blob, size_t bytes, std::string* err) {
    unsigned char* p = (unsigned char*)malloc(bytes ? bytes : 1);
    memcpy(p, blob.data(), bytes < blob.size() ? bytes : blob.size());
    Header h;
    const bool ok = lm_validate(bytes ? p : nullptr, bytes, &h, err);
    free(p);
    return ok;
}

int main() {
    std::string err;
    std::vector<unsigned char> blob;

    // ---- a hand-made order-4 table: the backoff chain through every level
    Grams g;
    g.add({1}, -1.f, -0.25f); g.add({2}, -1.5f, -0.5f); g.add({3}, -2.f, -0.125f); g.add({4}, -3.f, 0.f); g.add({0}, 0.f, -0.75f);
    g.add({0, 1}, -0.5f, -2.f); g.add({1, 2}, -0.625f, -4.f); g.add({2, 3}, -0.875f, -8.f); g.add({0, 1, 2}, -0.0625f, -16.f);
    g.add({1, 2, 3}, -0.03125f, -32.f); g.add({0, 1, 2, 3}, -0.015625f, 0.f);
    EXPECT(g.build(4, 6, 0, -10.0, &blob, &err));
    EXPECT(blob.size() == blob_bytes(5));                     // 11 entries -> 32 slots
    Header h;
    EXPECT(lm_validate(blob.data(), blob.size(), &h, &err) && h.entries == 11 && h.log2cap == 5);
    std::vector<Slot> slots((size_t)1 << h.log2cap);
    memcpy(slots.data(), blob.data() + sizeof(Header), slots.size() * sizeof(Slot));
    const int32_t present[3] = {1, 2, 3}, absent[3] = {3, 2, 1};
    for (int k = 1; k <= 3; ++k) EXPECT(lm_find(slots.data(), h.log2cap, lm_key(present, k)) != nullptr);
    for (int k = 2; k <= 3; ++k) EXPECT(lm_find(slots.data(), h.log2cap, lm_key(absent, k)) == nullptr);
    const int32_t line[4] = {1, 2, 3, 4}, unk_line[1] = {5}, bad_line[2] = {1, 0};
    double total = 0, terms[4];
    EXPECT(lm_score(slots.data(), h, line, 4, &total, terms, &err));
    EXPECT(terms[0] == -0.5 && terms[1] == -0.0625 && terms[2] == -0.015625 && terms[3] == -43.125 && total == -43.703125);
    EXPECT(lm_score(slots.data(), h, unk_line, 1, &total, nullptr, &err) && total == -10.75);
    EXPECT(lm_score(slots.data(), h, line, 0, &total, nullptr, &err) && total == 0.0);
    EXPECT(!lm_score(slots.data(), h, bad_line, 2, &total, nullptr, &err));

    // ---- random tables at orders 1..6 over 1024 classes: every inserted key is found with its values, random other keys are not
    std::mt19937_64 rng(7);
    for (int order = 1; order <= MAX_ORDER; ++order) {
        Grams r;
        std::vector<uint64_t> keys;
        for (int i = 0; i < 512; ++i) {           // a power of two: the table ends at exactly half load
            int32_t row[MAX_ORDER];
            const int k = 1 + (int)(rng() % order);
            uint64_t key;
            do {
                for (int j = 0; j < k; ++j) row[j] = 1 + (int32_t)(rng() % 1023);
                if (k > 1 && rng() % 4 == 0) row[0] = 0;
                if (rng() % 8 == 0) row[rng() % k] = 1023;
                if (k > 1 && row[k - 1] == 0) row[k - 1] = 1;
                key = lm_key(row, k);
            } while (std::find(keys.begin(), keys.end(), key) != keys.end());
            keys.push_back(key);
            r.ids.insert(r.ids.end(), row, row + MAX_ORDER);
            r.lens.push_back(k);
            r.lp.push_back(-(float)(i + 1) / 64.f);
            r.bo.push_back((float)i / 128.f);
        }
        EXPECT(r.build(order, 1024, 0, -9.0, &blob, &err));
        EXPECT(blob.size() == blob_bytes(10) && valid(blob, blob.size(), &err));
        slots.assign((size_t)1 << 10, Slot{});
        memcpy(slots.data(), blob.data() + sizeof(Header), slots.size() * sizeof(Slot));
        for (size_t i = 0; i < keys.size(); ++i) {
            const Slot* s = lm_find(slots.data(), 10, keys[i]);
            EXPECT(s && s->lp == r.lp[i] && s->bo == r.bo[i]);
        }
        for (int i = 0; i < 2000; ++i) {
            int32_t row[MAX_ORDER];
            const int k = 1 + (int)(rng() % MAX_ORDER);
            for (int j = 0; j < k; ++j) row[j] = 1 + (int32_t)(rng() % 1023);
            const uint64_t key = lm_key(row, k);
            EXPECT((lm_find(slots.data(), 10, key) != nullptr) == (std::find(keys.begin(), keys.end(), key) != keys.end()));
        }
        // ---- truncated and corrupted copies of this blob
        for (size_t cut : {(size_t)0, (size_t)1, sizeof(Header) - 1, sizeof(Header), sizeof(Header) + 15, blob.size() - 16, blob.size() - 1})
            EXPECT(!valid(blob, cut, &err));
        for (int i = 0; i < 400; ++i) {           // one random byte changed: accepted or refused, never a crash or a read outside
            std::vector<unsigned char> c = blob;
            c[rng() % c.size()] ^= (unsigned char)(1u << (rng() % 8));
            (void)valid(c, c.size(), &err);
        }
        for (size_t off = 0; off < sizeof(Header); ++off) {      // every header byte, every bit
            for (int bit = 0; bit < 8; ++bit) {
                std::vector<unsigned char> c = blob;
                c[off] ^= (unsigned char)(1u << bit);
                const bool ok = valid(c, c.size(), &err);
                // magic, version, log2cap and the entry count admit one value; a larger order, another class count or BOS id, unk_lp
                // and the reserved word may still describe a valid table
                EXPECT(!ok || (off >= 8 && off < 20) || off >= 32);
            }
        }
    }

    // ---- what the builder refuses
    struct { std::initializer_list<int32_t> gram; float lp, bo; int order, C, bos; double unk; } bad[] = {
        {{1, 2}, -1.f, 0.f, 1, 4, 0, -5.0},            // longer than the order
        {{4}, -1.f, 0.f, 2, 4, 0, -5.0},               // id >= num_classes
        {{-1}, -1.f, 0.f, 2, 4, 0, -5.0},
        {{1, 0}, -1.f, 0.f, 2, 4, 0, -5.0},            // BOS not first
        {{0}, -1.f, 0.f, 2, 4, 0, -5.0},               // the blank predicted
        {{1}, -INFINITY, 0.f, 2, 4, 0, -5.0}, {{1}, -1.f, NAN, 2, 4, 0, -5.0}, {{1}, -1.f, 0.f, 2, 4, 0, NAN},
        {{1}, -1.f, 0.f, 0, 4, 0, -5.0}, {{1}, -1.f, 0.f, 7, 4, 0, -5.0}, {{1}, -1.f, 0.f, 2, 1, 0, -5.0}, {{1}, -1.f, 0.f, 2, 1025, 0, -5.0},
        {{1}, -1.f, 0.f, 2, 4, 4, -5.0}, {{}, -1.f, 0.f, 2, 4, 0, -5.0},
    };
    for (const auto& b : bad) {
        Grams one;
        one.add(b.gram, b.lp, b.bo);
        err.clear();
        EXPECT(!one.build(b.order, b.C, b.bos, b.unk, &blob, &err) && !err.empty());
    }
    Grams twice;
    twice.add({1, 2}, -1.f, 0.f); twice.add({2}, -1.f, 0.f); twice.add({1, 2}, -2.f, 0.f);
    EXPECT(!twice.build(2, 4, 0, -5.0, &blob, &err) && err.find("twice") != std::string::npos);
    Grams none;
    EXPECT(none.build(1, 2, 0, -5.0, &blob, &err) && blob.size() == blob_bytes(1) && valid(blob, blob.size(), &err));

    printf(failures ? "lm_table_check: %d FAILED\n" : "lm_table_check: ok\n", failures);
    return failures ? 1 : 0;
}
