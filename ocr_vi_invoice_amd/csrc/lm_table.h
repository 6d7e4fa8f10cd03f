// The backoff character n-gram table of include/ocrvi.h ("Character n-gram language model"): key packing, the open-addressing table, the
// blob builder, the whole-blob validator and the float64 scorer.  Host C++ only -- no HIP, no libocrvi macros -- so that a stand-alone
// program (tools/lm_table_check.cpp) compiles against it; the device probe of ctc_beam_lm.hip restates lm_home / the probe loop.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace ocrvi {
namespace lm {

constexpr int MAX_ORDER = 6;            // OCRVI_LM_MAX_ORDER
constexpr int MAX_CLASSES = 1024;       // ten bits per symbol
constexpr int MAX_LOG2CAP = 40;
constexpr uint32_t MAGIC = 0x4d4c434fu; // "OCLM"
constexpr uint32_t VERSION = 1;
constexpr uint64_t HASH_MUL = 0x9e3779b97f4a7c15ull;

struct Slot {      // 16 bytes; key 0 = empty
    uint64_t key;
    float lp, bo;
};
struct Header {    // 48 bytes, then (1 << log2cap) slots
    uint32_t magic, version;
    int32_t order, num_classes, bos_id, log2cap;
    uint64_t entries;
    double unk_lp;
    uint64_t reserved;
};
static_assert(sizeof(Slot) == 16 && sizeof(Header) == 48, "lm blob layout");

inline size_t blob_bytes(int log2cap) { return sizeof(Header) + (sizeof(Slot) << log2cap); }

// g_1..g_k -> (k << 60) | sum g_j << (10 (j - 1)): the identity of the n-gram, never 0
inline uint64_t lm_key(const int32_t* g, int k) {
    uint64_t key = (uint64_t)k << 60;
    for (int j = 0; j < k; ++j) key |= (uint64_t)g[j] << (10 * j);
    return key;
}
inline uint64_t lm_home(uint64_t key, int log2cap) { return (key * HASH_MUL) >> (64 - log2cap); }

// The slot that holds `key`, or null.  Ends because a valid table has an empty slot.
inline const Slot* lm_find(const Slot* slots, int log2cap, uint64_t key) {
    const uint64_t mask = ((uint64_t)1 << log2cap) - 1;
    for (uint64_t at = lm_home(key, log2cap);; at = (at + 1) & mask) {
        if (slots[at].key == key) return slots + at;
        if (slots[at].key == 0) return nullptr;
    }
}

// What a key may look like in a table of this order / class count; `why` names the first rule it breaks.
inline bool lm_key_ok(uint64_t key, float lp, int order, int num_classes, int bos_id, const char** why) {
    const int k = (int)(key >> 60);
    if ((key >> 63) || k < 1 || k > order) { *why = "length tag outside 1..order"; return false; }
    if (k < MAX_ORDER && ((key & (((uint64_t)1 << 60) - 1)) >> (10 * k))) { *why = "bits set beyond the gram's symbols"; return false; }
    for (int j = 0; j < k; ++j) {
        const int id = (int)((key >> (10 * j)) & 1023);
        if (id >= num_classes) { *why = "symbol id >= num_classes"; return false; }
        if (id == bos_id && j > 0) { *why = "BOS (the blank id) anywhere but first"; return false; }
    }
    if (k == 1 && (int)(key & 1023) == bos_id && lp != 0.f) { *why = "blank as a predicted symbol (the 1-gram BOS is a context: its lp is 0)"; return false; }
    return true;
}

inline bool lm_header_ok(const Header& h, size_t bytes, std::string* err) {
    if (h.magic != MAGIC || h.version != VERSION) { *err = "bad magic / version"; return false; }
    if (h.order < 1 || h.order > MAX_ORDER) { *err = "order outside 1..6"; return false; }
    if (h.num_classes < 2 || h.num_classes > MAX_CLASSES) { *err = "num_classes outside 2..1024"; return false; }
    if (h.bos_id < 0 || h.bos_id >= h.num_classes) { *err = "bos_id outside [0, num_classes)"; return false; }
    if (h.log2cap < 1 || h.log2cap > MAX_LOG2CAP) { *err = "log2cap outside 1..40"; return false; }
    if (bytes != blob_bytes(h.log2cap)) { *err = "blob size is not header + (1 << log2cap) slots"; return false; }
    if (h.entries > (((uint64_t)1 << h.log2cap) >> 1)) { *err = "more entries than half the capacity"; return false; }
    if (!isfinite(h.unk_lp)) { *err = "unk_lp is not finite"; return false; }
    return true;
}

// The whole blob: header, capacity, load, every key's length tag and ids, finite values, and every key where a probe finds it (so no
// key twice).  After it the probe loop needs no bounds or sanity check.  The blob need not be aligned.
inline bool lm_validate(const void* blob, size_t bytes, Header* out, std::string* err) {
    if (!blob || bytes < sizeof(Header)) { *err = "blob shorter than its header"; return false; }
    Header h;
    memcpy(&h, blob, sizeof(h));
    if (!lm_header_ok(h, bytes, err)) return false;
    const uint64_t cap = (uint64_t)1 << h.log2cap;
    std::vector<Slot> slots(cap);
    memcpy(slots.data(), (const char*)blob + sizeof(Header), cap * sizeof(Slot));
    uint64_t used = 0;
    for (uint64_t i = 0; i < cap; ++i) {
        const Slot& s = slots[i];
        if (s.key == 0) continue;
        ++used;
        const char* why = "";
        if (!lm_key_ok(s.key, s.lp, h.order, h.num_classes, h.bos_id, &why)) { *err = std::string("slot key: ") + why; return false; }
        if (!isfinite(s.lp) || !isfinite(s.bo)) { *err = "a slot's lp / bo is not finite"; return false; }
    }
    if (used != h.entries) { *err = "entry count differs from the occupied slots"; return false; }
    for (uint64_t i = 0; i < cap; ++i)
        if (slots[i].key && lm_find(slots.data(), h.log2cap, slots[i].key) != &slots[i]) { *err = "a key is not where a probe finds it"; return false; }
    if (out) *out = h;
    return true;
}

// ids [n][MAX_ORDER] (entries beyond lens[i] ignored), lp / bo [n].  Inserted in the given order.
inline bool lm_build(const int32_t* ids, const int32_t* lens, const float* lp, const float* bo, size_t n, int order, int num_classes, int bos_id,
                     double unk_lp, std::vector<unsigned char>* blob, std::string* err) {
    Header h{};
    h.magic = MAGIC; h.version = VERSION; h.order = order; h.num_classes = num_classes; h.bos_id = bos_id; h.entries = n; h.unk_lp = unk_lp;
    h.log2cap = 1;
    while (h.log2cap < MAX_LOG2CAP && ((uint64_t)1 << h.log2cap) < 2 * (uint64_t)n) ++h.log2cap;
    if (!lm_header_ok(h, blob_bytes(h.log2cap), err)) return false;
    if (n && !(ids && lens && lp && bo)) { *err = "null gram arrays"; return false; }
    const uint64_t cap = (uint64_t)1 << h.log2cap, mask = cap - 1;
    std::vector<Slot> slots(cap, Slot{0, 0.f, 0.f});
    for (size_t i = 0; i < n; ++i) {
        const int k = lens[i];
        const int32_t* g = ids + i * MAX_ORDER;
        if (k < 1 || k > order) { *err = "gram " + std::to_string(i) + ": length outside 1..order"; return false; }
        for (int j = 0; j < k; ++j)
            if (g[j] < 0 || g[j] >= num_classes) { *err = "gram " + std::to_string(i) + ": symbol id outside [0, num_classes)"; return false; }
        if (!isfinite(lp[i]) || !isfinite(bo[i])) { *err = "gram " + std::to_string(i) + ": lp / bo is not finite"; return false; }
        const uint64_t key = lm_key(g, k);
        const char* why = "";
        if (!lm_key_ok(key, lp[i], order, num_classes, bos_id, &why)) { *err = "gram " + std::to_string(i) + ": " + why; return false; }
        uint64_t at = lm_home(key, h.log2cap);
        for (; slots[at].key; at = (at + 1) & mask)
            if (slots[at].key == key) { *err = "gram " + std::to_string(i) + ": given twice"; return false; }
        slots[at] = Slot{key, lp[i], bo[i]};
    }
    blob->resize(blob_bytes(h.log2cap));
    memcpy(blob->data(), &h, sizeof(h));
    memcpy(blob->data() + sizeof(h), slots.data(), cap * sizeof(Slot));
    return true;
}

// lm(c | h), h the context's k0 symbols (oldest first): the backoff chain of the header, float64.
inline double lm_cond(const Slot* slots, const Header& h, const int32_t* ctx, int k0, int c) {
    double acc = 0.0;
    int32_t g[MAX_ORDER];
    for (int k = k0; k >= 0; --k) {
        for (int j = 0; j < k; ++j) g[j] = ctx[k0 - k + j];
        g[k] = c;
        if (const Slot* s = lm_find(slots, h.log2cap, lm_key(g, k + 1))) return acc + (double)s->lp;
        if (k >= 1)
            if (const Slot* s = lm_find(slots, h.log2cap, lm_key(g, k))) acc += (double)s->bo;
    }
    return acc + h.unk_lp;
}

// g(ids[0..len)) and, when per_char is not null, each character's term.  `slots` / `h` of a validated blob.
inline bool lm_score(const Slot* slots, const Header& h, const int32_t* ids, int len, double* total, double* per_char, std::string* err) {
    int32_t ctx[MAX_ORDER];
    int k0 = 0;
    if (h.order > 1) ctx[k0++] = h.bos_id;
    double g = 0.0;
    for (int q = 0; q < len; ++q) {
        const int c = ids[q];
        if (c < 0 || c >= h.num_classes || c == h.bos_id) { *err = "id " + std::to_string(c) + " at " + std::to_string(q) + " is no label"; return false; }
        const double term = lm_cond(slots, h, ctx, k0, c);
        if (per_char) per_char[q] = term;
        g += term;
        if (h.order > 1) {
            if (k0 == h.order - 1) memmove(ctx, ctx + 1, (k0 - 1) * sizeof(int32_t)), --k0;
            ctx[k0++] = c;
        }
    }
    *total = g;
    return true;
}

}  // namespace lm
}  // namespace ocrvi
