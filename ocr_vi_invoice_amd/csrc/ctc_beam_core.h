// The acoustic step of the CTC prefix beam search, stated once for ctc_beam.hip and ctc_beam_lm.hip (include/ocrvi.h: with alpha = beta = 0
// the two give the same bytes): the constants, the candidate order and its reductions, the row load, the merge search, the stay
// candidates, the prefix copy, the ids/lens output, and the host checks both entries make.  What the two kernels do differently (how a
// round finds its winner, the LM rows) is in the .hip files.  DESIGN.md section 21 has the pass structure.
//
// Nothing here feeds a floating-point multiply into an add, and nothing may: then the code means the same with and without contraction,
// whatever the including file sets (ctc_beam_lm.hip turns it off below its includes, ctc_beam.hip does not).
#pragma once
#include "common.h"

namespace ocrvi {
namespace ctcbeam {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_W = OCRVI_CTC_BEAM_MAX;      // 64
constexpr int MAX_C = 1024;
constexpr int PER = MAX_C / THREADS;           // classes per thread at the widest row
constexpr size_t LDS_PREFIX_MAX = 32768;       // both prefix tables live in LDS up to this many bytes, in the caller's workspace beyond
typedef unsigned long long u64;
constexpr u64 HASH_EMPTY = 0x243f6a8885a308d3ull;

__host__ __device__ __forceinline__ int stride(int T) { return (T + 1) & ~1; }   // ids of one prefix, int16, padded to whole words

__device__ __forceinline__ double lse(double a, double b) {
    const double m = fmax(a, b);
    if (!(m > -INFINITY)) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}

// The hash of prefix l + c from the hash of l: a filter for the merge search, never the decision (equality of the ids is).
__device__ __forceinline__ u64 hash_ext(u64 h, int c) {
    h = (h ^ (u64)(c + 1)) * 0x9e3779b97f4a7c15ull;
    return h ^ (h >> 29);
}

// A candidate of the selection: its total and its index i * C + c.  Larger total first, equal totals by the smaller index.
struct Cand {
    double tot;
    int idx;    // -1: none
};
__device__ __forceinline__ bool before(double ta, int ia, double tb, int ib) { return ta > tb || (ta == tb && ia < ib); }
__device__ __forceinline__ Cand best(Cand a, Cand b) {
    if (b.idx >= 0 && (a.idx < 0 || before(b.tot, b.idx, a.tot, a.idx))) return b;
    return a;
}
__device__ __forceinline__ Cand wave_best(Cand w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand other;
        other.tot = __shfl_xor(w.tot, o, 64);
        other.idx = __shfl_xor(w.idx, o, 64);
        w = best(w, other);
    }
    return w;
}

struct Table {   // the beam, rank order; two of them, the step reads one and writes the other
    double pb[MAX_W], pnb[MAX_W], s[MAX_W];
    u64 hash[MAX_W];
    int last[MAX_W], len[MAX_W];
};

// A kernel's view of its LDS arrays and of who the thread is.  The arrays stay __shared__ variables of each kernel, declared one by one,
// and the ids are computed once: with the arrays in one struct and the ids taken from threadIdx in every function the kernels measured
// about 1 % slower at W = 1 (profiles/r30_ctc_beam_core.md).  A kernel fills this once and hands it to the functions below.
struct Lds {
    double (*v)[MAX_C];                  // [2]: the log-probabilities of this step and the next
    double *stay_pb, *stay_pnb, *stay_tot;
    int* merge_from;
    unsigned (*excl)[MAX_C / 32];        // [MAX_W]; bit c of row i: extension (i, c) merges into another entry's stay candidate
    double (*red_tot)[WAVES];            // [2]
    int (*red_idx)[WAVES];               // [2]
    int* sel_idx;                        // the selected candidates, rank order
    int b, tid, wave, lane;              // the row (workgroup) and the thread in it
};

// The workgroup's best of round r: every thread gives its own and gets the winner.  One barrier; the slots alternate with r, so round
// r + 1 may write while a slow wave still reads round r.
__device__ __forceinline__ Cand block_best(const Lds& s, Cand mine, int r) {
    Cand w = wave_best(mine);
    if (s.lane == 0) { s.red_tot[r & 1][s.wave] = w.tot; s.red_idx[r & 1][s.wave] = w.idx; }
    __syncthreads();
    w = {s.red_tot[r & 1][0], s.red_idx[r & 1][0]};
#pragma unroll
    for (int k = 1; k < WAVES; ++k) w = best(w, Cand{s.red_tot[r & 1][k], s.red_idx[r & 1][k]});
    return w;
}

__device__ __forceinline__ bool excluded(const Lds& s, int i, int c) { return (s.excl[i][c >> 5] >> (c & 31)) & 1u; }

// prefix tables [2][W][Ts] int16: LDS when they fit, else this row's part of the workspace (flat addressing serves both)
__device__ __forceinline__ int16_t* prefix_tables(unsigned char* smem, int16_t* ws_prefix, int in_lds, int b, int W, int Ts) {
    return in_lds ? (int16_t*)smem : ws_prefix + (size_t)b * 2 * W * Ts;
}

// Row t of this workgroup's line: thread tid holds the classes tid, tid + 256, ...
__device__ __forceinline__ void load_row(const Lds& s, const float* __restrict__ log_probs, int B, int C, int t, float (&r)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = s.tid + k * THREADS;
        r[k] = c < C ? log_probs[((size_t)t * B + s.b) * C + c] : 0.f;
    }
}
__device__ __forceinline__ void store_row(const Lds& s, int buf, int C, const float (&r)[PER]) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = s.tid + k * THREADS;
        if (c < C) s.v[buf][c] = r[k] != r[k] ? -INFINITY : (double)r[k];   // a NaN is probability 0
    }
}

__device__ __forceinline__ void clear_excl(const Lds& s) {
    for (int i = s.tid; i < MAX_W * (MAX_C / 32); i += THREADS) (&s.excl[0][0])[i] = 0u;
}

__device__ __forceinline__ int log2_ceil(int W) {
    int bits = 0;
    while ((1 << bits) < W) ++bits;
    return bits;
}

// The merge search: entry i extended by last(l_j) is entry j, over the pairs (i, j) of a W x 2^jbits grid, jbits = log2_ceil(W).  By
// length, then hash, then the ids.  Leaves merge_from[j] = i (-1: none) and the bit (i, last(l_j)) of excl; the caller's barrier follows.
__device__ __forceinline__ void merge_search(const Lds& s, const Table& tb, const int16_t* pcur, int n, int jbits, int Ts) {
    const int tid = s.tid;
    if (tid < n) s.merge_from[tid] = -1;
    __syncthreads();
    for (int p = tid; p < (n << jbits); p += THREADS) {
        const int i = p >> jbits, j = p & ((1 << jbits) - 1);
        if (j >= n || i == j) continue;
        const int li = tb.len[i];
        if (tb.len[j] != li + 1 || tb.hash[j] != hash_ext(tb.hash[i], tb.last[j])) continue;
        const int16_t* a = pcur + (size_t)i * Ts;
        const int16_t* c = pcur + (size_t)j * Ts;
        bool eq = true;
        for (int q = 0; q < li; ++q) eq = eq && (a[q] == c[q]);
        if (eq) {
            s.merge_from[j] = i;
            atomicOr(&s.excl[i][tb.last[j] >> 5], 1u << (tb.last[j] & 31));
        }
    }
}

// The stay candidates: entry j keeps its prefix, and takes in the entry that merges into it.  The caller's barrier follows.
__device__ __forceinline__ void stay_candidates(const Lds& s, const Table& tb, const double* vt, int n, int blank) {
    if (s.tid < n) {
        const int j = s.tid, lj = tb.last[j], i = s.merge_from[j];
        const double pbn = tb.s[j] + vt[blank];
        double pnbn = lj >= 0 ? tb.pnb[j] + vt[lj] : -INFINITY;
        if (i >= 0) pnbn = lse(pnbn, (lj == tb.last[i] ? tb.pb[i] : tb.s[i]) + vt[lj]);
        s.stay_pb[j] = pbn;
        s.stay_pnb[j] = pnbn;
        s.stay_tot[j] = lse(pbn, pnbn);
    }
}

// The merge bits of this step, cleared by the lanes that know them.
__device__ __forceinline__ void clear_merge_bits(const Lds& s, const Table& tb, int n) {
    const int tid = s.tid;
    if (tid < n && s.merge_from[tid] >= 0) s.excl[s.merge_from[tid]][tb.last[tid] >> 5] = 0u;
}

// The prefixes of the m selected candidates, in rank order: a wave per prefix.
__device__ __forceinline__ void copy_prefixes(const Lds& s, const Table& tb, const int16_t* pcur, int16_t* pnext, int m, int C, int blank,
                                              int Ts) {
    const int wave = s.wave, lane = s.lane;
    for (int r = wave; r < m; r += WAVES) {
        const int i = s.sel_idx[r] / C, c = s.sel_idx[r] - i * C, li = tb.len[i];
        const int16_t* src = pcur + (size_t)i * Ts;
        int16_t* dst = pnext + (size_t)r * Ts;
        for (int q = lane; q < li; q += 64) dst[q] = src[q];
        if (c != blank && lane == 0) dst[li] = (int16_t)c;
    }
}

// Hypothesis r of the output, by one wave: its ids and its length; a missing one (r >= n) is (-1, -1 ...).  Returns the length, 0 if missing.
__device__ __forceinline__ int write_ids_len(const Lds& s, const Table& tb, const int16_t* pcur, int r, int n, int nbest, int T, int Ts,
                                             int32_t* __restrict__ ids, int32_t* __restrict__ lens) {
    const int lane = s.lane;
    const int li = r < n ? tb.len[r] : 0;
    const size_t o = (size_t)s.b * nbest + r;
    for (int q = lane; q < T; q += 64) ids[o * T + q] = q < li ? (int32_t)pcur[(size_t)r * Ts + q] : -1;
    if (lane == 0) lens[o] = r < n ? li : -1;
    return li;
}

// ---------------------------------------------------------------------------------------------------- host
inline int check_shape(const char* who, int T, int B, int C, int beam) {
    OCRVI_CHECK(T >= 1 && T <= OCRVI_CTC_BEAM_MAX_T && B >= 1 && C >= 2 && C <= MAX_C, OCRVI_EINVAL,
                "%s: bad shape T %d B %d C %d (1 <= T <= %d, B >= 1, 2 <= C <= %d)", who, T, B, C, OCRVI_CTC_BEAM_MAX_T, MAX_C);
    OCRVI_CHECK(beam >= 1 && beam <= OCRVI_CTC_BEAM_MAX, OCRVI_EINVAL, "%s: beam %d outside [1, %d]", who, beam, OCRVI_CTC_BEAM_MAX);
    return OCRVI_OK;
}

// the workspace's prefix tables, all rows
inline size_t prefix_bytes(int T, int B, int beam) { return align_up((size_t)B * 2 * beam * stride(T) * sizeof(int16_t), 256); }

// The dynamic LDS of a launch: one row's prefix tables when they fit, else 0 and the kernel takes them from the workspace.
inline size_t prefix_lds_bytes(int T, int beam) {
    const size_t bytes = (size_t)2 * beam * stride(T) * sizeof(int16_t);
    return bytes <= LDS_PREFIX_MAX ? bytes : 0;
}

// The checks both entries make first, in this order: the pointers, the shape (by the entry's own workspace query, which leaves the bytes
// in *need), the blank and nbest.  `who` is the entry's name in the error text.
inline int check_args(const char* who, bool pointers, int (*workspace_bytes)(int, int, int, int, size_t*), int T, int B, int C, int blank_id,
                      int beam, int nbest, size_t* need) {
    OCRVI_CHECK(pointers, OCRVI_EINVAL, "%s: null argument", who);
    OCRVI_TRY(workspace_bytes(T, B, C, beam, need));
    OCRVI_CHECK(blank_id >= 0 && blank_id < C, OCRVI_EINVAL, "%s: blank %d outside [0, %d)", who, blank_id, C);
    OCRVI_CHECK(nbest >= 1 && nbest <= beam, OCRVI_EINVAL, "%s: nbest %d outside [1, beam = %d]", who, nbest, beam);
    return OCRVI_OK;
}

}  // namespace ctcbeam
}  // namespace ocrvi
