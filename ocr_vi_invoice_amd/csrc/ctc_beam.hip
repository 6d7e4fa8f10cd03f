// CTC prefix beam search on the device (include/ocrvi.h, "CTC prefix beam search"): one launch carries a beam of prefixes through all T
// steps of every row, in float64.  DESIGN.md section 21 has the pass structure and the measurements.
#include "common.h"

using namespace ocrvi;

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_W = OCRVI_CTC_BEAM_MAX;          // 64
constexpr int CB_MAX_C = 1024;
constexpr int CB_PER = CB_MAX_C / CB_THREADS;     // classes per thread at the widest row
constexpr size_t CB_LDS_PREFIX_MAX = 32768;       // both prefix tables live in LDS up to this many bytes, in the caller's workspace beyond
typedef unsigned long long u64;
constexpr u64 CB_HASH_EMPTY = 0x243f6a8885a308d3ull;

__host__ __device__ __forceinline__ int cb_stride(int T) { return (T + 1) & ~1; }   // ids of one prefix, int16, padded to whole words

__device__ __forceinline__ double cb_lse(double a, double b) {
    const double m = fmax(a, b);
    if (!(m > -INFINITY)) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}

// The hash of prefix l + c from the hash of l: a filter for the merge search, never the decision (equality of the ids is).
__device__ __forceinline__ u64 cb_hash_ext(u64 h, int c) {
    h = (h ^ (u64)(c + 1)) * 0x9e3779b97f4a7c15ull;
    return h ^ (h >> 29);
}

// A candidate of the selection: its total and its index i * C + c.  Larger total first, equal totals by the smaller index.
struct CbCand {
    double tot;
    int idx;    // -1: none
};
__device__ __forceinline__ bool cb_before(double ta, int ia, double tb, int ib) { return ta > tb || (ta == tb && ia < ib); }
__device__ __forceinline__ CbCand cb_best(CbCand a, CbCand b) {
    if (b.idx >= 0 && (a.idx < 0 || cb_before(b.tot, b.idx, a.tot, a.idx))) return b;
    return a;
}

struct CbTable {   // the beam, rank order; two of them, the step reads one and writes the other
    double pb[CB_W], pnb[CB_W], s[CB_W];
    u64 hash[CB_W];
    int last[CB_W], len[CB_W];
};

// One workgroup per row.  Thread tid owns the classes tid, tid + 256, ... of every entry: the candidate (i, c) is one LDS read and one add
// away from the table (only the W stay candidates take a logarithm), so nothing is stored per candidate: a thread keeps a cursor per
// class and recomputes the head of a list after it has been selected.
__global__ __launch_bounds__(CB_THREADS) void ctc_beam_kernel(const float* __restrict__ log_probs, int T, int B, int C, int blank, int W,
                                                             int nbest, int32_t* __restrict__ ids, int32_t* __restrict__ lens,
                                                             double* __restrict__ score, int16_t* __restrict__ ws_prefix, int prefix_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cb_smem[];
    __shared__ double v[2][CB_MAX_C];
    __shared__ CbTable tab[2];
    __shared__ double stay_pb[CB_W], stay_pnb[CB_W], stay_tot[CB_W];
    __shared__ int merge_from[CB_W];
    __shared__ unsigned excl[CB_W][CB_MAX_C / 32];   // bit c of row i: extension (i, c) merges into another entry's stay candidate
    __shared__ double red_tot[2][CB_WAVES];
    __shared__ int red_idx[2][CB_WAVES];
    __shared__ double sel_tot[CB_W];
    __shared__ int sel_idx[CB_W];

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int Ts = cb_stride(T);
    const int cwords = (C + 31) >> 5;
    // prefix tables [2][W][Ts] int16: LDS when they fit, else this row's part of the workspace (flat addressing serves both)
    int16_t* prefix = prefix_in_lds ? (int16_t*)cb_smem : ws_prefix + (size_t)b * 2 * W * Ts;
    int jbits = 0;
    while ((1 << jbits) < W) ++jbits;

    auto load_row = [&](int t, float (&r)[CB_PER]) {
#pragma unroll
        for (int k = 0; k < CB_PER; ++k) {
            const int c = tid + k * CB_THREADS;
            r[k] = c < C ? log_probs[((size_t)t * B + b) * C + c] : 0.f;
        }
    };
    auto store_row = [&](int buf, const float (&r)[CB_PER]) {
#pragma unroll
        for (int k = 0; k < CB_PER; ++k) {
            const int c = tid + k * CB_THREADS;
            if (c < C) v[buf][c] = r[k] != r[k] ? -INFINITY : (double)r[k];   // a NaN is probability 0
        }
    };

    float row[CB_PER];
    load_row(0, row);
    store_row(0, row);
    if (tid == 0) {
        tab[0].pb[0] = 0.0; tab[0].pnb[0] = -INFINITY; tab[0].s[0] = 0.0;
        tab[0].hash[0] = CB_HASH_EMPTY; tab[0].last[0] = -1; tab[0].len[0] = 0;
    }
    for (int i = tid; i < CB_W * (CB_MAX_C / 32); i += CB_THREADS) (&excl[0][0])[i] = 0u;
    int n = 1, cur = 0;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const CbTable& tb = tab[cur];
        CbTable& nx = tab[cur ^ 1];
        const double* vt = v[t & 1];
        const int16_t* pcur = prefix + (size_t)cur * W * Ts;
        int16_t* pnext = prefix + (size_t)(cur ^ 1) * W * Ts;
        if (t + 1 < T) load_row(t + 1, row);   // in flight during the step, stored to LDS at its end

        // ---- merge search: entry i extended by last(l_j) is entry j
        if (tid < n) merge_from[tid] = -1;
        __syncthreads();
        for (int p = tid; p < (n << jbits); p += CB_THREADS) {
            const int i = p >> jbits, j = p & ((1 << jbits) - 1);
            if (j >= n || i == j) continue;
            const int li = tb.len[i];
            if (tb.len[j] != li + 1 || tb.hash[j] != cb_hash_ext(tb.hash[i], tb.last[j])) continue;
            const int16_t* a = pcur + (size_t)i * Ts;
            const int16_t* c = pcur + (size_t)j * Ts;
            bool eq = true;
            for (int q = 0; q < li; ++q) eq = eq && (a[q] == c[q]);
            if (eq) {
                merge_from[j] = i;
                atomicOr(&excl[i][tb.last[j] >> 5], 1u << (tb.last[j] & 31));
            }
        }
        __syncthreads();

        // ---- the stay candidates
        if (tid < n) {
            const int j = tid, lj = tb.last[j], i = merge_from[j];
            const double pbn = tb.s[j] + vt[blank];
            double pnbn = lj >= 0 ? tb.pnb[j] + vt[lj] : -INFINITY;
            if (i >= 0) pnbn = cb_lse(pnbn, (lj == tb.last[i] ? tb.pb[i] : tb.s[i]) + vt[lj]);
            stay_pb[j] = pbn;
            stay_pnb[j] = pnbn;
            stay_tot[j] = cb_lse(pbn, pnbn);
        }
        __syncthreads();

        // ---- selection: W rounds of a workgroup arg-max; after a round only the winner's owner looks at its candidates again
        // The candidates a thread owns.  One irregular candidate at most: thread j < n the stay candidate of entry j, thread 64 + j the
        // repeat extension (j, last(l_j)), taken from pb_j.  And per class c of its own a list: the extensions (i, c) taken from s_i, in
        // rank order, which is their order in the selection (s_i does not increase with i, the add is monotonic, equal totals go by the
        // smaller i).  So a list is a cursor: its head is its best, and a selected head moves it on by one.
        CbCand irr = {-INFINITY, -1};
        if (tid < n) {
            if (stay_tot[tid] > -INFINITY) irr = {stay_tot[tid], tid * C + blank};
        } else if (tid >= CB_W && tid - CB_W < n) {
            const int j = tid - CB_W, c = tb.last[j];
            if (c >= 0 && !((excl[j][c >> 5] >> (c & 31)) & 1u)) {
                const double tot = tb.pb[j] + vt[c];
                if (tot > -INFINITY) irr = {tot, j * C + c};
            }
        }
        int cursor[CB_PER];
        auto skip = [&](int i, int c) -> int {   // the first entry from i on whose extension by c is a candidate of the list
            while (i < n && (tb.last[i] == c || ((excl[i][c >> 5] >> (c & 31)) & 1u))) ++i;
            return i;
        };
#pragma unroll
        for (int k = 0; k < CB_PER; ++k) {
            const int c = tid + k * CB_THREADS;
            cursor[k] = (c < C && c != blank && vt[c] > -INFINITY) ? skip(0, c) : n;
        }
        auto head = [&]() -> CbCand {            // the best of what this thread still owns
            CbCand best = irr;
#pragma unroll
            for (int k = 0; k < CB_PER; ++k) {
                const int c = tid + k * CB_THREADS;
                if (cursor[k] < n) best = cb_best(best, CbCand{tb.s[cursor[k]] + vt[c], cursor[k] * C + c});
            }
            return best;
        };
        auto take = [&](int idx) {               // idx was this thread's head and has been selected
            if (irr.idx == idx) { irr.idx = -1; return; }
#pragma unroll
            for (int k = 0; k < CB_PER; ++k) {
                const int c = tid + k * CB_THREADS;
                if (cursor[k] < n && cursor[k] * C + c == idx) cursor[k] = skip(cursor[k] + 1, c);
            }
        };
        CbCand mine = head();
        int m = 0;
        for (int r = 0; r < W; ++r) {
            CbCand w = mine;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                CbCand other;
                other.tot = __shfl_xor(w.tot, o, 64);
                other.idx = __shfl_xor(w.idx, o, 64);
                w = cb_best(w, other);
            }
            if (lane == 0) { red_tot[r & 1][wave] = w.tot; red_idx[r & 1][wave] = w.idx; }
            __syncthreads();
            w = {red_tot[r & 1][0], red_idx[r & 1][0]};
#pragma unroll
            for (int k = 1; k < CB_WAVES; ++k) w = cb_best(w, CbCand{red_tot[r & 1][k], red_idx[r & 1][k]});
            if (w.idx < 0) break;                         // fewer than W candidates of non-zero probability (uniform)
            if (tid == 0) { sel_tot[r] = w.tot; sel_idx[r] = w.idx; }
            m = r + 1;
            if (mine.idx == w.idx) { take(w.idx); mine = head(); }
        }
        __syncthreads();

        // ---- the next table, in rank order
        if (tid < m) {
            const int r = tid, i = sel_idx[r] / C, c = sel_idx[r] - i * C;
            if (c == blank) {
                nx.pb[r] = stay_pb[i]; nx.pnb[r] = stay_pnb[i]; nx.s[r] = stay_tot[i];
                nx.hash[r] = tb.hash[i]; nx.last[r] = tb.last[i]; nx.len[r] = tb.len[i];
            } else {
                nx.pb[r] = -INFINITY; nx.pnb[r] = sel_tot[r]; nx.s[r] = sel_tot[r];
                nx.hash[r] = cb_hash_ext(tb.hash[i], c); nx.last[r] = c; nx.len[r] = tb.len[i] + 1;
            }
        }
        // the merge bits of this step, cleared by the lanes that know them
        if (tid < n && merge_from[tid] >= 0) excl[merge_from[tid]][tb.last[tid] >> 5] = 0u;
        for (int r = wave; r < m; r += CB_WAVES) {
            const int i = sel_idx[r] / C, c = sel_idx[r] - i * C, li = tb.len[i];
            const int16_t* src = pcur + (size_t)i * Ts;
            int16_t* dst = pnext + (size_t)r * Ts;
            for (int q = lane; q < li; q += 64) dst[q] = src[q];
            if (c != blank && lane == 0) dst[li] = (int16_t)c;
        }
        if (t + 1 < T) store_row((t + 1) & 1, row);
        n = m;
        cur ^= 1;
        __syncthreads();
    }

    // ---- output: the first nbest entries; a missing hypothesis is (-1, -inf, -1 ...)
    const CbTable& tb = tab[cur];
    const int16_t* pcur = prefix + (size_t)cur * W * Ts;
    for (int r = wave; r < nbest; r += CB_WAVES) {
        const int li = r < n ? tb.len[r] : 0;
        int32_t* out = ids + ((size_t)b * nbest + r) * T;
        for (int q = lane; q < T; q += 64) out[q] = q < li ? (int32_t)pcur[(size_t)r * Ts + q] : -1;
        if (lane == 0) {
            lens[(size_t)b * nbest + r] = r < n ? li : -1;
            score[(size_t)b * nbest + r] = r < n ? tb.s[r] : -INFINITY;
        }
    }
}

int cb_check_shape(const char* who, int T, int B, int C, int beam) {
    OCRVI_CHECK(T >= 1 && T <= OCRVI_CTC_BEAM_MAX_T && B >= 1 && C >= 2 && C <= CB_MAX_C, OCRVI_EINVAL,
                "%s: bad shape T %d B %d C %d (1 <= T <= %d, B >= 1, 2 <= C <= %d)", who, T, B, C, OCRVI_CTC_BEAM_MAX_T, CB_MAX_C);
    OCRVI_CHECK(beam >= 1 && beam <= OCRVI_CTC_BEAM_MAX, OCRVI_EINVAL, "%s: beam %d outside [1, %d]", who, beam, OCRVI_CTC_BEAM_MAX);
    return OCRVI_OK;
}

}  // namespace

extern "C" int ocrvi_ctc_beam_workspace_bytes(int T, int B, int C, int beam, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "ctc_beam_workspace_bytes: null out");
    OCRVI_TRY(cb_check_shape("ctc_beam_workspace_bytes", T, B, C, beam));
    *bytes = align_up((size_t)B * 2 * beam * cb_stride(T) * sizeof(int16_t), 256);
    return OCRVI_OK;
}

extern "C" int ocrvi_ctc_beam(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest, int32_t* ids,
                              int32_t* lens, double* score, void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(log_probs && ids && lens && score && workspace, OCRVI_EINVAL, "ctc_beam: null argument");
    size_t need = 0;
    OCRVI_TRY(ocrvi_ctc_beam_workspace_bytes(T, B, C, beam, &need));
    OCRVI_CHECK(blank_id >= 0 && blank_id < C, OCRVI_EINVAL, "ctc_beam: blank %d outside [0, %d)", blank_id, C);
    OCRVI_CHECK(nbest >= 1 && nbest <= beam, OCRVI_EINVAL, "ctc_beam: nbest %d outside [1, beam = %d]", nbest, beam);
    OCRVI_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)score & 7) == 0, OCRVI_EINVAL,
                "ctc_beam: workspace must be 256-byte aligned and score 8-byte aligned");
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "ctc_beam: workspace %zu < %zu bytes", workspace_bytes, need);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t prefix_bytes = (size_t)2 * beam * cb_stride(T) * sizeof(int16_t);
    const int in_lds = prefix_bytes <= CB_LDS_PREFIX_MAX;
    ProfScope ps("ctc_beam", 0.0, (double)T * B * C * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(CB_THREADS), in_lds ? prefix_bytes : 0, (hipStream_t)stream, log_probs, T, B, C, blank_id,
                       beam, nbest, ids, lens, score, (int16_t*)workspace, in_lds);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
