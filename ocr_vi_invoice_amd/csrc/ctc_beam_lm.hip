// CTC prefix beam search with a character n-gram model fused in (include/ocrvi.h, "Character n-gram language model" and "CTC prefix beam
// search with LM fusion"): the model's host entries and handle, and the search kernel.  DESIGN.md section 22 has the selection scheme, the
// workspace and the measurements.  The acoustic half restates ctc_beam.hip expression for expression: with alpha = beta = 0 the two give
// the same bytes.
#include "lm_table.h"
#include "model.h"

// R = (s + alpha g) + beta len with every product and sum rounded on its own
#pragma clang fp contract(off)

using namespace ocrvi;

constexpr uint64_t LM_HANDLE_MAGIC = 0x6f6372766c6d6831ull;

struct ocrvi_lm {
    uint64_t magic = LM_HANDLE_MAGIC;
    int device = 0;
    lm::Header hdr{};
    DeviceStore store;
    const lm::Slot* slots = nullptr;   // device
};

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_W = OCRVI_CTC_BEAM_MAX;          // 64
constexpr int CL_MAX_C = 1024;
constexpr int CL_PER = CL_MAX_C / CL_THREADS;     // classes per thread at the widest row
constexpr int CL_BATCH = 8;                       // LM terms in flight per class during the first scan of a step
constexpr size_t CL_LDS_PREFIX_MAX = 32768;       // as ctc_beam.hip
typedef unsigned long long u64;
constexpr u64 CL_HASH_EMPTY = 0x243f6a8885a308d3ull;

__host__ __device__ __forceinline__ int cl_stride(int T) { return (T + 1) & ~1; }

__device__ __forceinline__ double cl_lse(double a, double b) {
    const double m = fmax(a, b);
    if (!(m > -INFINITY)) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}
__device__ __forceinline__ u64 cl_hash_ext(u64 h, int c) {
    h = (h ^ (u64)(c + 1)) * 0x9e3779b97f4a7c15ull;
    return h ^ (h >> 29);
}

struct ClCand {
    double tot;   // the rank total R
    int idx;      // i * C + c; -1: none
};
__device__ __forceinline__ bool cl_before(double ta, int ia, double tb, int ib) { return ta > tb || (ta == tb && ia < ib); }
__device__ __forceinline__ ClCand cl_best(ClCand a, ClCand b) {
    if (b.idx >= 0 && (a.idx < 0 || cl_before(b.tot, b.idx, a.tot, a.idx))) return b;
    return a;
}
__device__ __forceinline__ ClCand cl_wave_best(ClCand w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ClCand other;
        other.tot = __shfl_xor(w.tot, o, 64);
        other.idx = __shfl_xor(w.idx, o, 64);
        w = cl_best(w, other);
    }
    return w;
}

struct ClTable {   // the beam, rank order
    double pb[CL_W], pnb[CL_W], s[CL_W], g[CL_W];
    u64 hash[CL_W], ctx[CL_W];      // ctx: the LM context's symbols, oldest in the low ten bits
    int last[CL_W], len[CL_W], hlen[CL_W], slot[CL_W];   // hlen: symbols in ctx; slot: this prefix's row of LM terms in the workspace
};

struct ClLm {
    const lm::Slot* slots;
    int log2cap, order, bos;
    double unk_lp;
};

// 16-byte probe of the read-only table; ends because ocrvi_lm_create saw an empty slot
__device__ __forceinline__ bool cl_find(const ClLm& m, u64 key, float* lp, float* bo) {
    const u64 mask = ((u64)1 << m.log2cap) - 1;
    for (u64 at = (key * lm::HASH_MUL) >> (64 - m.log2cap);; at = (at + 1) & mask) {
        const uint4 q = *(const uint4*)(m.slots + at);
        const u64 k = (u64)q.x | ((u64)q.y << 32);
        if (k == key) { *lp = __uint_as_float(q.z); *bo = __uint_as_float(q.w); return true; }
        if (k == 0) return false;
    }
}

// One workgroup per row.  Thread tid owns the classes tid, tid + 256, ...: of each it keeps the best candidate over the entries i and
// the set of entries already selected.  A round is one workgroup arg-max over those; then the wave of the winning class's owner scans
// that one class again, lane i the candidate (i, c).
__global__ __launch_bounds__(CL_THREADS) void ctc_beam_lm_kernel(const float* __restrict__ log_probs, int T, int B, int C, int blank, int W,
                                                                int nbest, ClLm lmod, double alpha, double beta, int32_t* __restrict__ ids,
                                                                int32_t* __restrict__ lens, double* __restrict__ score,
                                                                double* __restrict__ ctc_score, double* __restrict__ lm_score,
                                                                int16_t* __restrict__ ws_prefix, double* ws_rows, int prefix_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
    __shared__ double v[2][CL_MAX_C];
    __shared__ double uni[CL_MAX_C];                  // the unigram level: lp of (c), unk_lp where there is none
    __shared__ ClTable tab[2];
    __shared__ double stay_pb[CL_W], stay_pnb[CL_W], stay_tot[CL_W];
    __shared__ int merge_from[CL_W];
    __shared__ unsigned excl[CL_W][CL_MAX_C / 32];
    __shared__ double red_tot[2][CL_WAVES];
    __shared__ int red_idx[2][CL_WAVES];
    __shared__ int sel_idx[CL_W];
    __shared__ int ext_rank[CL_W];                    // the ranks of the next table's new prefixes
    __shared__ double ext_acc[CL_W][lm::MAX_ORDER];   // [e][k]: the backoff weights summed before level k is tried
    __shared__ u64 used_slots;
    __shared__ int n_ext_s;

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int Ts = cl_stride(T);
    int16_t* prefix = prefix_in_lds ? (int16_t*)cl_smem : ws_prefix + (size_t)b * 2 * W * Ts;
    double* rows = ws_rows + (size_t)b * W * C;       // [W][C]: row `slot` holds lm(c | ctx) of the prefix that owns the slot
    int jbits = 0;
    while ((1 << jbits) < W) ++jbits;

    auto load_row = [&](int t, float (&r)[CL_PER]) {
#pragma unroll
        for (int k = 0; k < CL_PER; ++k) {
            const int c = tid + k * CL_THREADS;
            r[k] = c < C ? log_probs[((size_t)t * B + b) * C + c] : 0.f;
        }
    };
    auto store_row = [&](int buf, const float (&r)[CL_PER]) {
#pragma unroll
        for (int k = 0; k < CL_PER; ++k) {
            const int c = tid + k * CL_THREADS;
            if (c < C) v[buf][c] = r[k] != r[k] ? -INFINITY : (double)r[k];
        }
    };
    // The rows of LM terms of the n_ext new prefixes ext_rank[0..n_ext) of table tn.  First each context's backoff weights, one probe per
    // (prefix, level); then one thread per (prefix, class) walks down from the longest gram to the bigram; the unigram level is in LDS.
    auto fill_rows = [&](const ClTable& tn, int n_ext) {
        for (int p = tid; p < n_ext * lm::MAX_ORDER; p += CL_THREADS) {
            const int e = p / lm::MAX_ORDER, k = p - e * lm::MAX_ORDER, r = ext_rank[e], H = tn.hlen[r];
            double w = 0.0;
            if (k >= 1 && k <= H) {
                float lp, bo;
                if (cl_find(lmod, ((u64)k << 60) | (tn.ctx[r] >> (10 * (H - k))), &lp, &bo)) w = (double)bo;
            }
            ext_acc[e][k] = w;                       // for now the weight of level k itself (0 where the context is absent)
        }
        __syncthreads();
        if (tid < n_ext) {                           // acc before level k: the weights of the levels above it, added longest first
            const int H = tn.hlen[ext_rank[tid]];
            double acc = 0.0;
            for (int k = H; k >= 1; --k) {
                const double w = ext_acc[tid][k];
                ext_acc[tid][k] = acc;
                acc = acc + w;
            }
            ext_acc[tid][0] = acc;
        }
        __syncthreads();
        for (int p = tid; p < n_ext * C; p += CL_THREADS) {
            const int e = p / C, c = p - e * C, r = ext_rank[e], H = tn.hlen[r];
            if (c == blank) continue;
            const u64 ctx = tn.ctx[r];
            double term = ext_acc[e][0] + uni[c];
            for (int k = H; k >= 1; --k) {
                float lp, bo;
                if (cl_find(lmod, ((u64)(k + 1) << 60) | (ctx >> (10 * (H - k))) | ((u64)c << (10 * k)), &lp, &bo)) {
                    term = ext_acc[e][k] + (double)lp;
                    break;
                }
            }
            rows[(size_t)tn.slot[r] * C + c] = term;
        }
    };

    float row[CL_PER];
    load_row(0, row);
    store_row(0, row);
    for (int c = tid; c < C; c += CL_THREADS) {
        float lp, bo;
        uni[c] = (c != blank && cl_find(lmod, ((u64)1 << 60) | (u64)c, &lp, &bo)) ? (double)lp : lmod.unk_lp;
    }
    if (tid == 0) {
        ClTable& t0 = tab[0];
        t0.pb[0] = 0.0; t0.pnb[0] = -INFINITY; t0.s[0] = 0.0; t0.g[0] = 0.0;
        t0.hash[0] = CL_HASH_EMPTY; t0.last[0] = -1; t0.len[0] = 0; t0.slot[0] = 0;
        t0.hlen[0] = lmod.order > 1 ? 1 : 0;
        t0.ctx[0] = lmod.order > 1 ? (u64)lmod.bos : 0;
        ext_rank[0] = 0;
    }
    for (int i = tid; i < CL_W * (CL_MAX_C / 32); i += CL_THREADS) (&excl[0][0])[i] = 0u;
    int n = 1, cur = 0;
    __syncthreads();
    fill_rows(tab[0], 1);
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const ClTable& tb = tab[cur];
        ClTable& nx = tab[cur ^ 1];
        const double* vt = v[t & 1];
        const int16_t* pcur = prefix + (size_t)cur * W * Ts;
        int16_t* pnext = prefix + (size_t)(cur ^ 1) * W * Ts;
        if (t + 1 < T) load_row(t + 1, row);

        // ---- merge search: entry i extended by last(l_j) is entry j
        if (tid < n) merge_from[tid] = -1;
        __syncthreads();
        for (int p = tid; p < (n << jbits); p += CL_THREADS) {
            const int i = p >> jbits, j = p & ((1 << jbits) - 1);
            if (j >= n || i == j) continue;
            const int li = tb.len[i];
            if (tb.len[j] != li + 1 || tb.hash[j] != cl_hash_ext(tb.hash[i], tb.last[j])) continue;
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
            if (i >= 0) pnbn = cl_lse(pnbn, (lj == tb.last[i] ? tb.pb[i] : tb.s[i]) + vt[lj]);
            stay_pb[j] = pbn;
            stay_pnb[j] = pnbn;
            stay_tot[j] = cl_lse(pbn, pnbn);
        }
        __syncthreads();

        // ---- selection
        // The acoustic total of the extension (i, c), c != blank; -inf where it merged into another entry's stay candidate.
        auto ext_acoustic = [&](int i, int c) -> double {
            if ((excl[i][c >> 5] >> (c & 31)) & 1u) return -INFINITY;
            return (c == tb.last[i] ? tb.pb[i] : tb.s[i]) + vt[c];
        };
        auto rank_total = [&](double a, double g, int len) -> double { return (a + alpha * g) + beta * (double)len; };
        auto cand = [&](int i, int c, double term) -> ClCand {
            double a, g;
            int len;
            if (c == blank) { a = stay_tot[i]; g = tb.g[i]; len = tb.len[i]; }
            else { a = ext_acoustic(i, c); g = tb.g[i] + term; len = tb.len[i] + 1; }
            if (!(a > -INFINITY)) return ClCand{-INFINITY, -1};
            return ClCand{rank_total(a, g, len), i * C + c};
        };
        ClCand best[CL_PER];
        u64 taken[CL_PER];
#pragma unroll
        for (int k = 0; k < CL_PER; ++k) {
            const int c = tid + k * CL_THREADS;
            best[k] = ClCand{-INFINITY, -1};
            taken[k] = 0;
            if (c >= C || (c != blank && !(vt[c] > -INFINITY))) continue;
            for (int i0 = 0; i0 < n; i0 += CL_BATCH) {
                double term[CL_BATCH];
#pragma unroll
                for (int u = 0; u < CL_BATCH; ++u) term[u] = c == blank ? 0.0 : rows[(size_t)tb.slot[min(i0 + u, n - 1)] * C + c];
#pragma unroll
                for (int u = 0; u < CL_BATCH; ++u)
                    if (i0 + u < n) best[k] = cl_best(best[k], cand(i0 + u, c, term[u]));
            }
        }
        int m = 0;
        for (int r = 0; r < W; ++r) {
            ClCand mine = best[0];
#pragma unroll
            for (int k = 1; k < CL_PER; ++k) mine = cl_best(mine, best[k]);
            ClCand w = cl_wave_best(mine);
            if (lane == 0) { red_tot[r & 1][wave] = w.tot; red_idx[r & 1][wave] = w.idx; }
            __syncthreads();
            w = {red_tot[r & 1][0], red_idx[r & 1][0]};
#pragma unroll
            for (int k = 1; k < CL_WAVES; ++k) w = cl_best(w, ClCand{red_tot[r & 1][k], red_idx[r & 1][k]});
            if (w.idx < 0) break;                         // fewer than W candidates of non-zero probability (uniform)
            if (tid == 0) sel_idx[r] = w.idx;
            m = r + 1;
            // the winner's class again, without what has been selected of it: the owner's wave, lane i the entry i (wave-uniform branch)
            const int wi = w.idx / C, wc = w.idx - wi * C, owner = wc & (CL_THREADS - 1), wk = wc / CL_THREADS;
            if (wave == (owner >> 6)) {
                u64 tk = 0;
#pragma unroll
                for (int k = 0; k < CL_PER; ++k)
                    if (k == wk) tk = taken[k];
                tk = (u64)__shfl((unsigned)tk, owner & 63, 64) | ((u64)__shfl((unsigned)(tk >> 32), owner & 63, 64) << 32);
                tk |= (u64)1 << wi;
                ClCand again = {-INFINITY, -1};
                if (lane < n && !((tk >> lane) & 1)) again = cand(lane, wc, wc == blank ? 0.0 : rows[(size_t)tb.slot[lane] * C + wc]);
                again = cl_wave_best(again);
                if (tid == owner) {
#pragma unroll
                    for (int k = 0; k < CL_PER; ++k)
                        if (k == wk) { taken[k] = tk; best[k] = again; }
                }
            }
        }
        __syncthreads();

        // ---- the next table, in rank order; a new prefix takes the lowest row slot no surviving prefix holds
        if (tid == 0) used_slots = 0;
        __syncthreads();
        {
            const int r = tid;                            // (m <= 64: the lanes of wave 0)
            bool is_ext = false;
            int i = 0, c = 0;
            if (r < m) {
                i = sel_idx[r] / C; c = sel_idx[r] - i * C;
                is_ext = c != blank;
                if (!is_ext) atomicOr(&used_slots, (u64)1 << tb.slot[i]);
            }
            const u64 ext_mask = __builtin_amdgcn_ballot_w64(is_ext);
            __syncthreads();
            if (r < m) {
                if (!is_ext) {
                    nx.pb[r] = stay_pb[i]; nx.pnb[r] = stay_pnb[i]; nx.s[r] = stay_tot[i]; nx.g[r] = tb.g[i];
                    nx.hash[r] = tb.hash[i]; nx.ctx[r] = tb.ctx[i]; nx.last[r] = tb.last[i]; nx.len[r] = tb.len[i];
                    nx.hlen[r] = tb.hlen[i]; nx.slot[r] = tb.slot[i];
                } else {
                    const int e = __popcll(ext_mask & (((u64)1 << r) - 1));
                    u64 free_slots = ~used_slots;
                    for (int q = 0; q < e; ++q) free_slots &= free_slots - 1;
                    const int slot = __ffsll((long long)free_slots) - 1;     // < W: stays + new prefixes <= W
                    const double a = ext_acoustic(i, c);
                    const int H = tb.hlen[i];
                    nx.pb[r] = -INFINITY; nx.pnb[r] = a; nx.s[r] = a; nx.g[r] = tb.g[i] + rows[(size_t)tb.slot[i] * C + c];
                    nx.hash[r] = cl_hash_ext(tb.hash[i], c); nx.last[r] = c; nx.len[r] = tb.len[i] + 1; nx.slot[r] = slot;
                    if (lmod.order == 1) { nx.ctx[r] = 0; nx.hlen[r] = 0; }
                    else if (H < lmod.order - 1) { nx.ctx[r] = tb.ctx[i] | ((u64)c << (10 * H)); nx.hlen[r] = H + 1; }
                    else { nx.ctx[r] = (tb.ctx[i] >> 10) | ((u64)c << (10 * (H - 1))); nx.hlen[r] = H; }
                    ext_rank[e] = r;
                }
            }
            if (tid == 0) n_ext_s = __popcll(ext_mask);
        }
        __syncthreads();
        // the merge bits of this step, cleared by the lanes that know them
        if (tid < n && merge_from[tid] >= 0) excl[merge_from[tid]][tb.last[tid] >> 5] = 0u;
        for (int r = wave; r < m; r += CL_WAVES) {
            const int i = sel_idx[r] / C, c = sel_idx[r] - i * C, li = tb.len[i];
            const int16_t* src = pcur + (size_t)i * Ts;
            int16_t* dst = pnext + (size_t)r * Ts;
            for (int q = lane; q < li; q += 64) dst[q] = src[q];
            if (c != blank && lane == 0) dst[li] = (int16_t)c;
        }
        if (t + 1 < T) store_row((t + 1) & 1, row);
        fill_rows(nx, n_ext_s);                           // (every selected candidate has been read: the rows of dropped prefixes are free)
        n = m;
        cur ^= 1;
        __syncthreads();
    }

    // ---- output: the first nbest entries; a missing hypothesis is (-1, -inf, -inf, -inf, -1 ...)
    const ClTable& tb = tab[cur];
    const int16_t* pcur = prefix + (size_t)cur * W * Ts;
    for (int r = wave; r < nbest; r += CL_WAVES) {
        const int li = r < n ? tb.len[r] : 0;
        int32_t* out = ids + ((size_t)b * nbest + r) * T;
        for (int q = lane; q < T; q += 64) out[q] = q < li ? (int32_t)pcur[(size_t)r * Ts + q] : -1;
        if (lane == 0) {
            const size_t o = (size_t)b * nbest + r;
            lens[o] = r < n ? li : -1;
            score[o] = r < n ? (tb.s[r] + alpha * tb.g[r]) + beta * (double)li : -INFINITY;
            ctc_score[o] = r < n ? tb.s[r] : -INFINITY;
            lm_score[o] = r < n ? tb.g[r] : -INFINITY;
        }
    }
}

int cl_check_shape(const char* who, int T, int B, int C, int beam) {
    OCRVI_CHECK(T >= 1 && T <= OCRVI_CTC_BEAM_MAX_T && B >= 1 && C >= 2 && C <= CL_MAX_C, OCRVI_EINVAL,
                "%s: bad shape T %d B %d C %d (1 <= T <= %d, B >= 1, 2 <= C <= %d)", who, T, B, C, OCRVI_CTC_BEAM_MAX_T, CL_MAX_C);
    OCRVI_CHECK(beam >= 1 && beam <= OCRVI_CTC_BEAM_MAX, OCRVI_EINVAL, "%s: beam %d outside [1, %d]", who, beam, OCRVI_CTC_BEAM_MAX);
    return OCRVI_OK;
}
size_t cl_prefix_bytes(int T, int B, int beam) { return align_up((size_t)B * 2 * beam * cl_stride(T) * sizeof(int16_t), 256); }

}  // namespace

// ---------------------------------------------------------------------------------------------------- the model: host entries
extern "C" int ocrvi_lm_build(const int32_t* gram_ids, const int32_t* gram_lens, const float* lp, const float* bo, size_t n_grams, int order,
                              int num_classes, int bos_id, double unk_lp, void* blob, size_t blob_capacity, size_t* blob_bytes) {
    OCRVI_CHECK(blob_bytes, OCRVI_EINVAL, "lm_build: null out");
    std::vector<unsigned char> out;
    std::string err;
    OCRVI_CHECK(lm::lm_build(gram_ids, gram_lens, lp, bo, n_grams, order, num_classes, bos_id, unk_lp, &out, &err), OCRVI_EINVAL, "lm_build: %s",
                err.c_str());
    *blob_bytes = out.size();
    if (!blob) return OCRVI_OK;                        // the size query
    OCRVI_CHECK(blob_capacity >= out.size(), OCRVI_ENOMEM, "lm_build: blob buffer %zu < %zu bytes", blob_capacity, out.size());
    memcpy(blob, out.data(), out.size());
    return OCRVI_OK;
}

extern "C" int ocrvi_lm_score(const void* blob, size_t blob_bytes, const int32_t* ids, int len, double* total, double* per_char) {
    OCRVI_CHECK(total && len >= 0 && (ids || len == 0), OCRVI_EINVAL, "lm_score: null argument or negative length");
    lm::Header h;
    std::string err;
    OCRVI_CHECK(lm::lm_validate(blob, blob_bytes, &h, &err), OCRVI_EINVAL, "lm_score: %s", err.c_str());
    std::vector<lm::Slot> slots((size_t)1 << h.log2cap);   // (the caller's blob need not be aligned)
    memcpy(slots.data(), (const char*)blob + sizeof(lm::Header), slots.size() * sizeof(lm::Slot));
    OCRVI_CHECK(lm::lm_score(slots.data(), h, ids, len, total, per_char, &err), OCRVI_EINVAL, "lm_score: %s", err.c_str());
    return OCRVI_OK;
}

extern "C" int ocrvi_lm_create(int device, const void* blob, size_t blob_bytes, ocrvi_lm** out) {
    OCRVI_CHECK(out, OCRVI_EINVAL, "lm_create: null out");
    lm::Header h;
    std::string err;
    OCRVI_CHECK(lm::lm_validate(blob, blob_bytes, &h, &err), OCRVI_EINVAL, "lm_create: %s", err.c_str());
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    ocrvi_lm* m = new ocrvi_lm;
    m->device = device;
    m->hdr = h;
    void* d = nullptr;
    const int rc = m->store.upload((const char*)blob + sizeof(lm::Header), blob_bytes - sizeof(lm::Header), &d);
    if (rc != OCRVI_OK) {
        delete m;
        return rc;
    }
    m->slots = (const lm::Slot*)d;
    *out = m;
    return OCRVI_OK;
}

extern "C" void ocrvi_lm_destroy(ocrvi_lm* h) {
    if (!h || h->magic != LM_HANDLE_MAGIC) return;
    h->magic = 0;
    delete h;
}

// ---------------------------------------------------------------------------------------------------- the search
extern "C" int ocrvi_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "ctc_beam_lm_workspace_bytes: null out");
    OCRVI_TRY(cl_check_shape("ctc_beam_lm_workspace_bytes", T, B, C, beam));
    *bytes = cl_prefix_bytes(T, B, beam) + align_up((size_t)B * beam * C * sizeof(double), 256);
    return OCRVI_OK;
}

extern "C" int ocrvi_ctc_beam_lm(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest, const ocrvi_lm* lmh,
                                 double alpha, double beta, int32_t* ids, int32_t* lens, double* score, double* ctc_score, double* lm_score,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(log_probs && ids && lens && score && ctc_score && lm_score && workspace, OCRVI_EINVAL, "ctc_beam_lm: null argument");
    size_t need = 0;
    OCRVI_TRY(ocrvi_ctc_beam_lm_workspace_bytes(T, B, C, beam, &need));
    OCRVI_CHECK(blank_id >= 0 && blank_id < C, OCRVI_EINVAL, "ctc_beam_lm: blank %d outside [0, %d)", blank_id, C);
    OCRVI_CHECK(nbest >= 1 && nbest <= beam, OCRVI_EINVAL, "ctc_beam_lm: nbest %d outside [1, beam = %d]", nbest, beam);
    OCRVI_CHECK(lmh && lmh->magic == LM_HANDLE_MAGIC, OCRVI_EINVAL, "ctc_beam_lm: null handle, or not a handle of ocrvi_lm_create");
    OCRVI_CHECK(lmh->device == device, OCRVI_EINVAL, "ctc_beam_lm: the model is on device %d, the call on %d", lmh->device, device);
    OCRVI_CHECK(lmh->hdr.num_classes == C, OCRVI_EINVAL, "ctc_beam_lm: the model has %d classes, the rows %d", lmh->hdr.num_classes, C);
    OCRVI_CHECK(lmh->hdr.bos_id == blank_id, OCRVI_EINVAL, "ctc_beam_lm: the model's BOS id %d is not the blank %d", lmh->hdr.bos_id, blank_id);
    OCRVI_CHECK(isfinite(alpha) && isfinite(beta) && alpha >= 0.0, OCRVI_EINVAL, "ctc_beam_lm: alpha %g, beta %g: need finite values, alpha >= 0",
                alpha, beta);
    OCRVI_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)score & 7) == 0 && ((uintptr_t)ctc_score & 7) == 0 && ((uintptr_t)lm_score & 7) == 0,
                OCRVI_EINVAL, "ctc_beam_lm: workspace must be 256-byte aligned and the scores 8-byte aligned");
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "ctc_beam_lm: workspace %zu < %zu bytes", workspace_bytes, need);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t prefix_bytes = (size_t)2 * beam * cl_stride(T) * sizeof(int16_t);
    const int in_lds = prefix_bytes <= CL_LDS_PREFIX_MAX;
    const ClLm m = {lmh->slots, lmh->hdr.log2cap, lmh->hdr.order, lmh->hdr.bos_id, lmh->hdr.unk_lp};
    OCRVI_TRY(ensure_max_smem((const void*)ctc_beam_lm_kernel, (int)CL_LDS_PREFIX_MAX));   // static + dynamic LDS passes 64 KiB
    ProfScope ps("ctc_beam_lm", 0.0, (double)T * B * C * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(ctc_beam_lm_kernel, dim3(B), dim3(CL_THREADS), in_lds ? prefix_bytes : 0, (hipStream_t)stream, log_probs, T, B, C, blank_id,
                       beam, nbest, m, alpha, beta, ids, lens, score, ctc_score, lm_score, (int16_t*)workspace,
                       (double*)((char*)workspace + cl_prefix_bytes(T, B, beam)), in_lds);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
