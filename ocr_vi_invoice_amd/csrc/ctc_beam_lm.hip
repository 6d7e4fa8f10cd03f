// CTC prefix beam search with a character n-gram model fused in (include/ocrvi.h, "Character n-gram language model" and "CTC prefix beam
// search with LM fusion"): the model's host entries and handle, and the search kernel.  DESIGN.md section 22 has the selection scheme, the
// workspace and the measurements.  The acoustic half is ctc_beam_core.h, shared with ctc_beam.hip: with alpha = beta = 0 the two give the
// same bytes.
#include "ctc_beam_core.h"
#include "lm_table.h"
#include "model.h"

// R = (s + alpha g) + beta len with every product and sum rounded on its own
#pragma clang fp contract(off)

using namespace ocrvi;
using namespace ocrvi::ctcbeam;

constexpr uint64_t LM_HANDLE_MAGIC = 0x6f6372766c6d6831ull;

struct ocrvi_lm {
    uint64_t magic = LM_HANDLE_MAGIC;
    int device = 0;
    lm::Header hdr{};
    DeviceStore store;
    const lm::Slot* slots = nullptr;   // device
};

namespace {

constexpr int CL_BATCH = 8;                       // LM terms in flight per class during the first scan of a step

struct ClTable : Table {   // the beam with each prefix's LM state
    double g[MAX_W];
    u64 ctx[MAX_W];                 // the LM context's symbols, oldest in the low ten bits
    int hlen[MAX_W], slot[MAX_W];   // hlen: symbols in ctx; slot: this prefix's row of LM terms in the workspace
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
__global__ __launch_bounds__(THREADS) void ctc_beam_lm_kernel(const float* __restrict__ log_probs, int T, int B, int C, int blank, int W,
                                                             int nbest, ClLm lmod, double alpha, double beta, int32_t* __restrict__ ids,
                                                             int32_t* __restrict__ lens, double* __restrict__ score,
                                                             double* __restrict__ ctc_score, double* __restrict__ lm_score,
                                                             int16_t* __restrict__ ws_prefix, double* ws_rows, int prefix_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
    __shared__ double v[2][MAX_C];
    __shared__ double uni[MAX_C];                     // the unigram level: lp of (c), unk_lp where there is none
    __shared__ ClTable tab[2];
    __shared__ double stay_pb[MAX_W], stay_pnb[MAX_W], stay_tot[MAX_W];
    __shared__ int merge_from[MAX_W];
    __shared__ unsigned excl[MAX_W][MAX_C / 32];
    __shared__ double red_tot[2][WAVES];
    __shared__ int red_idx[2][WAVES];
    __shared__ int sel_idx[MAX_W];
    __shared__ int ext_rank[MAX_W];                   // the ranks of the next table's new prefixes
    __shared__ double ext_acc[MAX_W][lm::MAX_ORDER];  // [e][k]: the backoff weights summed before level k is tried
    __shared__ u64 used_slots;
    __shared__ int n_ext_s;

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const Lds lds = {v, stay_pb, stay_pnb, stay_tot, merge_from, excl, red_tot, red_idx, sel_idx, b, tid, wave, lane};
    const int Ts = stride(T);
    int16_t* prefix = prefix_tables(cl_smem, ws_prefix, prefix_in_lds, b, W, Ts);
    const int jbits = log2_ceil(W);
    double* rows = ws_rows + (size_t)b * W * C;       // [W][C]: row `slot` holds lm(c | ctx) of the prefix that owns the slot

    // The rows of LM terms of the n_ext new prefixes ext_rank[0..n_ext) of table tn.  First each context's backoff weights, one probe per
    // (prefix, level); then one thread per (prefix, class) walks down from the longest gram to the bigram; the unigram level is in LDS.
    auto fill_rows = [&](const ClTable& tn, int n_ext) {
        for (int p = tid; p < n_ext * lm::MAX_ORDER; p += THREADS) {
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
        for (int p = tid; p < n_ext * C; p += THREADS) {
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

    float row[PER];
    load_row(lds, log_probs, B, C, 0, row);
    store_row(lds, 0, C, row);
    for (int c = tid; c < C; c += THREADS) {
        float lp, bo;
        uni[c] = (c != blank && cl_find(lmod, ((u64)1 << 60) | (u64)c, &lp, &bo)) ? (double)lp : lmod.unk_lp;
    }
    if (tid == 0) {
        ClTable& t0 = tab[0];
        t0.pb[0] = 0.0; t0.pnb[0] = -INFINITY; t0.s[0] = 0.0; t0.g[0] = 0.0;
        t0.hash[0] = HASH_EMPTY; t0.last[0] = -1; t0.len[0] = 0; t0.slot[0] = 0;
        t0.hlen[0] = lmod.order > 1 ? 1 : 0;
        t0.ctx[0] = lmod.order > 1 ? (u64)lmod.bos : 0;
        ext_rank[0] = 0;
    }
    clear_excl(lds);
    int n = 1, cur = 0;
    __syncthreads();
    fill_rows(tab[0], 1);
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const ClTable& tb = tab[cur];
        ClTable& nx = tab[cur ^ 1];
        const double* vt = lds.v[t & 1];
        const int16_t* pcur = prefix + (size_t)cur * W * Ts;
        int16_t* pnext = prefix + (size_t)(cur ^ 1) * W * Ts;
        if (t + 1 < T) load_row(lds, log_probs, B, C, t + 1, row);

        merge_search(lds, tb, pcur, n, jbits, Ts);
        __syncthreads();
        stay_candidates(lds, tb, vt, n, blank);
        __syncthreads();

        // ---- selection
        // The acoustic total of the extension (i, c), c != blank; -inf where it merged into another entry's stay candidate.
        auto ext_acoustic = [&](int i, int c) -> double {
            if (excluded(lds, i, c)) return -INFINITY;
            return (c == tb.last[i] ? tb.pb[i] : tb.s[i]) + vt[c];
        };
        auto rank_total = [&](double a, double g, int len) -> double { return (a + alpha * g) + beta * (double)len; };
        auto cand = [&](int i, int c, double term) -> Cand {
            double a, g;
            int len;
            if (c == blank) { a = lds.stay_tot[i]; g = tb.g[i]; len = tb.len[i]; }
            else { a = ext_acoustic(i, c); g = tb.g[i] + term; len = tb.len[i] + 1; }
            if (!(a > -INFINITY)) return Cand{-INFINITY, -1};
            return Cand{rank_total(a, g, len), i * C + c};
        };
        Cand top[PER];   // per class of its own, the best candidate not yet selected
        u64 taken[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = tid + k * THREADS;
            top[k] = Cand{-INFINITY, -1};
            taken[k] = 0;
            if (c >= C || (c != blank && !(vt[c] > -INFINITY))) continue;
            for (int i0 = 0; i0 < n; i0 += CL_BATCH) {
                double term[CL_BATCH];
#pragma unroll
                for (int u = 0; u < CL_BATCH; ++u) term[u] = c == blank ? 0.0 : rows[(size_t)tb.slot[min(i0 + u, n - 1)] * C + c];
#pragma unroll
                for (int u = 0; u < CL_BATCH; ++u)
                    if (i0 + u < n) top[k] = best(top[k], cand(i0 + u, c, term[u]));
            }
        }
        int m = 0;
        for (int r = 0; r < W; ++r) {
            Cand mine = top[0];
#pragma unroll
            for (int k = 1; k < PER; ++k) mine = best(mine, top[k]);
            const Cand w = block_best(lds, mine, r);
            if (w.idx < 0) break;                         // fewer than W candidates of non-zero probability (uniform)
            if (tid == 0) lds.sel_idx[r] = w.idx;
            m = r + 1;
            // the winner's class again, without what has been selected of it: the owner's wave, lane i the entry i (wave-uniform branch)
            const int wi = w.idx / C, wc = w.idx - wi * C, owner = wc & (THREADS - 1), wk = wc / THREADS;
            if (wave == (owner >> 6)) {
                u64 tk = 0;
#pragma unroll
                for (int k = 0; k < PER; ++k)
                    if (k == wk) tk = taken[k];
                tk = (u64)__shfl((unsigned)tk, owner & 63, 64) | ((u64)__shfl((unsigned)(tk >> 32), owner & 63, 64) << 32);
                tk |= (u64)1 << wi;
                Cand again = {-INFINITY, -1};
                if (lane < n && !((tk >> lane) & 1)) again = cand(lane, wc, wc == blank ? 0.0 : rows[(size_t)tb.slot[lane] * C + wc]);
                again = wave_best(again);
                if (tid == owner) {
#pragma unroll
                    for (int k = 0; k < PER; ++k)
                        if (k == wk) { taken[k] = tk; top[k] = again; }
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
                i = lds.sel_idx[r] / C; c = lds.sel_idx[r] - i * C;
                is_ext = c != blank;
                if (!is_ext) atomicOr(&used_slots, (u64)1 << tb.slot[i]);
            }
            const u64 ext_mask = __builtin_amdgcn_ballot_w64(is_ext);
            __syncthreads();
            if (r < m) {
                if (!is_ext) {
                    nx.pb[r] = lds.stay_pb[i]; nx.pnb[r] = lds.stay_pnb[i]; nx.s[r] = lds.stay_tot[i]; nx.g[r] = tb.g[i];
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
                    nx.hash[r] = hash_ext(tb.hash[i], c); nx.last[r] = c; nx.len[r] = tb.len[i] + 1; nx.slot[r] = slot;
                    if (lmod.order == 1) { nx.ctx[r] = 0; nx.hlen[r] = 0; }
                    else if (H < lmod.order - 1) { nx.ctx[r] = tb.ctx[i] | ((u64)c << (10 * H)); nx.hlen[r] = H + 1; }
                    else { nx.ctx[r] = (tb.ctx[i] >> 10) | ((u64)c << (10 * (H - 1))); nx.hlen[r] = H; }
                    ext_rank[e] = r;
                }
            }
            if (tid == 0) n_ext_s = __popcll(ext_mask);
        }
        __syncthreads();
        clear_merge_bits(lds, tb, n);
        copy_prefixes(lds, tb, pcur, pnext, m, C, blank, Ts);
        if (t + 1 < T) store_row(lds, (t + 1) & 1, C, row);
        fill_rows(nx, n_ext_s);                           // (every selected candidate has been read: the rows of dropped prefixes are free)
        n = m;
        cur ^= 1;
        __syncthreads();
    }

    // ---- output: the first nbest entries; a missing hypothesis is (-1, -inf, -inf, -inf, -1 ...)
    const ClTable& tb = tab[cur];
    const int16_t* pcur = prefix + (size_t)cur * W * Ts;
    for (int r = wave; r < nbest; r += WAVES) {
        const int li = write_ids_len(lds, tb, pcur, r, n, nbest, T, Ts, ids, lens);
        if (lane == 0) {
            const size_t o = (size_t)b * nbest + r;
            score[o] = r < n ? (tb.s[r] + alpha * tb.g[r]) + beta * (double)li : -INFINITY;
            ctc_score[o] = r < n ? tb.s[r] : -INFINITY;
            lm_score[o] = r < n ? tb.g[r] : -INFINITY;
        }
    }
}

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
    OCRVI_TRY(check_shape("ctc_beam_lm_workspace_bytes", T, B, C, beam));
    *bytes = prefix_bytes(T, B, beam) + align_up((size_t)B * beam * C * sizeof(double), 256);
    return OCRVI_OK;
}

extern "C" int ocrvi_ctc_beam_lm(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest, const ocrvi_lm* lmh,
                                 double alpha, double beta, int32_t* ids, int32_t* lens, double* score, double* ctc_score, double* lm_score,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    size_t need = 0;
    OCRVI_TRY(check_args("ctc_beam_lm", log_probs && ids && lens && score && ctc_score && lm_score && workspace,
                         ocrvi_ctc_beam_lm_workspace_bytes, T, B, C, blank_id, beam, nbest, &need));
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
    const size_t lds_bytes = prefix_lds_bytes(T, beam);
    const ClLm m = {lmh->slots, lmh->hdr.log2cap, lmh->hdr.order, lmh->hdr.bos_id, lmh->hdr.unk_lp};
    OCRVI_TRY(ensure_max_smem((const void*)ctc_beam_lm_kernel, (int)LDS_PREFIX_MAX));   // static + dynamic LDS passes 64 KiB
    ProfScope ps("ctc_beam_lm", 0.0, (double)T * B * C * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(ctc_beam_lm_kernel, dim3(B), dim3(THREADS), lds_bytes, (hipStream_t)stream, log_probs, T, B, C, blank_id, beam, nbest, m,
                       alpha, beta, ids, lens, score, ctc_score, lm_score, (int16_t*)workspace,
                       (double*)((char*)workspace + prefix_bytes(T, B, beam)), lds_bytes != 0);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
