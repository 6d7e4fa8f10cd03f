// CTC prefix beam search on the device (include/ocrvi.h, "CTC prefix beam search"): one launch carries a beam of prefixes through all T
// steps of every row, in float64.  DESIGN.md section 21 has the pass structure and the measurements.
#include "ctc_beam_core.h"

using namespace ocrvi;
using namespace ocrvi::ctcbeam;

namespace {

// One workgroup per row.  Thread tid owns the classes tid, tid + 256, ... of every entry: the candidate (i, c) is one LDS read and one add
// away from the table (only the W stay candidates take a logarithm), so nothing is stored per candidate: a thread keeps a cursor per
// class and recomputes the head of a list after it has been selected.
__global__ __launch_bounds__(THREADS) void ctc_beam_kernel(const float* __restrict__ log_probs, int T, int B, int C, int blank, int W,
                                                          int nbest, int32_t* __restrict__ ids, int32_t* __restrict__ lens,
                                                          double* __restrict__ score, int16_t* __restrict__ ws_prefix, int prefix_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cb_smem[];
    __shared__ double v[2][MAX_C];
    __shared__ Table tab[2];
    __shared__ double stay_pb[MAX_W], stay_pnb[MAX_W], stay_tot[MAX_W];
    __shared__ int merge_from[MAX_W];
    __shared__ unsigned excl[MAX_W][MAX_C / 32];
    __shared__ double red_tot[2][WAVES];
    __shared__ int red_idx[2][WAVES];
    __shared__ double sel_tot[MAX_W];
    __shared__ int sel_idx[MAX_W];

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const Lds lds = {v, stay_pb, stay_pnb, stay_tot, merge_from, excl, red_tot, red_idx, sel_idx, b, tid, wave, lane};
    const int Ts = stride(T);
    int16_t* prefix = prefix_tables(cb_smem, ws_prefix, prefix_in_lds, b, W, Ts);
    const int jbits = log2_ceil(W);

    float row[PER];
    load_row(lds, log_probs, B, C, 0, row);
    store_row(lds, 0, C, row);
    if (tid == 0) {
        tab[0].pb[0] = 0.0; tab[0].pnb[0] = -INFINITY; tab[0].s[0] = 0.0;
        tab[0].hash[0] = HASH_EMPTY; tab[0].last[0] = -1; tab[0].len[0] = 0;
    }
    clear_excl(lds);
    int n = 1, cur = 0;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const Table& tb = tab[cur];
        Table& nx = tab[cur ^ 1];
        const double* vt = lds.v[t & 1];
        const int16_t* pcur = prefix + (size_t)cur * W * Ts;
        int16_t* pnext = prefix + (size_t)(cur ^ 1) * W * Ts;
        if (t + 1 < T) load_row(lds, log_probs, B, C, t + 1, row);   // in flight during the step, stored to LDS at its end

        merge_search(lds, tb, pcur, n, jbits, Ts);
        __syncthreads();
        stay_candidates(lds, tb, vt, n, blank);
        __syncthreads();

        // ---- selection: W rounds of a workgroup arg-max; after a round only the winner's owner looks at its candidates again
        // The candidates a thread owns.  One irregular candidate at most: thread j < n the stay candidate of entry j, thread 64 + j the
        // repeat extension (j, last(l_j)), taken from pb_j.  And per class c of its own a list: the extensions (i, c) taken from s_i, in
        // rank order, which is their order in the selection (s_i does not increase with i, the add is monotonic, equal totals go by the
        // smaller i).  So a list is a cursor: its head is its best, and a selected head moves it on by one.
        Cand irr = {-INFINITY, -1};
        if (tid < n) {
            if (lds.stay_tot[tid] > -INFINITY) irr = {lds.stay_tot[tid], tid * C + blank};
        } else if (tid >= MAX_W && tid - MAX_W < n) {
            const int j = tid - MAX_W, c = tb.last[j];
            if (c >= 0 && !excluded(lds, j, c)) {
                const double tot = tb.pb[j] + vt[c];
                if (tot > -INFINITY) irr = {tot, j * C + c};
            }
        }
        int cursor[PER];
        auto skip = [&](int i, int c) -> int {   // the first entry from i on whose extension by c is a candidate of the list
            while (i < n && (tb.last[i] == c || excluded(lds, i, c))) ++i;
            return i;
        };
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = tid + k * THREADS;
            cursor[k] = (c < C && c != blank && vt[c] > -INFINITY) ? skip(0, c) : n;
        }
        auto head = [&]() -> Cand {            // the best of what this thread still owns
            Cand h = irr;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int c = tid + k * THREADS;
                if (cursor[k] < n) h = best(h, Cand{tb.s[cursor[k]] + vt[c], cursor[k] * C + c});
            }
            return h;
        };
        auto take = [&](int idx) {               // idx was this thread's head and has been selected
            if (irr.idx == idx) { irr.idx = -1; return; }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int c = tid + k * THREADS;
                if (cursor[k] < n && cursor[k] * C + c == idx) cursor[k] = skip(cursor[k] + 1, c);
            }
        };
        Cand mine = head();
        int m = 0;
        for (int r = 0; r < W; ++r) {
            const Cand w = block_best(lds, mine, r);
            if (w.idx < 0) break;                         // fewer than W candidates of non-zero probability (uniform)
            if (tid == 0) { sel_tot[r] = w.tot; lds.sel_idx[r] = w.idx; }
            m = r + 1;
            if (mine.idx == w.idx) { take(w.idx); mine = head(); }
        }
        __syncthreads();

        // ---- the next table, in rank order
        if (tid < m) {
            const int r = tid, i = lds.sel_idx[r] / C, c = lds.sel_idx[r] - i * C;
            if (c == blank) {
                nx.pb[r] = lds.stay_pb[i]; nx.pnb[r] = lds.stay_pnb[i]; nx.s[r] = lds.stay_tot[i];
                nx.hash[r] = tb.hash[i]; nx.last[r] = tb.last[i]; nx.len[r] = tb.len[i];
            } else {
                nx.pb[r] = -INFINITY; nx.pnb[r] = sel_tot[r]; nx.s[r] = sel_tot[r];
                nx.hash[r] = hash_ext(tb.hash[i], c); nx.last[r] = c; nx.len[r] = tb.len[i] + 1;
            }
        }
        clear_merge_bits(lds, tb, n);
        copy_prefixes(lds, tb, pcur, pnext, m, C, blank, Ts);
        if (t + 1 < T) store_row(lds, (t + 1) & 1, C, row);
        n = m;
        cur ^= 1;
        __syncthreads();
    }

    // ---- output: the first nbest entries; a missing hypothesis is (-1, -inf, -1 ...)
    const Table& tb = tab[cur];
    const int16_t* pcur = prefix + (size_t)cur * W * Ts;
    for (int r = wave; r < nbest; r += WAVES) {
        write_ids_len(lds, tb, pcur, r, n, nbest, T, Ts, ids, lens);
        if (lane == 0) score[(size_t)b * nbest + r] = r < n ? tb.s[r] : -INFINITY;
    }
}

}  // namespace

extern "C" int ocrvi_ctc_beam_workspace_bytes(int T, int B, int C, int beam, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "ctc_beam_workspace_bytes: null out");
    OCRVI_TRY(check_shape("ctc_beam_workspace_bytes", T, B, C, beam));
    *bytes = prefix_bytes(T, B, beam);
    return OCRVI_OK;
}

extern "C" int ocrvi_ctc_beam(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest, int32_t* ids,
                              int32_t* lens, double* score, void* workspace, size_t workspace_bytes, void* stream) {
    size_t need = 0;
    OCRVI_TRY(check_args("ctc_beam", log_probs && ids && lens && score && workspace, ocrvi_ctc_beam_workspace_bytes, T, B, C, blank_id, beam,
                         nbest, &need));
    OCRVI_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)score & 7) == 0, OCRVI_EINVAL,
                "ctc_beam: workspace must be 256-byte aligned and score 8-byte aligned");
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "ctc_beam: workspace %zu < %zu bytes", workspace_bytes, need);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t lds_bytes = prefix_lds_bytes(T, beam);
    ProfScope ps("ctc_beam", 0.0, (double)T * B * C * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(THREADS), lds_bytes, (hipStream_t)stream, log_probs, T, B, C, blank_id, beam, nbest, ids,
                       lens, score, (int16_t*)workspace, lds_bytes != 0);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
