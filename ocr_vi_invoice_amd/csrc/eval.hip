// Validation on the device (include/ocrvi.h, "Validation"): the DB loss sums and pixel counts, the CTC negative log-likelihood and the
// Levenshtein distance.  Every entry is enqueue-only on the caller's stream; DESIGN.md section 9 has the pass structure.
#include <algorithm>

#include "common.h"

using namespace ocrvi;

namespace {

// ================================================================ ocrvi_det_eval
constexpr int EV_THREADS = 256;
constexpr int EV_MAX_BLOCKS = 1024;
constexpr int EV_BINS = 2048;
constexpr int EV_LEVELS = 3;       // 9 + 11 + 11 bits of the loss below its sign (always 0), most significant first
constexpr int EV_L0_BINS = 512;    // level 0: the exponent and one bit of the mantissa, where real losses crowd into a few dozen bins,
constexpr int EV_L0_COPIES = 8;    // so the fused pass keeps 8 copies of each bin side by side, one per lane & 7
constexpr int EV_NSUM = 8;         // doubles per block in the partials table: 6 of the fused pass, the top-k partial, one spare
typedef unsigned long long u64;

struct EvCtrl {
    u64 counts[5];   // tp, fp, fn, positives, negatives (integer atomics of the fused pass)
    u64 k;           // negative_count, set by the first scan
    u64 k_rem;       // how many of the k sit at or below the current prefix
    unsigned prefix; // the bits of the k-th value found so far; all 32 after the last scan
    unsigned done;   // the k-th value is final (k = 0, or fewer than k non-zero losses: the k-th is 0)
};
constexpr size_t EV_OFF_CTRL = (size_t)EV_LEVELS * EV_BINS * sizeof(u64);
constexpr size_t EV_OFF_PART = EV_OFF_CTRL + 256;
constexpr size_t EV_OFF_STREAM = EV_OFF_PART + (size_t)EV_MAX_BLOCKS * EV_NSUM * sizeof(double);
static_assert(sizeof(EvCtrl) <= 256 && EV_OFF_STREAM % 256 == 0, "workspace layout");

__device__ __forceinline__ int ev_shift(int level) { return level == 0 ? 22 : (level == 1 ? 11 : 0); }
__device__ __forceinline__ int ev_bits(int level) { return level == 0 ? 9 : 11; }
static_assert(EV_L0_BINS == 1 << 9, "level 0 has 9 bits");

static inline int ev_blocks(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + EV_THREADS * 16 - 1) / (EV_THREADS * 16), 1), EV_MAX_BLOCKS); }

struct EvAcc {
    double s[6] = {0, 0, 0, 0, 0, 0};   // positive BCE, dice intersection, sum pred mask, sum gt mask, L1 numerator, sum thresh_mask
    u64 c[5] = {0, 0, 0, 0, 0};
};

// One pixel of the fused pass: every fp32 term as the reference forms it, widened to float64 for the sum.  Returns the bits of the
// negative's loss (0 for a pixel that is no negative).
__device__ __forceinline__ unsigned ev_pixel(EvAcc& a, float bin, float th, float tb, float x, float g, float m, float tm, float tk) {
    const float gm = g * m, ngm = (1.f - g) * m;
    const int pv = ((int)gm) & 255, nv = ((int)ngm) & 255;   // .byte(): truncation, then the low 8 bits
    const float loss = fmaxf(x, 0.f) - x * g + log1pf(expf(-fabsf(x)));
    a.s[0] += (double)(loss * (float)pv);
    a.s[1] += (double)((tb * g) * m);
    a.s[2] += (double)(tb * m);
    a.s[3] += (double)gm;
    a.s[4] += (double)(fabsf(th - tm) * tk);
    a.s[5] += (double)tk;
    const float P = (bin > 0.5f ? 1.f : 0.f) * m;
    a.c[0] += (P == 1.f && gm == 1.f);
    a.c[1] += (P == 1.f && gm == 0.f);
    a.c[2] += (P == 0.f && gm == 1.f);
    a.c[3] += (u64)pv;
    a.c[4] += (u64)nv;
    return nv ? __float_as_uint(loss * (float)nv) : 0u;
}

__device__ __forceinline__ void ev_hist_add(unsigned* lds_hist, unsigned bits, int level, unsigned prefix) {
    if (bits == 0u) return;   // zeros are never counted: when the bins hold fewer than k values the k-th value is 0
    const int sh = ev_shift(level), nb = ev_bits(level);
    if ((bits >> (sh + nb)) != prefix) return;
    atomicAdd(&lds_hist[(bits >> sh) & ((1u << nb) - 1u)], 1u);
}

// Level 0 in the fused pass: copy lane & 7 of the bin, the copies of one bin in neighbouring banks.
__device__ __forceinline__ void ev_hist0_add(unsigned* lds_hist, unsigned bits) {
    if (bits == 0u) return;
    const unsigned bin = (bits >> ev_shift(0)) & (EV_L0_BINS - 1);   // the mask keeps a negative loss (gt outside [0, 1]) inside the table
    atomicAdd(&lds_hist[bin * EV_L0_COPIES + (threadIdx.x & (EV_L0_COPIES - 1))], 1u);
}

__device__ __forceinline__ void ev_hist0_flush(const unsigned* lds_hist, u64* hist) {
    for (int i = threadIdx.x; i < EV_L0_BINS; i += EV_THREADS) {
        unsigned v = 0;
#pragma unroll
        for (int c = 0; c < EV_L0_COPIES; ++c) v += lds_hist[i * EV_L0_COPIES + c];
        if (v) atomicAdd(&hist[i], (u64)v);
    }
}

__device__ __forceinline__ void ev_hist_flush(const unsigned* lds_hist, u64* hist) {
    for (int i = threadIdx.x; i < EV_BINS; i += EV_THREADS)
        if (lds_hist[i]) atomicAdd(&hist[i], (u64)lds_hist[i]);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Fused pass: each of the eight maps is read once; writes the loss stream, the level-0 histogram, the integer counts (atomics) and one
// row of float64 partials per block.  VEC: all nine pointers are 16-byte aligned and the body runs on groups of four pixels.
template <bool VEC>
__global__ __launch_bounds__(EV_THREADS) void det_eval_fused_kernel(const float* __restrict__ binary, const float* __restrict__ thresh,
                                                                    const float* __restrict__ thresh_binary, const float* __restrict__ logits,
                                                                    const float* __restrict__ gt, const float* __restrict__ mask,
                                                                    const float* __restrict__ thresh_map, const float* __restrict__ thresh_mask,
                                                                    size_t n, unsigned* __restrict__ stream, u64* __restrict__ hist,
                                                                    EvCtrl* __restrict__ ctrl, double* __restrict__ partials) {
    __shared__ unsigned lds_hist[EV_L0_BINS * EV_L0_COPIES];
    __shared__ double lds_sum[EV_THREADS / 64][6];
    for (int i = threadIdx.x; i < EV_L0_BINS * EV_L0_COPIES; i += EV_THREADS) lds_hist[i] = 0;
    __syncthreads();
    EvAcc a;
    const size_t tid = (size_t)blockIdx.x * EV_THREADS + threadIdx.x, nthr = (size_t)gridDim.x * EV_THREADS;
    size_t done = 0;
    if constexpr (VEC) {
        const size_t n4 = n / 4;
        for (size_t i = tid; i < n4; i += nthr) {
            const float4 b = ((const float4*)binary)[i], t = ((const float4*)thresh)[i], tb = ((const float4*)thresh_binary)[i];
            const float4 x = ((const float4*)logits)[i], g = ((const float4*)gt)[i], m = ((const float4*)mask)[i];
            const float4 tm = ((const float4*)thresh_map)[i], tk = ((const float4*)thresh_mask)[i];
            uint4 o;
            o.x = ev_pixel(a, b.x, t.x, tb.x, x.x, g.x, m.x, tm.x, tk.x);
            o.y = ev_pixel(a, b.y, t.y, tb.y, x.y, g.y, m.y, tm.y, tk.y);
            o.z = ev_pixel(a, b.z, t.z, tb.z, x.z, g.z, m.z, tm.z, tk.z);
            o.w = ev_pixel(a, b.w, t.w, tb.w, x.w, g.w, m.w, tm.w, tk.w);
            ((uint4*)stream)[i] = o;
            ev_hist0_add(lds_hist, o.x); ev_hist0_add(lds_hist, o.y);
            ev_hist0_add(lds_hist, o.z); ev_hist0_add(lds_hist, o.w);
        }
        done = n4 * 4;
    }
    for (size_t i = done + tid; i < n; i += nthr) {
        const unsigned o = ev_pixel(a, binary[i], thresh[i], thresh_binary[i], logits[i], gt[i], mask[i], thresh_map[i], thresh_mask[i]);
        stream[i] = o;
        ev_hist0_add(lds_hist, o);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double v = wave_sum(a.s[q]);
        if (lane == 0) lds_sum[wave][q] = v;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const u64 v = wave_sum(a.c[q]);
        if (lane == 0 && v) atomicAdd(&ctrl->counts[q], v);
    }
    __syncthreads();
    if (threadIdx.x < 6) {   // waves in index order
        double v = lds_sum[0][threadIdx.x];
        for (int w = 1; w < EV_THREADS / 64; ++w) v += lds_sum[w][threadIdx.x];
        partials[(size_t)blockIdx.x * EV_NSUM + threadIdx.x] = v;
    }
    ev_hist0_flush(lds_hist, hist);
}

// One block.  Level 0 first fixes k = min(negatives, trunc(positives * ratio)).  Walks the level's bins from the top until they hold the
// k_rem-th value, narrows the prefix to that bin and keeps what is left of k_rem inside it.  Thread t owns 8 bins, top down; a scan over
// the threads' sums tells the one thread whose bins hold the k_rem-th value, and it alone writes.
__global__ __launch_bounds__(EV_THREADS) void det_eval_scan_kernel(const u64* __restrict__ hist, EvCtrl* __restrict__ ctrl, int level,
                                                                   double negative_ratio) {
    constexpr int PER = EV_BINS / EV_THREADS;
    __shared__ u64 incl[EV_THREADS];
    // everything the block reads from ctrl is read here, before the first barrier; the writes come after the last
    if (level > 0 && ctrl->done) return;
    const unsigned old_prefix = ctrl->prefix;
    u64 k_rem;
    if (level == 0) {
        const u64 pos = ctrl->counts[3], neg = ctrl->counts[4];
        const double want = trunc((double)pos * negative_ratio);
        u64 k = neg;
        if (!(want >= 1.0)) k = 0;                                  // 0, negative or NaN
        else if (want < 9.0e18 && (u64)want < neg) k = (u64)want;
        k_rem = k;
        if (k == 0) {
            if (threadIdx.x == 0) {
                ctrl->k = 0; ctrl->k_rem = 0; ctrl->prefix = 0x7f800000u; ctrl->done = 1;   // nothing is above +inf: the top-k sum is 0
            }
            return;
        }
    } else {
        k_rem = ctrl->k_rem;
    }
    const int nbins = 1 << ev_bits(level);
    u64 mine[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {   // bins EV_BINS-1 - t*PER .. EV_BINS-1 - t*PER - (PER-1)
        const int b = EV_BINS - 1 - (threadIdx.x * PER + j);
        mine[j] = b < nbins ? hist[b] : 0;
        s += mine[j];
    }
    incl[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < EV_THREADS; o <<= 1) {
        const u64 v = (int)threadIdx.x >= o ? incl[threadIdx.x - o] : 0;
        __syncthreads();
        incl[threadIdx.x] += v;
        __syncthreads();
    }
    const u64 total = incl[EV_THREADS - 1];
    u64 above = incl[threadIdx.x] - s;   // what the threads before this one hold
    if (level == 0 && threadIdx.x == 0) ctrl->k = k_rem;
    if (total < k_rem) {   // fewer than k_rem non-zero values left: the k-th value is 0 and every non-zero loss is above it
        if (threadIdx.x == 0) {
            ctrl->k_rem = 0; ctrl->prefix = 0; ctrl->done = 1;
        }
        return;
    }
    if (!(above < k_rem && k_rem <= above + s)) return;
    int jb = PER - 1;
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (!found) {
            if (above + mine[j] >= k_rem) { found = true; jb = j; }
            else above += mine[j];
        }
    }
    const int b = EV_BINS - 1 - (threadIdx.x * PER + jb);
    ctrl->prefix = (level == 0 ? 0u : (old_prefix << ev_bits(level))) | (unsigned)b;
    ctrl->k_rem = k_rem - above;
}

__global__ __launch_bounds__(EV_THREADS) void det_eval_hist_kernel(const unsigned* __restrict__ stream, size_t n, int level,
                                                                   const EvCtrl* __restrict__ ctrl, u64* __restrict__ hist) {
    __shared__ unsigned lds_hist[EV_BINS];
    if (ctrl->done) return;
    const unsigned prefix = ctrl->prefix;
    for (int i = threadIdx.x; i < EV_BINS; i += EV_THREADS) lds_hist[i] = 0;
    __syncthreads();
    const size_t tid = (size_t)blockIdx.x * EV_THREADS + threadIdx.x, nthr = (size_t)gridDim.x * EV_THREADS;
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += nthr) {
        const uint4 o = ((const uint4*)stream)[i];
        ev_hist_add(lds_hist, o.x, level, prefix); ev_hist_add(lds_hist, o.y, level, prefix);
        ev_hist_add(lds_hist, o.z, level, prefix); ev_hist_add(lds_hist, o.w, level, prefix);
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nthr) ev_hist_add(lds_hist, stream[i], level, prefix);
    __syncthreads();
    ev_hist_flush(lds_hist, hist);
}

// Sum of the losses strictly above the k-th value, one float64 partial per block.
__global__ __launch_bounds__(EV_THREADS) void det_eval_above_kernel(const unsigned* __restrict__ stream, size_t n, const EvCtrl* __restrict__ ctrl,
                                                                    double* __restrict__ partials) {
    __shared__ double lds_sum[EV_THREADS / 64];
    const unsigned v = ctrl->prefix;
    double s = 0;
    const size_t tid = (size_t)blockIdx.x * EV_THREADS + threadIdx.x, nthr = (size_t)gridDim.x * EV_THREADS;
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += nthr) {
        const uint4 o = ((const uint4*)stream)[i];
        if (o.x > v) s += (double)__uint_as_float(o.x);
        if (o.y > v) s += (double)__uint_as_float(o.y);
        if (o.z > v) s += (double)__uint_as_float(o.z);
        if (o.w > v) s += (double)__uint_as_float(o.w);
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nthr) {
        const unsigned o = stream[i];
        if (o > v) s += (double)__uint_as_float(o);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) lds_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EV_THREADS / 64; ++w) s += lds_sum[w];
        partials[(size_t)blockIdx.x * EV_NSUM + 6] = s;
    }
}

// One block of 7 waves: wave q adds column q of the partials table, lane l the rows l, l + 64, ... in order, then the fixed shuffle tree.
__global__ __launch_bounds__(7 * 64) void det_eval_final_kernel(const double* __restrict__ partials, int blocks, const EvCtrl* __restrict__ ctrl,
                                                                void* __restrict__ record) {
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0;
    for (int b = lane; b < blocks; b += 64) s += partials[(size_t)b * EV_NSUM + q];
    s = wave_sum(s);
    if (lane != 0) return;
    long long* ri = (long long*)record;
    double* rd = (double*)record;
    if (q == 0) {
        for (int i = 0; i < 5; ++i) ri[i] = (long long)ctrl->counts[i];
        ri[OCRVI_DET_EVAL_K] = (long long)ctrl->k;
    }
    if (q == 6) {
        const u64 k_rem = ctrl->k_rem;
        rd[OCRVI_DET_EVAL_TOPK_BCE] = k_rem ? s + (double)k_rem * (double)__uint_as_float(ctrl->prefix) : s;
    } else {
        const int slot[6] = {OCRVI_DET_EVAL_POS_BCE, OCRVI_DET_EVAL_DICE_INTER, OCRVI_DET_EVAL_PRED_MASK, OCRVI_DET_EVAL_GT_MASK,
                             OCRVI_DET_EVAL_L1_NUM, OCRVI_DET_EVAL_THRESH_MASK};
        rd[slot[q]] = s;
    }
}

// ================================================================ ocrvi_ctc_loss
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// One wave per sequence; state s of the extended sequence lives in lane s & 63, the two alpha rows in LDS.
__global__ __launch_bounds__(64) void ctc_loss_kernel(const float* __restrict__ log_probs, int T, int B, int C, const int32_t* __restrict__ targets,
                                                      int Lmax, const int32_t* __restrict__ target_lengths,
                                                      const int32_t* __restrict__ input_lengths, int blank, double* __restrict__ nll) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];
    const int S_max = 2 * Lmax + 1;
    double* alpha = (double*)ctc_smem;                       // [2][S_max]
    int* label = (int*)(alpha + 2 * (size_t)S_max);          // [Lmax]
    const int b = blockIdx.x, lane = threadIdx.x;
    const int L = min(max(target_lengths[b], 0), Lmax);
    const int Tb = input_lengths ? min(max(input_lengths[b], 0), T) : T;
    const int S = 2 * L + 1;
    for (int i = lane; i < L; i += 64) label[i] = targets[(size_t)b * Lmax + i];
    __syncthreads();
    if (Tb == 0) {   // no step: only the empty labelling has a path
        if (lane == 0) nll[b] = L == 0 ? 0.0 : INFINITY;
        return;
    }
    // emission of state s at step t; a label outside [0, C) has probability 0 (no address is formed for it)
    auto emit = [&](int t, int s) -> double {
        const int c = (s & 1) ? label[s >> 1] : blank;
        return (c >= 0 && c < C) ? (double)log_probs[((size_t)t * B + b) * C + c] : -INFINITY;
    };
    for (int s = lane; s < S; s += 64) alpha[s] = s < 2 ? emit(0, s) : -INFINITY;
    __syncthreads();
    int cur = 0;
    for (int t = 1; t < Tb; ++t) {
        const double* prev = alpha + (size_t)cur * S_max;
        double* next = alpha + (size_t)(cur ^ 1) * S_max;
        for (int s = lane; s < S; s += 64) {
            const double a0 = prev[s];
            const double a1 = s >= 1 ? prev[s - 1] : -INFINITY;
            const bool skip = (s & 1) && s >= 3 && label[s >> 1] != label[(s >> 1) - 1];
            const double a2 = skip ? prev[s - 2] : -INFINITY;
            const double e = emit(t, s);
            const double l = lse3(a0, a1, a2);
            next[s] = (l == -INFINITY || e == -INFINITY) ? -INFINITY : l + e;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (lane == 0) {
        const double* last = alpha + (size_t)cur * S_max;
        const double l = lse3(last[S - 1], S >= 2 ? last[S - 2] : -INFINITY, -INFINITY);
        nll[b] = -l;
    }
}

// ================================================================ ocrvi_edit_distance
constexpr int ED_BIG = 1 << 29;

// One wave per pair.  Rows run over the prediction (ids < 2 dropped), columns over the ground truth; a row of the DP lies across the
// lanes, 64 columns at a time, and the insertion chain d[j] = min_k<=j (t[k] + j - k) is j + the prefix minimum of t[k] - k.
__global__ __launch_bounds__(64) void edit_distance_kernel(const int32_t* __restrict__ pred_ids, int T, const int32_t* __restrict__ pred_lens,
                                                           const int32_t* __restrict__ gt_ids, int G, const int32_t* __restrict__ gt_lens,
                                                           int32_t* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ed_smem[];
    int* pred = (int*)ed_smem;            // [T] compacted
    int* gt = pred + T;                   // [G]
    int* row = gt + G;                    // [2][G + 1]
    const int b = blockIdx.x, lane = threadIdx.x;
    const int plen = min(max(pred_lens[b], 0), T), n = min(max(gt_lens[b], 0), G);
    int m = 0;
    for (int base = 0; base < plen; base += 64) {
        const int i = base + lane;
        const int id = i < plen ? pred_ids[(size_t)b * T + i] : 0;
        const bool keep = id >= 2;
        const unsigned long long bal = __ballot(keep);
        if (keep) pred[m + __popcll(bal & ((1ull << lane) - 1ull))] = id;
        m += __popcll(bal);
    }
    for (int j = lane; j < n; j += 64) gt[j] = gt_ids[(size_t)b * G + j];
    for (int j = lane; j <= n; j += 64) row[j] = j;
    __syncthreads();
    int cur = 0;
    for (int i = 1; i <= m; ++i) {
        const int* prev = row + (size_t)cur * (G + 1);
        int* next = row + (size_t)(cur ^ 1) * (G + 1);
        const int p = pred[i - 1];
        int carry = ED_BIG;   // min of t[k] - k over the chunks already done
        for (int base = 0; base <= n; base += 64) {
            const int j = base + lane;
            int u = ED_BIG;
            if (j <= n) {
                const int t = j == 0 ? i : min(prev[j] + 1, prev[j - 1] + (gt[j - 1] != p));
                u = t - j;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(u, o, 64);
                if (lane >= o) u = min(u, v);
            }
            u = min(u, carry);
            if (j <= n) next[j] = u + j;
            carry = __shfl(u, 63, 64);
        }
        cur ^= 1;
        __syncthreads();
    }
    if (lane == 0) dist[b] = row[(size_t)cur * (G + 1) + n];
}

}  // namespace

extern "C" int ocrvi_det_eval_workspace_bytes(int N, int H, int W, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "det_eval_workspace_bytes: null out");
    OCRVI_CHECK(N >= 1 && H >= 1 && W >= 1, OCRVI_EINVAL, "det_eval_workspace_bytes: bad shape %d x %d x %d", N, H, W);
    *bytes = EV_OFF_STREAM + align_up((size_t)N * H * W * sizeof(unsigned), 256);
    return OCRVI_OK;
}

extern "C" int ocrvi_det_eval(int device, const float* binary, const float* thresh, const float* thresh_binary, const float* bin_logits,
                              const float* gt, const float* mask, const float* thresh_map, const float* thresh_mask, int N, int H, int W,
                              double negative_ratio, void* record, void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(binary && thresh && thresh_binary && bin_logits && gt && mask && thresh_map && thresh_mask && record && workspace, OCRVI_EINVAL,
                "det_eval: null argument");
    size_t need = 0;
    OCRVI_TRY(ocrvi_det_eval_workspace_bytes(N, H, W, &need));
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "det_eval: workspace %zu < %zu bytes", workspace_bytes, need);
    OCRVI_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)record & 7) == 0, OCRVI_EINVAL,
                "det_eval: workspace must be 256-byte aligned and the record 8-byte aligned");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)N * H * W;
    const int blocks = ev_blocks(n);   // a function of the shape alone: the float64 sums are reproducible on every device
    char* ws = (char*)workspace;
    u64* hist = (u64*)ws;
    EvCtrl* ctrl = (EvCtrl*)(ws + EV_OFF_CTRL);
    double* partials = (double*)(ws + EV_OFF_PART);
    unsigned* loss = (unsigned*)(ws + EV_OFF_STREAM);
    OCRVI_HIP(hipMemsetAsync(ws, 0, EV_OFF_PART, s));
    const uintptr_t al = (uintptr_t)binary | (uintptr_t)thresh | (uintptr_t)thresh_binary | (uintptr_t)bin_logits | (uintptr_t)gt |
                         (uintptr_t)mask | (uintptr_t)thresh_map | (uintptr_t)thresh_mask;
    ProfScope ps("det_eval", 0.0, (double)n * 32.0, s);
    if ((al & 15) == 0)
        hipLaunchKernelGGL(det_eval_fused_kernel<true>, dim3(blocks), dim3(EV_THREADS), 0, s, binary, thresh, thresh_binary, bin_logits, gt, mask,
                           thresh_map, thresh_mask, n, loss, hist, ctrl, partials);
    else
        hipLaunchKernelGGL(det_eval_fused_kernel<false>, dim3(blocks), dim3(EV_THREADS), 0, s, binary, thresh, thresh_binary, bin_logits, gt, mask,
                           thresh_map, thresh_mask, n, loss, hist, ctrl, partials);
    for (int level = 0; level < EV_LEVELS; ++level) {
        if (level > 0)
            hipLaunchKernelGGL(det_eval_hist_kernel, dim3(blocks), dim3(EV_THREADS), 0, s, loss, n, level, ctrl, hist + (size_t)level * EV_BINS);
        hipLaunchKernelGGL(det_eval_scan_kernel, dim3(1), dim3(EV_THREADS), 0, s, hist + (size_t)level * EV_BINS, ctrl, level, negative_ratio);
    }
    hipLaunchKernelGGL(det_eval_above_kernel, dim3(blocks), dim3(EV_THREADS), 0, s, loss, n, ctrl, partials);
    hipLaunchKernelGGL(det_eval_final_kernel, dim3(1), dim3(7 * 64), 0, s, partials, blocks, ctrl, record);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_ctc_loss(int device, const float* log_probs, int T, int B, int C, const int32_t* targets, int Lmax,
                              const int32_t* target_lengths, const int32_t* input_lengths, int blank, double* nll, void* stream) {
    OCRVI_CHECK(log_probs && target_lengths && nll && (targets || Lmax == 0), OCRVI_EINVAL, "ctc_loss: null argument");
    OCRVI_CHECK(T >= 1 && B >= 1 && C >= 1 && Lmax >= 0 && Lmax <= OCRVI_CTC_LOSS_MAX_TARGET, OCRVI_EINVAL,
                "ctc_loss: bad shape T %d B %d C %d Lmax %d (Lmax <= %d)", T, B, C, Lmax, OCRVI_CTC_LOSS_MAX_TARGET);
    OCRVI_CHECK(blank >= 0 && blank < C, OCRVI_EINVAL, "ctc_loss: blank %d outside [0, %d)", blank, C);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t smem = 2 * (size_t)(2 * Lmax + 1) * sizeof(double) + (size_t)Lmax * sizeof(int);
    ProfScope ps("ctc_loss", 0.0, (double)T * B * C * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(ctc_loss_kernel, dim3(B), dim3(64), smem, (hipStream_t)stream, log_probs, T, B, C, targets, Lmax, target_lengths,
                       input_lengths, blank, nll);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_edit_distance(int device, const int32_t* pred_ids, int T, const int32_t* pred_lens, const int32_t* gt_ids, int G,
                                   const int32_t* gt_lens, int B, int32_t* dist, void* stream) {
    OCRVI_CHECK(pred_lens && gt_lens && dist && (pred_ids || T == 0) && (gt_ids || G == 0), OCRVI_EINVAL, "edit_distance: null argument");
    OCRVI_CHECK(B >= 1 && T >= 0 && G >= 0 && T <= OCRVI_EDIT_DISTANCE_MAX_LEN && G <= OCRVI_EDIT_DISTANCE_MAX_LEN, OCRVI_EINVAL,
                "edit_distance: bad shape B %d T %d G %d (rows of at most %d ids)", B, T, G, OCRVI_EDIT_DISTANCE_MAX_LEN);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t smem = ((size_t)T + G + 2 * ((size_t)G + 1)) * sizeof(int);
    ProfScope ps("edit_distance", 0.0, (double)B * (T + G) * 4.0, (hipStream_t)stream);
    hipLaunchKernelGGL(edit_distance_kernel, dim3(B), dim3(64), smem, (hipStream_t)stream, pred_ids, T, pred_lens, gt_ids, G, gt_lens, dist);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
