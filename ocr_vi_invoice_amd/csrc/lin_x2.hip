// Token-stationary Linear for the f16x2 mode, K = 256 / 384:   out[M][N] = f16x2(A[M][K] . W^T + b)   (no activation, no residual)
//
// The recogniser's qkv-type projections (mixer.qkv, frm.h_qkv, frm.v_kv) on GEMM1 of mlp_x2.hip instead of the ring GEMM (gemm_ring.h), which
// streams BOTH operands through LDS and pays one exposed LDS latency and one barrier per K-step.  Here K is short enough for a wave's tokens to
// stay in registers for a whole row tile:
//   * one persistent workgroup per CU, 8 waves (two per SIMD); a tile is 128 tokens, 16 per wave;
//   * prologue per tile: the wave's 16 token rows (f16x2, chunk form) -> MFMA B-operand fragments in registers, (hi, lo) quartets:
//     K / 4 VGPRs per lane; lane (lr, g) owns channels 32 ks + 8 g .. + 8 of token lr for every K-step ks (mlp_x2's ownership);
//   * the only streamed operand is the weights, identical for every tile: units of 32 output columns x K (pack_lin_x2_stream: LDS image
//     order, quartet form, XOR-swizzled) copied linearly by the LDS-DMA through a ring of 3 (K = 384) / 4 (K = 256) units that runs ahead
//     across unit and tile boundaries; counted vmcnt, one barrier per unit;
//   * per unit: two 16-column accumulators that start at bias / wscale, K-steps in ascending order, three MFMAs per fragment pair, weight
//     fragments read two K-steps ahead; then  * wscale -> range check -> pack -> two 16-byte stores per lane;
//   * the MFMA layout puts four DIFFERENT tokens into four consecutive lanes, and the memory pipe works quad by quad: a 16-byte access per
//     lane then touches four cache lines per quad (mlp_x2.hip's epilogue has the measurement).  So the token rows are LOADED by lane
//     4 lr + g and moved to lane 16 g + lr with one ds_bpermute per dword, and the packed output chunks are moved back to lane 4 lr + g before
//     the stores: a quad reads 128 and writes 64 contiguous bytes of one token per instruction.
// Arithmetic: the K-slot assignment, the K-step order, the product order inside Mma::three, the accumulator start and the epilogue
// expression are the ring's (gemm_ring.h, BIAS_FIRST), so every output element has the ring's bits.
#include <stdlib.h>
#include <string.h>

#include "gemm_ring.h"
#include "kernels.h"
#include "weight_pack.h"

namespace ocrvi {
OCRVI_RANGE_FLAG_TU()

struct LinX2Params {
    const char* a = nullptr;        // [M][K] f16x2
    const char* wstream = nullptr;  // pack_lin_x2_stream: N / 32 units of 128 K bytes, then {wscale}
    const float* bias = nullptr;    // [N] or null
    void* out = nullptr;            // [M][N] f16x2
    unsigned out_bytes = 0;         // M * N * 4: range of the output buffer descriptor
    int M = 0, N = 0;
};

constexpr int LIN_X2_MAX_N = 2048;   // the bias lives in LDS behind the ring

template <int K, int R>
__global__ __launch_bounds__(512, 2) void lin_x2_kernel(const LinX2Params p) {
    typedef f16x2_t T;
    typedef Mma<T>::u4v U;
    constexpr int NWV = 8, NT = 64 * NWV;
    constexpr int KS = K / 32;            // 128-byte K-steps
    constexpr int UNIT = 32 * K * 4;      // bytes of a unit: [KS][32 weight rows][128 B]
    constexpr int IPW = UNIT / 1024 / NWV;   // DMA instructions per wave per unit
    constexpr int PF = R - 1;             // units in flight
    constexpr int NST = 2;                // stores per wave and unit (unconditional: the counted waits rely on it)
    static_assert(UNIT % (1024 * NWV) == 0 && R >= 2 && (PF - 1) * IPW + NST < 64, "ring geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    float* const c_b = (float*)(smem + R * UNIT);   // [N] bias / wscale

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, g = lane >> 4;
    const int q_tok = lane >> 2, q_g = lane & 3;          // the quad-per-token layout of the global accesses: lane 4 t + q <-> MFMA lane 16 q + t
    const int to_mfma = 4 * (4 * lr + g);                 // ds_bpermute byte address: lane (lr, g) takes what lane 4 lr + g loaded
    const int to_quad = 4 * (16 * q_g + q_tok);           // ... and lane 4 t + q takes what lane 16 q + t computed
    const int NU = p.N >> 5;              // units per token tile
    const float ws = *(const float*)(p.wstream + (size_t)NU * UNIT);
    {   // the accumulators start at the bias in their own scale (the weights carry a power of two: the division is exact)
        const float bsc = 1.f / ws;
        for (int i = tid; i < p.N; i += NT) c_b[i] = p.bias ? p.bias[i] * bsc : 0.f;
    }
    __syncthreads();  // (also drains those loads: no VMEM op is in flight when the ring starts)

    const int ntiles = (p.M + 127) >> 7;
    const int G = gridDim.x;
    const int my_tiles = (ntiles - (int)blockIdx.x + G - 1) / G;

    // ---- weight ring (mlp_x2.hip): ring unit q of the stream is unit q % NU of the packed buffer, already in LDS image order; this wave copies
    // 1-KiB pieces wave, wave + 8, ... of it.  Branch-free: past the end of the workgroup's stream it keeps fetching units nobody reads (their
    // slots are free), drained before the kernel ends.
    const char* const wbase = uniform_ptr(p.wstream);
    int prod_slot = 0, prod_mod = 0, cons_slot = 0;
    auto issue_unit = [&]() {
        const char* src = wbase + (size_t)prod_mod * UNIT + wave * 1024;
        const unsigned dst = lds0 + prod_slot * UNIT + wave * 1024;
#pragma unroll
        for (int j = 0; j < IPW; ++j) glds16(src + j * (NWV * 1024), (unsigned)lane * 16u, __builtin_amdgcn_readfirstlane(dst + j * (NWV * 1024)));
        prod_slot = prod_slot + 1 == R ? 0 : prod_slot + 1;
        prod_mod = prod_mod + 1 == NU ? 0 : prod_mod + 1;
    };
    // wait for the oldest unit in flight, free the slot before it, keep the ring full.  Younger than that unit's DMAs are the DMAs of the
    // PF - 1 units behind it and the previous unit's NST stores (none at the first unit of a tile, where everything has landed already).
    auto next_unit = [&]() -> const char* {
        wait_vm_barrier<(PF - 1) * IPW + NST>();
        issue_unit();
        const char* s = smem + cons_slot * UNIT;
        cons_slot = cons_slot + 1 == R ? 0 : cons_slot + 1;
        return s;
    };
    for (int i = 0; i < PF; ++i) issue_unit();
    const int sw = swz128(lr);
    const int fo0 = ((2 * g) ^ sw) << 4, fo1 = ((2 * g + 1) ^ sw) << 4;   // hi / lo quartet of this lane's 8 k-slots in a [row][128 B] image
    unsigned long long range_mask = 0;
    // stores through a buffer descriptor: the hardware's range check drops the lanes of tokens past M, the instruction still issues
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)p.out_bytes, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    const unsigned ldo_b = (unsigned)p.N * 4u;

    for (int t = 0; t < my_tiles; ++t) {
        const int tile = (int)blockIdx.x + t * G;
        const int tok = tile * 128 + wave * 16 + q_tok;   // the token this lane loads and stores (quad layout)
        // ---- prologue: this wave's 16 token rows -> B-operand fragments (tokens past M read row M - 1 and store nothing)
        U xH[KS], xL[KS];
        {
            const char* xr = p.a + (size_t)min(tok, p.M - 1) * (K * 4) + 32 * q_g;
            uint4 c[KS][2];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                c[ks][0] = *(const uint4*)(xr + 128 * ks);
                c[ks][1] = *(const uint4*)(xr + 128 * ks + 16);
            }
            auto mv = [&](unsigned v) { return (unsigned)__builtin_amdgcn_ds_bpermute(to_mfma, (int)v); };
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 c0 = make_uint4(mv(c[ks][0].x), mv(c[ks][0].y), mv(c[ks][0].z), mv(c[ks][0].w));
                const uint4 c1 = make_uint4(mv(c[ks][1].x), mv(c[ks][1].y), mv(c[ks][1].z), mv(c[ks][1].w));
                Mma<T>::regroup(c0, c1, xH[ks], xL[ks]);
            }
        }
        // every VMEM op issued so far by this wave (ring DMAs, the previous tile's stores, the loads above) has completed: the counted
        // waits of the unit loop start from the DMAs issued from here on (any older unit has landed)
        wait_vm_only<0>();
        const unsigned row_b = tok < p.M ? (unsigned)tok * ldo_b + 16u * (unsigned)q_g : OOB;

        for (int u = 0; u < NU; ++u) {
            const char* const U1 = next_unit();
            f32x4 acc[2];
            {
                // (the lane's offset from an opaque copy of the thread index, so that it is not carried through the unit loop)
                int l = threadIdx.x;
                asm volatile("" : "+v"(l));
                const float* bp = c_b + 32 * u + 4 * ((l & 63) >> 4);
                const float4 b0 = *(const float4*)bp, b1 = *(const float4*)(bp + 16);
                acc[0] = (f32x4){b0.x, b0.y, b0.z, b0.w};
                acc[1] = (f32x4){b1.x, b1.y, b1.z, b1.w};
            }
            constexpr int P1 = 2;   // K-steps read ahead
            uint4 wr[P1 + 1][2][2];   // [set][block][hi, lo]
            auto rd1 = [&](int ks, int set) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const char* r = U1 + (ks * 32 + 16 * a + lr) * 128;
                    wr[set][a][0] = *(const uint4*)(r + fo0);
                    wr[set][a][1] = *(const uint4*)(r + fo1);
                }
            };
#pragma unroll
            for (int i = 0; i < P1; ++i) rd1(i, i);
            // (fenced as in mlp_x2.hip: left alone hipcc sinks every fragment read to just in front of its first MFMA and waits lgkmcnt(0) for it)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + P1 < KS) rd1(ks + P1, (ks + P1) % (P1 + 1));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    Mma<T>::three(Mma<T>::as_u4v(wr[ks % (P1 + 1)][a][0]), Mma<T>::as_u4v(wr[ks % (P1 + 1)][a][1]), xH[ks], xL[ks], acc[a]);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- epilogue: weight scale, range check, pack; the chunk of channels 16 a + 4 g .. + 4 of token lr goes to lane 4 lr + g, which
            // stores it (no per-store branch: a token past M has an out-of-range offset)
            const unsigned off = row_b != OOB ? row_b + 128u * (unsigned)u : OOB;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float v[4] = {unscale<T>(acc[a][0], ws), unscale<T>(acc[a][1], ws), unscale<T>(acc[a][2], ws), unscale<T>(acc[a][3], ws)};
                range_mask |= f16x2_out_of_range(v);
                const uint4 e = Chunk<T>::pack(v);
                auto mv = [&](unsigned x) { return (unsigned)__builtin_amdgcn_ds_bpermute(to_quad, (int)x); };
                __builtin_amdgcn_raw_buffer_store_b128((u32x4){mv(e.x), mv(e.y), mv(e.z), mv(e.w)}, orsrc, off != OOB ? off + 64u * a : OOB, 0, 0);
            }
        }
    }
    wait_vm_only<0>();  // the ring's run-ahead fetches
    f16x2_raise(range_mask);
}

// ---------------------------------------------------------------- host: packing + launch
bool lin_x2_eligible(int dtype, int K, int N) {
    return mlp_x2_eligible(dtype, K) && (K == 256 || K == 384) && N > 0 && N % 32 == 0 && N <= LIN_X2_MAX_N;
}

// N / 32 units in output-column order, each the LDS image [K / 32][32 weight rows][128 B] (the fc1-slice layout of pack_mlp_x2_stream): row
// r of unit u is output column 32 u + r, its K-step ks the 32 weights w[32 u + r][32 ks ..] in order.  Rows are stored under
// swz128(32 ks + r); scale, halves and row form: weight_pack.h.  Tail: the weight scale's inverse (fp32).
void pack_lin_x2_stream(const float* w, int N, int K, std::vector<char>& out) {
    const int KS = K / 32, NU = N / 32;
    const float scale = f16x2_weight_scale(w, (size_t)N * K);
    const size_t units = (size_t)NU * KS * 32 * 128;
    out.assign(units + 4, 0);
    char* dst = out.data();
    for (int u = 0; u < NU; ++u)
        for (int ks = 0; ks < KS; ++ks)
            for (int r = 0; r < 32; ++r, dst += 128) f16x2_put_row(w + (size_t)(32 * u + r) * K + 32 * ks, scale, swz128(32 * ks + r), dst);
    const float tail = 1.0f / scale;
    memcpy(out.data() + units, &tail, 4);
}

template <int K, int R>
static int launch_lin_x2(const LinX2Params& p, int max_workgroups, hipStream_t s) {
    const int smem = R * 128 * K + LIN_X2_MAX_N * 4;
    auto kern = lin_x2_kernel<K, R>;
    OCRVI_TRY(ensure_max_smem((const void*)kern, smem));
    int n_cu = 0;
    OCRVI_TRY(device_cus(&n_cu));
    const int ntiles = (p.M + 127) / 128;
    const int grid = persistent_grid(ntiles, max_workgroups > 0 ? std::min(n_cu, max_workgroups) : n_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, s, p);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

int k_lin_x2(const void* a, const void* wstream, const float* bias, void* out, int M, int K, int N, hipStream_t s, int max_workgroups) {
    OCRVI_CHECK((K == 256 || K == 384) && N > 0 && N % 32 == 0 && N <= LIN_X2_MAX_N && a && wstream && out && M > 0 &&
                    (size_t)M * N * 4 < ((size_t)1 << 32) - 16,
                OCRVI_EINVAL, "lin_x2: bad argument (M %d, K %d, N %d)", M, K, N);
    LinX2Params p;
    p.a = (const char*)a; p.wstream = (const char*)wstream; p.bias = bias; p.out = out; p.M = M; p.N = N;
    p.out_bytes = (unsigned)((size_t)M * N * 4);
    char tag[64];
    snprintf(tag, sizeof(tag), "lin_x2_k%d_f16x2", K);
    ProfScope ps(tag, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N), s);
    if (K == 256) return launch_lin_x2<256, 4>(p, max_workgroups, s);
    return launch_lin_x2<384, 3>(p, max_workgroups, s);
}

}  // namespace ocrvi
