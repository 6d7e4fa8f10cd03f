// ResNet-50 layer1 chain in ONE f16x2 kernel: conv2 3x3 64->64 + ReLU (t2), conv3 1x1 64->256 + identity + ReLU (y) and -- unless built
// y-only (PHC = false) -- the NEXT block's conv1 1x1 256->64 + ReLU (t1').  Everything behind the 3x3 is per pixel, and a wave of
// conv3_halo's NC = 64 tile ends phase A with all 64 channels of t2 for its 2 x 16 pixels in its accumulators: t2 never goes to memory and
// y is not read back for conv1.  Per chain the traffic falls from t1 + 2 t2 + identity + 2 y + t1' to t1 + identity + y + t1'.
//
// Phase A is conv3_halo_kernel<f16x2_t, 64, ACT_RELU>'s unit loop, copied unchanged (same MFMA order per accumulator: t2 has the bits the
// stand-alone kernel stores).  Then per tile and wave:
//   t2 = ReLU(acc * ws2 + bias2), rounded to f16x2 with Chunk::pack as the unfused path rounds it when it stores t2.
//   Its chunks are the pixel operand of conv3 STRAIGHT FROM THE ACCUMULATOR LANES (no LDS scratch: the ring keeps its 64 KiB): lane
//   (lr, g) holds channels 16 a + 4 g + e of pixel lr, so K-step j of conv3 takes (chunk a = 2 j, chunk a = 2 j + 1), i.e. lane group g
//   supplies k-slots {32 j + 4 g + e, 32 j + 16 + 4 g + e}; the host packs the weights' k-slots in the same order (pack_bneck_tail), as
//   mlp_x2 does for fc2.  The same holds between y's groups of 32 channels and conv1's K-steps.
//   Eight groups q of 32 conv3 channels:
//     B: 32 pixels x 32 channels, K = 64: 2 rows x 2 column blocks x 2 K-steps x three products = 24 MFMAs; * ws3 + bias3 + identity (fp32
//        sum of the f16x2 identity's halves) + ReLU, range check, pack, store y.
//     C: the packed y chunks of the group are K-step q of conv1 (32 pixels x 64 channels, 24 MFMAs).
//   Then t1' = ReLU(accC * ws1 + bias1'), range check, pack, store.
//
// Weight stream: per group one 8-KiB unit for B (K 64 x N 32, rows (j, n)) and one for C (K 32 x N 64), host-packed as (hi, lo) quartets in
// LDS image order (swz_halo baked in) and streamed through conv3_halo's ring of eight 8-KiB slots behind the tile's 18 conv2 units: a tile
// is TS = 18 + 16 (18 + 8 y-only) units, one 1-KiB piece per wave each, one counted wait + barrier per unit as in phase A.  A unit's
// fragments are rows 16 a + lr for every unit kind, so phase A's look-ahead also fetches the first tail unit's; in the tail (no registers
// for a second copy) a fragment is used for both rows and then re-requested from the next unit, under the MFMAs behind it.
//
// Identity: the 16 dwords per lane of group q + 1 are requested (inline-asm loads, invisible to hipcc's own waits) behind group q's y
// stores, a C step and a B step of MFMAs ahead of their use, into the registers group q's epilogue has just consumed.
//
// vmcnt accounting (extends conv3_halo.h's proof; VMEM ops of a wave retire in issue order).  Local step l = 0 .. TS - 1 of a tile.  The
// wait of step l must cover weight unit l + 1, issued in step l - 6 behind that step's patch; younger than it are
//   * the 5 units l + 2 .. l + 6;
//   * the patch pieces (>= PPW_MIN = 5) issued at steps l - 5 .. l - 1 (patches go out at l = 0 and l = 9);
//   * the other operations of steps l - 6 .. l - 1 (`body`): 4 identity loads behind step 17; 4 y stores + 4 identity loads in every
//     B step but the last, which has the stores alone (a load nobody binds would land in registers hipcc has handed to something else:
//     it did, in the next tile's first pixel fragment); 8 t1' stores behind the last C step.
//   Steps with l < 6 reach into the previous tile (none of it in a workgroup's first tile).  bt_wait sums these at compile time; every
//   store is unconditional (out-of-range lanes: dump page), so the counts are exact, and the largest (33; 53 y-only) fits the 6-bit counter.
//   The identity of group q is awaited in B's epilogue with only the weight units issued since (1 or 2) younger.
#pragma once
#include "conv3_halo.h"

namespace ocrvi {

template <bool PHC> struct BtCfg {
    using C = HaloCfg<64>;
    static constexpr int TU = PHC ? 16 : 8, TS = 18 + TU, GS = PHC ? 2 : 1;   // tail units, steps per tile, steps per group
    static constexpr int BIAS = 0, PB = 2048;   // LDS: fp32 bias2 [64], bias3 [256], bias1' [64] first (one base register + immediates), then the patches and the ring
    static constexpr int SMEM = PB + 2 * C::PATCH + C::NWS * C::WU;
    static constexpr int body(int l) {   // VMEM operations of step l other than its weight unit and patch
        if (l == 17) return 4;
        if (l < 18) return 0;
        const int k = l - 18;
        if (!PHC) return k == 7 ? 4 : 8;
        return (k & 1) == 0 ? (k == 14 ? 4 : 8) : (k == 15 ? 8 : 0);
    }
    static constexpr int patch(int l) { return (l == 0 || l == 9) ? C::PPW_MIN : 0; }
    static constexpr int wait(int l, bool wrap) {   // operations younger than unit l + 1 at the wait of step l
        int n = C::NWS - 3;
        for (int k = l - 6; k <= l - 1; ++k) {
            int kk = k;
            if (kk < 0) { if (!wrap) continue; kk += TS; }
            n += body(kk);
            if (k >= l - 5) n += patch(kk);
        }
        return n;
    }
    static constexpr int max_wait() {
        int m = 0;
        for (int l = 0; l < TS; ++l) m = wait(l, true) > m ? wait(l, true) : m;
        return m;
    }
    static_assert(C::NWS == 8 && C::WPW == 1 && C::RW == 2, "NC = 64 tile");
    static_assert(max_wait() < 64, "vmcnt is a 6-bit counter");
    static_assert(SMEM <= 160 * 1024, "LDS");
};

template <bool PHC>
__global__ __launch_bounds__(512, 2) void bneck_tail_kernel(const BneckTailParams p, int tiles_x, int tiles_y) {
    using T = f16x2_t;
    using B = BtCfg<PHC>;
    using C = HaloCfg<64>;
    constexpr int PW = C::PW, NI_P = C::NI_P, PSLOTS = C::PSLOTS, NWS = C::NWS, RW = C::RW, TS = B::TS;
    constexpr int ncb = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, g = lane >> 4;
    const int ntile = p.n_img * tiles_y * tiles_x;
    const int G = gridDim.x;
    const int first = xcd_remap(blockIdx.x, gridDim.x);
    const int my_tiles = first < ntile ? (ntile - first + G - 1) / G : 0;
    const char* const X = (const char*)p.x;
    const char* const zero = (const char*)p.zero_page + (lane & 7) * 16;
    constexpr int pix_b = 64 * 4, wrow_b = 576 * 4;

    {   // the three biases into LDS
        float* bl = (float*)(smem + B::BIAS);
        for (int n = tid; n < 384; n += 512) {
            float v = 0.f;
            if (n < 64) v = p.bias2 ? p.bias2[n] : 0.f;
            else if (n < 320 || PHC) v = p.bias_t ? p.bias_t[n - 64] : 0.f;
            bl[n] = v;
        }
        __syncthreads();
    }

    // ---- weight stream: unit u of the cyclic per-tile sequence = conv2's (cb, tap) units 0 .. 17 (rows (wave) * 8 + lane / 8 of the
    // [64][576] matrix), then the tail units (LDS images: this wave's piece is bytes wave * 1024 + lane * 16)
    unsigned wvoff2, wvofft = (unsigned)(wave * 1024 + lane * 16);
    {
        const int n = wave * 8 + (lane >> 3), cq = lane & 7;
        wvoff2 = (unsigned)(n * wrow_b + ((cq ^ swz_halo(n)) << 4));
    }
    int wi_u = 0, wi_s = 0;   // next unit to issue (index in the tile's sequence), and its step index (-> ring slot)
    auto issue_w = [&]() {
        const bool tail = wi_u >= 18;   // (wave-uniform)
        const int cb = wi_u >= 9 ? 1 : 0, tap = wi_u - 9 * cb;
        const char* base = uniform_ptr(tail ? (const char*)p.wt + (size_t)(wi_u - 18) * 8192 : (const char*)p.w2 + (size_t)(tap * 64 + cb * 32) * 4);
        const unsigned dst = lds0 + B::PB + 2 * C::PATCH + (wi_s & (NWS - 1)) * C::WU;
        glds16_sc1(base, tail ? wvofft : wvoff2, __builtin_amdgcn_readfirstlane(dst + wave * 1024));
        ++wi_s;
        if (++wi_u == TS) wi_u = 0;
    };

    // ---- patch stream (conv3_halo): stage k = (my tile k / 2, channel block k % 2)
    // (the per-lane sources are rebuilt for every stage, not kept from channel block 0 to 1: they would be live across the whole tail)
    int pi_tile = 0, pi_cb = 0, pi_k = 0;
    auto issue_patch = [&]() {
        const char* src[PSLOTS];
        const int t = pi_tile;
        const bool live = t < my_tiles;
        const int tile = first + t * G;
        const int tx = tile % tiles_x, r = tile / tiles_x, ty = r % tiles_y, img = r / tiles_y;
        const int y0 = ty * C::TH - 1, x0 = tx * C::TW - 1;
#pragma unroll
        for (int j = 0; j < PSLOTS; ++j) {
            const int pp = (wave + 8 * j) * 8 + (lane >> 3), cq = lane & 7;
            const int py = pp / PW, px = pp - py * PW;
            const int iy = y0 + py, ix = x0 + px;
            const char* s = zero;
            if (live && pp < C::NPIX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                s = X + ((size_t)(img * p.H + iy) * p.W + ix) * pix_b + ((cq ^ swz_halo(pp)) << 4);
            src[j] = s;
        }
        const unsigned base = lds0 + B::PB + (pi_k & 1) * C::PATCH;
#pragma unroll
        for (int j = 0; j < PSLOTS; ++j) {
            const int i = wave + 8 * j;
            if (i < NI_P) {                                        // (wave-uniform)
                const bool is_zero = src[j] == zero;
                glds16v(is_zero ? src[j] : src[j] + (size_t)pi_cb * 128, __builtin_amdgcn_readfirstlane(base + i * 1024));
            }
        }
        ++pi_k;
        if (++pi_cb == ncb) { pi_cb = 0; ++pi_tile; }
    };

    if (my_tiles == 0) return;
    issue_patch();
#pragma unroll
    for (int u = 0; u < NWS - 1; ++u) issue_w();

    typedef typename Mma<T>::u4v U;
    f32x4 acc[RW][4];
    const int row0 = wave * RW;                                        // first output row of this wave in the tile
    int xoff[8][2], woff[2];
    int pbuf = 0;                                                      // patch buffer (0 / 1) whose offset xoff holds
    // (rebuilt behind every tile's tail instead of being kept: sixteen registers the tail needs)
    auto set_xoff = [&]() {
        int lr_ = lr;
        asm volatile("" : "+v"(lr_));   // (opaque: hipcc otherwise hoists the lane-dependent parts out of the tile loop and spills them)
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pp = row0 * PW + lr_;
                xoff[m][h] = B::PB + pbuf * C::PATCH + pp * 128 + (((2 * g + h) ^ swz_halo(pp + m)) << 4);
            }
    };
    set_xoff();
#pragma unroll
    for (int h = 0; h < 2; ++h) woff[h] = lr * 128 + (((2 * g + h) ^ swz_halo(lr)) << 4);
    int s = 0;                                                         // step (= weight unit) index
    U wH[4], wL[4];
    uint4 x0[2];
    // fragments of the unit in ring slot (s + 1) -- rows 16 a + lr for every unit kind: legal once barrier s is passed (see the protocol)
    auto ahead_frag = [&](int a) {
        const char* const Wn = smem + B::PB + 2 * C::PATCH + ((s + 1) & (NWS - 1)) * C::WU;
        wH[a] = Mma<T>::as_u4v(lds16(Wn + woff[0] + a * 16 * 128));
        wL[a] = Mma<T>::as_u4v(lds16(Wn + woff[1] + a * 16 * 128));
    };
    auto ahead_w = [&]() {
#pragma unroll
        for (int a = 0; a < 4; ++a) ahead_frag(a);
    };
    auto ahead = [&](auto tn) {   // ... and the first pixel row of the conv2 unit with tap TN
        constexpr int TN = decltype(tn)::value, k = (TN / 3) * PW + TN % 3;
        ahead_w();
        x0[0] = lds16(smem + xoff[k & 7][0] + k * 128);
        x0[1] = lds16(smem + xoff[k & 7][1] + k * 128);
    };
    auto ahead_x0 = [&]() {   // the first pixel row of the next tile's first unit (tap 0: patch pixel 0 of the wave's rows)
        set_xoff();
        x0[0] = lds16(smem + xoff[0][0]);
        x0[1] = lds16(smem + xoff[0][1]);
    };
    wait_vm_barrier<(NWS - 2)>();
    --s;
    ahead(IC<0>());
    ++s;
    const float* const bl = (const float*)(smem + B::BIAS);
    unsigned long long bad = 0;   // lanes that packed a value fp16 cannot carry: raised once, behind the pipeline (hipcc waits vmcnt(0) there)
    for (int t = 0; t < my_tiles; ++t) {
        // ---------------------------------------------------------------- phase A: conv3_halo's unit loop
        for (int cb = 0; cb < ncb; ++cb) {
            auto step = [&](auto tc) {
                constexpr int TAP = decltype(tc)::value, DY = TAP / 3, DX = TAP % 3;
                if (cb == 1) wait_vm_barrier<B::wait(9 + TAP, true)>();
                else if (t > 0) wait_vm_barrier<B::wait(TAP, true)>();
                else wait_vm_barrier<B::wait(TAP, false)>();
                if constexpr (TAP == 0) issue_patch();   // next stage into the patch buffer every wave is done reading
                issue_w();                            // unit s + NWS - 1 into the slot of unit s - 1
                if (TAP == 0 && cb == 0) {   // (first unit of a tile)
#pragma unroll
                    for (int r = 0; r < RW; ++r)
#pragma unroll
                        for (int a = 0; a < 4; ++a) acc[r][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                U cH[4], cL[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    cH[a] = wH[a]; cL[a] = wL[a];
                    asm volatile("" : "+v"(cH[a]), "+v"(cL[a]));
                }
                uint4 xf[RW][2];
                xf[0][0] = x0[0]; xf[0][1] = x0[1];
                auto rdx = [&](int r) {
                    const int k = (r + DY) * PW + DX;
                    xf[r][0] = lds16(smem + xoff[k & 7][0] + k * 128);
                    xf[r][1] = lds16(smem + xoff[k & 7][1] + k * 128);
                };
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    U xH, xL;
                    Mma<T>::regroup(xf[r][0], xf[r][1], xH, xL);
                    asm volatile("" : "+v"(xH), "+v"(xL));
                    __builtin_amdgcn_sched_barrier(0);
                    if (r + 1 < RW) {
                        rdx(r + 1);
                    } else {
                        if constexpr (TAP == 8) {
                            const int d = pbuf ? -C::PATCH : C::PATCH;
                            pbuf ^= 1;
#pragma unroll
                            for (int m = 0; m < 8; ++m) { xoff[m][0] += d; xoff[m][1] += d; }
                        }
                        // (behind the tile's last conv2 unit the next unit is the first tail unit: same rows; the pixel row it also fetches
                        // is read again behind the last tail unit)
                        ahead(IC<(TAP + 1) % 9>());
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int a = 0; a < 4; ++a) Mma<T>::three(cH[a], cL[a], xH, xL, acc[r][a]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                ++s;
            };
            step(IC<0>()); step(IC<1>()); step(IC<2>()); step(IC<3>()); step(IC<4>());
            step(IC<5>()); step(IC<6>()); step(IC<7>()); step(IC<8>());
        }
        // ---------------------------------------------------------------- the tile's pixels; identity of group 0
        const int tile = first + t * G;
        const int tx = tile % tiles_x, r_ = tile / tiles_x, ty = r_ % tiles_y, img = r_ / tiles_y;
        const int ox = tx * C::TW + lr;
        bool pix_ok[RW];
        size_t pix[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int oy = ty * C::TH + row0 + r;
            pix_ok[r] = oy < p.H && ox < p.W;
            pix[r] = pix_ok[r] ? (size_t)(img * p.H + oy) * p.W + ox : 0;
        }
        u32x4 idr[RW][2];
        auto load_idn = [&](int q) {
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const char* a = pix_ok[r] ? (const char*)p.idn + (pix[r] * 256 + (size_t)(32 * q + 16 * c + 4 * g)) * 4 : zero;
                    gload16(idr[r][c], a);
                }
        };
        load_idn(0);
        // ---------------------------------------------------------------- t2 -> conv3's pixel operand
        U tH[RW][2], tL[RW][2];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            uint4 ch[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float4 bv = *(const float4*)(bl + a * 16 + 4 * g);
                float v[4] = {fmaxf(acc[r][a][0] * p.ws2 + bv.x, 0.f), fmaxf(acc[r][a][1] * p.ws2 + bv.y, 0.f),
                              fmaxf(acc[r][a][2] * p.ws2 + bv.z, 0.f), fmaxf(acc[r][a][3] * p.ws2 + bv.w, 0.f)};
                bad |= f16x2_out_of_range(v) & __builtin_amdgcn_ballot_w64(pix_ok[r]);
                ch[a] = Chunk<T>::pack(v);
            }
            Mma<T>::regroup(ch[0], ch[1], tH[r][0], tL[r][0]);
            Mma<T>::regroup(ch[2], ch[3], tH[r][1], tL[r][1]);
        }
        f32x4 accC[RW][4];
        if constexpr (PHC) {
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int a = 0; a < 4; ++a) accC[r][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        // ---------------------------------------------------------------- eight groups of 32 conv3 channels
        auto group = [&](auto qc) {
            constexpr int Q = decltype(qc)::value, LB = 18 + Q * B::GS;
            // ---- B: conv3 for channels 32 Q .. 32 Q + 31
            wait_vm_barrier<B::wait(LB, true)>();
            issue_w();
            // (no second copy of the fragments here -- the tail has no registers for one: a fragment is used for both rows, then the same
            // registers request the next unit's fragment, which lands under the MFMAs of the fragments behind it and the epilogue)
            f32x4 ya[RW][2];
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) ya[r][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {   // fragment a = rows 16 a + lr = (K-step a / 2, column block a % 2)
                asm volatile("" : "+v"(wH[a]), "+v"(wL[a]));
#pragma unroll
                for (int r = 0; r < RW; ++r) Mma<T>::three(wH[a], wL[a], tH[r][a >> 1], tL[r][a >> 1], ya[r][a & 1]);
                __builtin_amdgcn_sched_barrier(0);
                ahead_frag(a);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (!PHC && Q == 7) ahead_x0();
            ++s;
            // identity of this group: issued behind the previous group's y stores (behind step 17 for group 0); younger are only the weight
            // units issued since
            if constexpr (Q == 0 || !PHC) wait_vm_only<1>(); else wait_vm_only<2>();
            U yH[RW], yL[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                uint4 ch[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    bind16(idr[r][c]);
                    const u32x4 u = idr[r][c];
                    float rv[4];
                    Chunk<T>::unpack(make_uint4(u.x, u.y, u.z, u.w), rv);
                    const float4 bv = *(const float4*)(bl + 64 + 32 * Q + 16 * c + 4 * g);
                    float v[4] = {fmaxf(ya[r][c][0] * p.ws3 + bv.x + rv[0], 0.f), fmaxf(ya[r][c][1] * p.ws3 + bv.y + rv[1], 0.f),
                                  fmaxf(ya[r][c][2] * p.ws3 + bv.z + rv[2], 0.f), fmaxf(ya[r][c][3] * p.ws3 + bv.w + rv[3], 0.f)};
                    bad |= f16x2_out_of_range(v) & __builtin_amdgcn_ballot_w64(pix_ok[r]);
                    ch[c] = Chunk<T>::pack(v);
                    char* dst = pix_ok[r] ? (char*)p.y + (pix[r] * 256 + (size_t)(32 * Q + 16 * c + 4 * g)) * 4 : (char*)p.dump_page + lane * 16;
                    *(uint4*)dst = ch[c];
                }
                if constexpr (PHC) Mma<T>::regroup(ch[0], ch[1], yH[r], yL[r]);
            }
            __builtin_amdgcn_sched_barrier(0);   // (the stores above are issued before the loads below: the counts of the proof)
            if constexpr (Q < 7) load_idn(Q + 1);
            if constexpr (PHC) {
                // ---- C: K-step Q of the next conv1 from the rounded y
                wait_vm_barrier<B::wait(LB + 1, true)>();
                issue_w();
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    asm volatile("" : "+v"(wH[a]), "+v"(wL[a]));
#pragma unroll
                    for (int r = 0; r < RW; ++r) Mma<T>::three(wH[a], wL[a], yH[r], yL[r], accC[r][a]);
                    __builtin_amdgcn_sched_barrier(0);
                    ahead_frag(a);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (Q == 7) ahead_x0();
                ++s;
            }
        };
        group(IC<0>()); group(IC<1>()); group(IC<2>()); group(IC<3>());
        group(IC<4>()); group(IC<5>()); group(IC<6>()); group(IC<7>());
        if constexpr (PHC) {   // ---- t1' = ReLU(accC * ws1 + bias1'): 8 stores per wave
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float4 bv = *(const float4*)(bl + 320 + a * 16 + 4 * g);
                    float v[4] = {fmaxf(accC[r][a][0] * p.ws1 + bv.x, 0.f), fmaxf(accC[r][a][1] * p.ws1 + bv.y, 0.f),
                                  fmaxf(accC[r][a][2] * p.ws1 + bv.z, 0.f), fmaxf(accC[r][a][3] * p.ws1 + bv.w, 0.f)};
                    bad |= f16x2_out_of_range(v) & __builtin_amdgcn_ballot_w64(pix_ok[r]);
                    char* dst = pix_ok[r] ? (char*)p.t1n + (pix[r] * 64 + (size_t)(a * 16 + 4 * g)) * 4 : (char*)p.dump_page + lane * 16;
                    *(uint4*)dst = Chunk<T>::pack(v);
                }
        }
    }
    wait_vm_only<0>();
    f16x2_raise(bad);
}

template <bool PHC>
static int launch_bneck_tail_t(const BneckTailParams& p_in, hipStream_t stream) {
    using B = BtCfg<PHC>;
    BneckTailParams p = p_in;
    OCRVI_TRY(ring_pages(&p.zero_page, &p.dump_page));
    int n_cu = 0;
    OCRVI_TRY(device_cus(&n_cu));
    const HaloPlan pl = conv3_halo_plan(p.n_img, p.H, p.W, 64, n_cu);   // (phase A's tile: one column tile of 64)
    auto kern = bneck_tail_kernel<PHC>;
    OCRVI_TRY(ensure_max_smem((const void*)kern, B::SMEM));
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(512), B::SMEM, stream, p, pl.tiles_x, pl.tiles_y);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

}  // namespace ocrvi
