// Kernel-level hooks of the C ABI (include/ocrvi.h, "test/bench hooks"): run ONE production kernel on
// caller-supplied float32 NCHW device tensors.  They allocate scratch, convert layouts, time with HIP events on
// their own stream (the MFMA kernels' hooks; the memory-bound kernels' hooks at the end take no timing arguments),
// and synchronise -- test infrastructure around the same kernels the model graphs launch.
#include <algorithm>
#include <memory>

#include "conv_launch.h"
#include "model.h"

using namespace ocrvi;
namespace ocrvi {
OCRVI_RANGE_FLAG_TU()   // binds this unit's f16x2 range-flag pointer (common.h)
}

namespace {
template <typename T>
__global__ void nchw_f32_to_nhwc_kernel(const float* __restrict__ x, T* __restrict__ y, int N, int C, int HW) {
    const size_t total = (size_t)N * C * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t t = i / C;
        const int p = (int)(t % HW), n = (int)(t / HW);
        store_elem<T>(y, i, x[((size_t)n * C + c) * HW + p]);
    }
}
int to_nhwc(int dt, const float* x, void* y, int N, int C, int HW, hipStream_t s) {
    const size_t total = (size_t)N * C * HW;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    switch (dt) {
        case OCRVI_F32: hipLaunchKernelGGL(nchw_f32_to_nhwc_kernel<float>, dim3(grid), dim3(256), 0, s, x, (float*)y, N, C, HW); break;
        case OCRVI_BF16: hipLaunchKernelGGL(nchw_f32_to_nhwc_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, x, (bf16_t*)y, N, C, HW); break;
        case OCRVI_F16: hipLaunchKernelGGL(nchw_f32_to_nhwc_kernel<f16_t>, dim3(grid), dim3(256), 0, s, x, (f16_t*)y, N, C, HW); break;
        case OCRVI_F16X2: hipLaunchKernelGGL(nchw_f32_to_nhwc_kernel<f16x2_t>, dim3(grid), dim3(256), 0, s, x, (f16x2_t*)y, N, C, HW); break;
        default: set_error("unknown dtype %d", dt); return OCRVI_EINVAL;
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
// [N][18][P] offsets + [N][9][P] masks -> [N*P][32] rows (the layout the offset conv's epilogue writes)
__global__ void pack_offsets_kernel(const float* __restrict__ off, const float* __restrict__ mask, float* __restrict__ o, int N, int P) {
    const size_t total = (size_t)N * P * 32;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i & 31);
        const size_t m = i >> 5;
        const int p = (int)(m % P), n = (int)(m / P);
        float v = 0.f;
        if (c < 18) v = off[((size_t)n * 18 + c) * P + p];
        else if (c < 27) v = mask[((size_t)n * 9 + (c - 18)) * P + p];
        o[i] = v;
    }
}
struct Scratch {
    std::vector<void*> p;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Scratch() {
        for (void* q : p) (void)hipFree(q);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
    }
    int alloc(size_t bytes, void** out) {
        OCRVI_HIP(hipMalloc(out, bytes ? bytes : 16));
        p.push_back(*out);
        return OCRVI_OK;
    }
    int init() {
        unsigned* flag = nullptr;
        OCRVI_TRY(range_flag_bind(&flag));   // the hooks run f16x2 kernels too: ocrvi_range_flag / ocrvi_range_reset see them
        OCRVI_HIP(hipStreamCreate(&s));
        OCRVI_HIP(hipEventCreate(&e0));
        OCRVI_HIP(hipEventCreate(&e1));
        return OCRVI_OK;
    }
};
template <typename F>
int timed(Scratch& sc, int iters, float* avg_ms, F&& launch) {
    OCRVI_TRY(launch());  // warm-up / the run whose output is checked
    if (iters > 0 && avg_ms) {
        OCRVI_HIP(hipEventRecord(sc.e0, sc.s));
        for (int i = 0; i < iters; ++i) OCRVI_TRY(launch());
        OCRVI_HIP(hipEventRecord(sc.e1, sc.s));
        OCRVI_HIP(hipEventSynchronize(sc.e1));
        float ms = 0.f;
        OCRVI_HIP(hipEventElapsedTime(&ms, sc.e0, sc.e1));
        *avg_ms = ms / iters;
    }
    return OCRVI_OK;
}
}  // namespace

// res: null, or device float32 NCHW [N, Co, Ho, Wo] added in the epilogue before the activation (RES_SAME)
// out_raw: the caller's own device output buffer (NHWC [>= N Ho Wo][Co] of `dtype` elements, ocrvi_test_deform_conv_raw), or null for one
// of exactly N Ho Wo rows allocated here
static int test_deform_conv(int device, int dtype, const float* x, const float* offset, const float* mask, const float* weight_host,
                            const float* bias_host, const float* res, int N, int C, int H, int W, int Co, int stride, int relu, void* out_raw,
                            float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && offset && mask && weight_host && out && (stride == 1 || stride == 2), OCRVI_EINVAL, "test_deform_conv: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, Co, C, 3, 3, 1, AM_DCN, dtype);
    OCRVI_TRY(upload_packed(st, pc, AM_DCN, &L));
    void *xn = nullptr, *yn = out_raw, *offs = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * dtype_size(dtype), &xn));
    if (!yn) OCRVI_TRY(sc.alloc((size_t)N * Ho * Wo * Co * dtype_size(dtype), &yn));
    OCRVI_TRY(sc.alloc((size_t)N * Ho * Wo * 32 * 4, &offs));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    hipLaunchKernelGGL(pack_offsets_kernel, dim3(1024), dim3(256), 0, sc.s, offset, mask, (float*)offs, N, Ho * Wo);
    OCRVI_HIP(hipGetLastError());
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C;
    Tensor ty; ty.p = yn; ty.n = N; ty.h = Ho; ty.w = Wo; ty.c = Co;
    Tensor tr = ty;
    ConvOpts o;
    o.sh = o.sw = stride; o.pad = 1; o.act = relu ? ACT_RELU : ACT_NONE; o.offs = (const float*)offs;
    if (res) {   // the residual has the output's shape and element type
        void* rn = nullptr;
        OCRVI_TRY(sc.alloc((size_t)N * Ho * Wo * Co * dtype_size(dtype), &rn));
        OCRVI_TRY(to_nhwc(dtype, res, rn, N, Co, Ho * Wo, sc.s));
        tr.p = rn;
        o.res = &tr; o.res_mode = RES_SAME;
    }
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, ty, o); }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, N, Ho, Wo, Co, Co, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_deform_conv(int device, int dtype, const float* x, const float* offset, const float* mask,
                                      const float* weight_host, const float* bias_host, int N, int C, int H, int W, int Co, int stride,
                                      int relu, float* out, int iters, float* avg_ms) {
    return test_deform_conv(device, dtype, x, offset, mask, weight_host, bias_host, nullptr, N, C, H, W, Co, stride, relu, nullptr, out, iters,
                            avg_ms);
}

extern "C" int ocrvi_test_deform_conv_res(int device, int dtype, const float* x, const float* offset, const float* mask,
                                          const float* weight_host, const float* bias_host, const float* res, int N, int C, int H, int W,
                                          int Co, int stride, int relu, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(res, OCRVI_EINVAL, "test_deform_conv_res: res is required");
    return test_deform_conv(device, dtype, x, offset, mask, weight_host, bias_host, res, N, C, H, W, Co, stride, relu, nullptr, out, iters, avg_ms);
}

extern "C" int ocrvi_test_deform_conv_raw(int device, int dtype, const float* x, const float* offset, const float* mask,
                                          const float* weight_host, const float* bias_host, const float* res, int N, int C, int H, int W,
                                          int Co, int stride, int relu, void* out_raw, float* out) {
    OCRVI_CHECK(out_raw, OCRVI_EINVAL, "test_deform_conv_raw: out_raw is null");
    return test_deform_conv(device, dtype, x, offset, mask, weight_host, bias_host, res, N, C, H, W, Co, stride, relu, out_raw, out, 0, nullptr);
}

// Host only: what launch_conv would do with the deformable 3x3 (pad 1) that ocrvi_test_deform_conv runs, on a device of n_cu compute
// units.  No device is touched.
extern "C" int ocrvi_test_dcn_plan(int dtype, int N, int C, int H, int W, int Co, int stride, int n_cu, int32_t plan[8]) {
    OCRVI_CHECK(plan && dtype_valid(dtype) && N > 0 && C > 0 && H > 0 && W > 0 && Co > 0 && (stride == 1 || stride == 2) && n_cu > 0,
                OCRVI_EINVAL, "test_dcn_plan: bad argument");
    const int bke = conv_bke(dtype);
    OCRVI_CHECK(C % bke == 0 && Co > 64, OCRVI_EINVAL, "test_dcn_plan: needs C %% %d == 0 and Co > 64 (got %d, %d)", bke, C, Co);
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    ConvParams p;   // as conv() fills it for pack_conv's layer; the pointers are only tested for being there
    p.x = p.w = (const void*)256; p.out = (void*)256; p.offs = (const float*)256;
    p.n_img = N; p.H = H; p.W = W; p.OH = Ho; p.OW = Wo; p.M = N * Ho * Wo;
    p.KH = 3; p.SH = p.SW = stride; p.PH = p.PW = 1;
    p.Cin = p.Cin_g = C;
    p.N_g = Co; p.Np = cdiv(Co, 128) * 128; p.Kp = 9 * C;
    p.ldo = Co;
    const bool pipe = dcn_pipe_eligible(p, dtype);
    OCRVI_CHECK(pipe || !dcn_pipe_packing(dtype, C), OCRVI_EINVAL, "test_dcn_plan: packed for the pipelined kernel but not eligible for it");
    if (pipe) {
        const DcnPipePlan pl = dcn_pipe_plan((int)dtype_size(dtype), N, Ho, Wo, p.Np, C, n_cu);
        plan[0] = 1; plan[1] = 128; plan[2] = pl.bn; plan[3] = pl.patch_lw;
        plan[4] = pl.total; plan[5] = pl.grid; plan[6] = cdiv(pl.total, pl.grid); plan[7] = pl.nk;
    } else {   // conv_gemm's AM_DCN mode: one tile per workgroup (OCRVI_DCN_TILE_M, the test knob of the launcher, is not looked at)
        const int bn = p.Np % 256 == 0 ? 256 : 128, bm = dcn_gemm_tile_m(p.M, p.Np, n_cu);
        const int total = cdiv(p.M, bm) * (p.Np / bn);
        plan[0] = 0; plan[1] = bm; plan[2] = bn; plan[3] = 0;
        plan[4] = total; plan[5] = total; plan[6] = 1; plan[7] = p.Kp / bke;
    }
    return OCRVI_OK;
}

// out_raw: the caller's own device output buffer (NHWC [>= N H/4 W/4][64] of `dtype` elements, ocrvi_test_stem_pool_raw), or null for one of
// exactly that many rows allocated here
static int test_stem_pool(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int H, int W, int fused,
                          void* out_raw, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && weight_host && bias_host && out && N > 0 && H >= 8 && W >= 8 && H % 4 == 0 && W % 4 == 0, OCRVI_EINVAL, "test_stem_pool: bad argument");
    OCRVI_CHECK(!fused || dtype == OCRVI_F16X2, OCRVI_EINVAL, "test_stem_pool: the fused kernel is the f16x2 form");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, 64, 3, 7, 7, 1, AM_ROWS, dtype);
    OCRVI_TRY(upload_packed(st, pc, AM_ROWS, &L));
    const int Hp = H + 6, Wp = W + 8;
    // (the raw form names its kernel: the fused one must be what the detector would take for this stem)
    OCRVI_CHECK(!out_raw || !fused || stem_pool_eligible(dtype, pc.N_g, pc.Kp, pc.KH, H, W), OCRVI_EINVAL,
                "test_stem_pool_raw: this call does not take the fused kernel (OCRVI_STEM_FUSED=0?)");
    void *xp = nullptr, *sn = nullptr, *yn = out_raw;
    OCRVI_TRY(sc.alloc((size_t)N * Hp * Wp * 4 * dtype_size(dtype), &xp));
    OCRVI_TRY(sc.alloc((size_t)N * (H / 2) * (W / 2) * 64 * dtype_size(dtype), &sn));
    if (!yn) OCRVI_TRY(sc.alloc((size_t)N * (H / 4) * (W / 4) * 64 * dtype_size(dtype), &yn));
    OCRVI_TRY(k_nchw3_to_nhwc4_pad(dtype, x, xp, N, H, W, 3, 3, Hp, Wp, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xp; tx.n = N; tx.h = Hp; tx.w = Wp; tx.c = 4;
    Tensor ts; ts.p = sn; ts.n = N; ts.h = H / 2; ts.w = W / 2; ts.c = 64;
    ConvOpts o;
    o.sh = o.sw = 2; o.pad = 3; o.act = ACT_RELU; o.Hp = Hp; o.Wp = Wp;
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() -> int {
        if (fused) return k_stem_pool(dtype, xp, L.w, L.bias, L.wscale, yn, N, H, W, Hp, Wp, sc.s);
        OCRVI_TRY(conv(r, L, tx, ts, o));
        return k_maxpool3x3s2(dtype, sn, yn, N, H / 2, W / 2, 64, sc.s);
    }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, N, H / 4, W / 4, 64, 64, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_stem_pool(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int H, int W,
                                    int fused, float* out, int iters, float* avg_ms) {
    return test_stem_pool(device, dtype, x, weight_host, bias_host, N, H, W, fused, nullptr, out, iters, avg_ms);
}

extern "C" int ocrvi_test_stem_pool_raw(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int H, int W,
                                        int fused, void* out_raw, float* out) {
    OCRVI_CHECK(out_raw, OCRVI_EINVAL, "test_stem_pool_raw: out_raw is null");
    return test_stem_pool(device, dtype, x, weight_host, bias_host, N, H, W, fused, out_raw, out, 0, nullptr);
}

extern "C" int ocrvi_test_conv(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int C,
                               int H, int W, int Co, int ksize, int sh, int sw, int groups, int act, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && weight_host && out && (ksize == 1 || ksize == 3) && groups >= 1 && C % groups == 0 && Co % groups == 0, OCRVI_EINVAL,
                "test_conv: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / sh + 1, Wo = (W + 2 * pad - ksize) / sw + 1;
    const int amode = ksize == 1 ? AM_CONV1 : AM_CONV3;
    DeviceStore st;
    ConvLayer L;
    // OCRVI_TEST_PADC=n (timing experiments only; the result is then meaningless): give the activation rows a channel stride of C + n
    const int padc = getenv("OCRVI_TEST_PADC") ? atoi(getenv("OCRVI_TEST_PADC")) : 0;
    // (as a model's loader would: a stride-1 3x3 with a bias + ReLU / none epilogue asks for conv3_halo's weight form)
    const bool halo = ksize == 3 && sh == 1 && sw == 1 && (act == ACT_NONE || act == ACT_RELU) && padc % 4 == 0;
    PackedConv pc = pack_conv(weight_host, bias_host, Co, C / groups, ksize, ksize, groups, amode, dtype, halo);
    OCRVI_TRY(upload_packed(st, pc, amode, &L));
    void *xn = nullptr, *yn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * (C + padc) * dtype_size(dtype), &xn));
    OCRVI_TRY(sc.alloc((size_t)N * Ho * Wo * Co * dtype_size(dtype), &yn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C + padc;
    Tensor ty; ty.p = yn; ty.n = N; ty.h = Ho; ty.w = Wo; ty.c = Co;
    ConvOpts o;
    o.sh = sh; o.sw = sw; o.pad = pad; o.act = act;
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, ty, o); }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, N, Ho, Wo, Co, Co, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// Stride-1 conv (1x1, or 3x3 pad 1) with a residual in the epilogue: out = act(conv(x) + bias + res).  res_mode RES_SAME: res is
// [N, Co, H, W] (Bottleneck conv3, BasicBlock conv2); RES_UP2: res is [N, Co, H/2, W/2], added nearest-2x upsampled (the FPN laterals,
// neck.py:36-38).  The residual is converted to the mode's element type, as the model's own residuals are.
extern "C" int ocrvi_test_conv_res(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, const float* res, int N,
                                   int C, int H, int W, int Co, int ksize, int res_mode, int act, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && weight_host && out && (ksize == 1 || ksize == 3) && N > 0 && C > 0 && H > 0 && W > 0 && Co > 0 && dtype_valid(dtype),
                OCRVI_EINVAL, "test_conv_res: bad argument");
    OCRVI_CHECK(act == ACT_NONE || act == ACT_RELU || act == ACT_GELU, OCRVI_EINVAL, "test_conv_res: unknown activation %d", act);
    OCRVI_CHECK(res ? (res_mode == RES_SAME || res_mode == RES_UP2) : res_mode == RES_NONE, OCRVI_EINVAL,
                "test_conv_res: res_mode %d %s a residual (1 = same shape, 2 = half resolution)", res_mode, res ? "with" : "without");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int amode = ksize == 1 ? AM_CONV1 : AM_CONV3;
    DeviceStore st;
    ConvLayer L;
    // (as a model's loader would: a 3x3 that runs WITHOUT a residual asks for conv3_halo's weight form; with one it must not -- conv3_halo
    // takes no residual and launch_conv rejects quartet weights everywhere else)
    const bool halo = !res && ksize == 3 && (act == ACT_NONE || act == ACT_RELU);
    PackedConv pc = pack_conv(weight_host, bias_host, Co, C, ksize, ksize, 1, amode, dtype, halo);
    OCRVI_TRY(upload_packed(st, pc, amode, &L));
    void *xn = nullptr, *yn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * dtype_size(dtype), &xn));
    OCRVI_TRY(sc.alloc((size_t)N * H * W * Co * dtype_size(dtype), &yn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C;
    Tensor ty; ty.p = yn; ty.n = N; ty.h = H; ty.w = W; ty.c = Co;
    Tensor tr = ty;
    ConvOpts o;
    o.pad = ksize / 2; o.act = act;
    if (res) {
        if (res_mode == RES_UP2) { tr.h = H / 2; tr.w = W / 2; }   // (odd H or W: launch_conv refuses the call before anything reads it)
        void* rn = nullptr;
        OCRVI_TRY(sc.alloc(tr.pixels() * Co * dtype_size(dtype), &rn));
        OCRVI_TRY(to_nhwc(dtype, res, rn, N, Co, tr.h * tr.w, sc.s));
        tr.p = rn;
        o.res = &tr; o.res_mode = res_mode;
    }
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, ty, o); }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, N, H, W, Co, Co, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// A 3x3 (pad 1) or 1x1 convolution, grouped and strided, with the recogniser's epilogues, written straight into the caller's buffer.
// res: null, or device float32 NCHW [N, Co, Ho, Wo]; it keeps fp32 when the output is fp32 (out_f32, or an fp32 model) and is cast to the
// compute type otherwise.  in_place: the residual is copied into out_raw and that one buffer is residual and output, as LocalMixing's
// second convolution runs on the residual stream (rec_model.hip).  The weights are packed in the chunk form (dense stride-1 f16x2 layers
// that a loader packs for conv3_halo are ocrvi_test_conv's).
extern "C" int ocrvi_test_conv_raw(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, const float* res, int N,
                                   int C, int H, int W, int Co, int ksize, int sh, int sw, int groups, int act, int res_post, int out_f32,
                                   int in_place, void* out_raw, float* out) {
    OCRVI_CHECK(x && weight_host && out && out_raw && (ksize == 1 || ksize == 3) && N > 0 && H > 0 && W > 0 && sh > 0 && sw > 0 && groups >= 1 &&
                    C > 0 && Co > 0 && C % groups == 0 && Co % groups == 0 && dtype_valid(dtype),
                OCRVI_EINVAL, "test_conv_raw: bad argument");
    OCRVI_CHECK(act == ACT_NONE || act == ACT_RELU || act == ACT_GELU, OCRVI_EINVAL, "test_conv_raw: unknown activation %d", act);
    const bool f32o = out_f32 || dtype == OCRVI_F32;
    OCRVI_CHECK(!in_place || (res && f32o), OCRVI_EINVAL, "test_conv_raw: in_place needs a residual and an fp32 output");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / sh + 1, Wo = (W + 2 * pad - ksize) / sw + 1;
    const int amode = ksize == 1 ? AM_CONV1 : AM_CONV3;
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, Co, C / groups, ksize, ksize, groups, amode, dtype);
    OCRVI_TRY(upload_packed(st, pc, amode, &L));
    void* xn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * dtype_size(dtype), &xn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C;
    Tensor ty; ty.p = out_raw; ty.n = N; ty.h = Ho; ty.w = Wo; ty.c = Co; ty.f32 = f32o;
    Tensor tr = ty;
    ConvOpts o;
    o.sh = sh; o.sw = sw; o.pad = pad; o.act = act;
    if (res) {   // the residual has the output's shape and element type
        const int rdt = f32o ? OCRVI_F32 : dtype;
        void* rn = out_raw;
        if (!in_place) OCRVI_TRY(sc.alloc((size_t)N * Ho * Wo * Co * dtype_size(rdt), &rn));
        OCRVI_TRY(to_nhwc(rdt, res, rn, N, Co, Ho * Wo, sc.s));
        tr.p = rn;
        o.res = &tr; o.res_mode = RES_SAME; o.res_post = res_post;
    }
    OCRVI_TRY(conv(r, L, tx, ty, o));
    OCRVI_TRY(k_nhwc_to_nchw_f32(f32o ? OCRVI_F32 : dtype, out_raw, out, N, Ho, Wo, Co, Co, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// Host only: which kernel launch_conv gives the 3x3 (pad 1) convolution that ocrvi_test_conv_raw runs, on a device of n_cu compute units,
// and gconv32's tiling from the function its launcher uses.  No device is touched.
extern "C" int ocrvi_test_gconv_plan(int dtype, int N, int C, int H, int W, int Co, int sh, int sw, int groups, int out_f32, int has_res,
                                     int n_cu, int32_t plan[12]) {
    OCRVI_CHECK(plan && dtype_valid(dtype) && N > 0 && H > 0 && W > 0 && sh > 0 && sw > 0 && groups >= 1 && C > 0 && Co > 0 && C % groups == 0 &&
                    Co % groups == 0 && n_cu > 0,
                OCRVI_EINVAL, "test_gconv_plan: bad argument");
    const int bke = conv_bke(dtype), bn = conv_bn_for(Co / groups);
    const bool f32o = out_f32 || dtype == OCRVI_F32;
    ConvParams p;   // as conv() fills it for pack_conv's layer; the pointers are only tested for alignment
    p.x = p.w = (const void*)256; p.out = (void*)256; p.bias = (const float*)256;
    p.n_img = N; p.H = H; p.W = W; p.OH = (H - 1) / sh + 1; p.OW = (W - 1) / sw + 1; p.M = N * p.OH * p.OW;
    p.KH = 3; p.SH = sh; p.SW = sw; p.PH = p.PW = 1;
    p.Cin = C; p.Cin_g = C / groups; p.groups = groups;
    p.N_g = Co / groups; p.Np = cdiv(p.N_g, bn) * bn; p.Kp = cdiv(9 * p.Cin_g, bke) * bke;
    p.ldo = Co; p.out_f32 = f32o ? 1 : 0;
    if (has_res) { p.res = (const void*)256; p.res_mode = RES_SAME; p.ldr = Co; p.res_f32 = f32o ? 1 : 0; }
    for (int i = 0; i < 12; ++i) plan[i] = 0;
    plan[10] = groups; plan[11] = p.Kp / bke;
    if (dtype_size(dtype) == 2 && gconv32_eligible(p, AM_CONV3, 2)) {
        const Gconv32Plan pl = gconv32_plan(N, H, W, groups, n_cu);
        plan[0] = 1; plan[3] = pl.th; plan[4] = pl.nbx; plan[5] = pl.bands_y; plan[6] = pl.bands_x;
        plan[7] = pl.grid_x; plan[8] = pl.tiles_min; plan[9] = pl.tiles_max;
        return OCRVI_OK;
    }
    if ((dtype == OCRVI_F16X2 && conv3_halo_eligible(p, AM_CONV3, dtype)) || gemm_ring_eligible(p, AM_CONV3, dtype)) {
        plan[0] = 2;   // conv3_halo or the ring GEMM: not this hook's to describe
        return OCRVI_OK;
    }
    plan[1] = 128; plan[2] = bn;                                    // launch_mode: conv_gemm, one tile per workgroup
    plan[7] = cdiv(p.M, 128) * (p.Np / bn); plan[8] = plan[9] = 1;
    return OCRVI_OK;
}

// gconv_x2_kernel alone (gconv_x2.hip): ocrvi_test_conv_raw's call for LocalMixing's f16x2 convolutions, straight to the kernel.  With
// OCRVI_GCONV32=0 the call goes where the model then sends it, through conv() (A/B timing of the two paths with one hook).
extern "C" int ocrvi_test_gconv_x2(int device, const float* x, const float* weight_host, const float* bias_host, const float* res, int N, int C, int H,
                                   int W, int act, int res_post, int out_f32, int in_place, int max_workgroups, void* out_raw, float* out, int iters,
                                   float* avg_ms) {
    OCRVI_CHECK(x && weight_host && out && out_raw && N > 0 && H > 0 && W > 0 && C >= 64 && C % 32 == 0, OCRVI_EINVAL, "test_gconv_x2: bad argument");
    OCRVI_CHECK(act == ACT_NONE || act == ACT_RELU || act == ACT_GELU, OCRVI_EINVAL, "test_gconv_x2: unknown activation %d", act);
    OCRVI_CHECK(!in_place || (res && out_f32), OCRVI_EINVAL, "test_gconv_x2: in_place needs a residual and an fp32 output");
    const int dtype = OCRVI_F16X2, groups = C / 32;
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, C, 32, 3, 3, groups, AM_CONV3, dtype);
    OCRVI_TRY(upload_packed(st, pc, AM_CONV3, &L));
    void* xn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * 4, &xn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    void* rn = nullptr;
    if (res) {   // fp32 beside an fp32 output, f16x2 otherwise (which the kernel does not take)
        rn = out_raw;
        if (!in_place) OCRVI_TRY(sc.alloc((size_t)N * H * W * C * 4, &rn));
        OCRVI_TRY(to_nhwc(out_f32 ? OCRVI_F32 : dtype, res, rn, N, C, H * W, sc.s));
    }
    Tensor tx = wrap(xn, N, H, W, C, false), ty = wrap(out_raw, N, H, W, C, out_f32 != 0), tr = wrap(rn, N, H, W, C, out_f32 != 0);
    ConvOpts o;
    o.pad = 1; o.act = act; o.res_post = res_post;
    if (res) { o.res = &tr; o.res_mode = RES_SAME; }
    const ConvParams p = fill_conv_params(L, tx, ty, o);
    if (gconv32_on()) {
        OCRVI_CHECK(gconv_x2_eligible(p, dtype), OCRVI_EINVAL, "test_gconv_x2: the kernel does not take this call (out_f32 %d, res %d, res_post %d)",
                    out_f32, res != nullptr, res_post);
        OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return k_gconv_x2(p, sc.s, max_workgroups); }));
    } else {
        OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return launch_conv_dt(dtype, p, AM_CONV3, sc.s); }));
    }
    OCRVI_TRY(k_nhwc_to_nchw_f32(out_f32 ? OCRVI_F32 : dtype, out_raw, out, N, H, W, C, C, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// Host only: the tiling k_gconv_x2 launches on a device of n_cu compute units.  No device is touched.
extern "C" int ocrvi_test_gconv_x2_plan(int N, int C, int H, int W, int n_cu, int max_workgroups, int32_t plan[10]) {
    OCRVI_CHECK(plan && N > 0 && H > 0 && W > 0 && C >= 64 && C % 32 == 0 && n_cu > 0, OCRVI_EINVAL, "test_gconv_x2_plan: bad argument");
    const GconvX2Plan pl = gconv_x2_plan(N, H, W, C / 32, n_cu, max_workgroups);
    const int32_t v[10] = {pl.bh, pl.nbx, pl.bands_y, pl.bands_x, pl.ntile, pl.grid_x, pl.tiles_min, pl.tiles_max, C / 32, pl.smem};
    for (int i = 0; i < 10; ++i) plan[i] = v[i];
    return OCRVI_OK;
}

namespace {
// The ConvParams of a dense stride-1 3x3 (pad 1) f16x2 layer with a bias and ReLU / none, as conv() fills them for a layer whose loader
// asked pack_conv for conv3_halo's weight form (`quartets`: whether the packer gave it)
ConvParams halo_conv_params(const void* x, const void* w, void* out, int N, int C, int H, int W, int Co, int Np, int act, bool quartets) {
    ConvParams p;
    p.x = x; p.w = w; p.out = out; p.bias = (const float*)256;
    p.n_img = N; p.H = p.OH = H; p.W = p.OW = W; p.M = N * H * W;
    p.KH = 3; p.SH = p.SW = 1; p.PH = p.PW = 1;
    p.Cin = p.Cin_g = C;
    p.N_g = Co; p.Np = Np; p.Kp = 9 * C;
    p.ldo = Co; p.act = act;
    p.w_quartets = quartets ? 1 : 0;
    return p;
}
}  // namespace

// conv3_halo_kernel alone (conv3_halo.h), f16x2, straight into the caller's buffer: OCRVI_EINVAL unless the packer gives the quartet form
// and launch_conv sends this call to conv3_halo.
extern "C" int ocrvi_test_conv3_halo_raw(int device, const float* x, const float* weight_host, const float* bias_host, int N, int C, int H, int W,
                                         int Co, int act, void* out_raw, float* out) {
    OCRVI_CHECK(x && weight_host && out && out_raw && N > 0 && C > 0 && H > 0 && W > 0 && Co > 0, OCRVI_EINVAL, "test_conv3_halo_raw: bad argument");
    OCRVI_CHECK(act == ACT_NONE || act == ACT_RELU, OCRVI_EINVAL, "test_conv3_halo_raw: activation %d (none or ReLU)", act);
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int dt = OCRVI_F16X2;
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, Co, C, 3, 3, 1, AM_CONV3, dt, true);
    OCRVI_CHECK(pc.quartets, OCRVI_EINVAL, "test_conv3_halo_raw: %d -> %d is not packed as quartets (OCRVI_CONV3_HALO=0?)", C, Co);
    OCRVI_TRY(upload_packed(st, pc, AM_CONV3, &L));
    void* xn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * 4, &xn));
    OCRVI_CHECK(conv3_halo_eligible(halo_conv_params(xn, L.w, out_raw, N, C, H, W, Co, pc.Np, act, true), AM_CONV3, dt), OCRVI_EINVAL,
                "test_conv3_halo_raw: this call does not take conv3_halo");
    OCRVI_TRY(to_nhwc(dt, x, xn, N, C, H * W, sc.s));
    Runner r(dt, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C;
    Tensor ty; ty.p = out_raw; ty.n = N; ty.h = H; ty.w = W; ty.c = Co;
    ConvOpts o;
    o.pad = 1; o.act = act;
    OCRVI_TRY(conv(r, L, tx, ty, o));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dt, out_raw, out, N, H, W, Co, Co, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// Host only: the launch of the three halo-tile kernels of the f16x2 detector on a device of n_cu compute units, from the functions their
// launchers launch on (conv3_halo_plan, stem_pool_plan) and the predicates their callers dispatch on.  No device is touched.
extern "C" int ocrvi_test_halo_plan(int kind, int N, int C, int H, int W, int Co, int n_cu, int32_t plan[8]) {
    OCRVI_CHECK(plan && kind >= 0 && kind <= 2 && N > 0 && H > 0 && W > 0 && n_cu > 0, OCRVI_EINVAL, "test_halo_plan: bad argument");
    for (int i = 0; i < 8; ++i) plan[i] = 0;
    if (kind == 2) {   // k_stem_pool (C, Co: the stem's 3 -> 64)
        OCRVI_CHECK(H % 4 == 0 && W % 4 == 0 && H >= 8 && W >= 8, OCRVI_EINVAL, "test_halo_plan: the stem takes H, W = multiples of 4 from 8 up");
        const StemPoolPlan pl = stem_pool_plan(N, H, W, n_cu);
        plan[0] = (stem_pool_eligible(OCRVI_F16X2, 64, 7 * 32, 7, H, W) && pl.total > 0) ? 1 : 0;
        plan[1] = 64; plan[2] = 1; plan[3] = pl.txN; plan[4] = pl.tyN; plan[5] = pl.grid; plan[6] = pl.tiles_min; plan[7] = pl.tiles_max;
        return OCRVI_OK;
    }
    int Np = 64;
    bool taken = true;
    if (kind == 0) {
        OCRVI_CHECK(C > 0 && Co > 0, OCRVI_EINVAL, "test_halo_plan: bad channel counts");
        const int bn = conv_bn_for(Co);
        Np = cdiv(Co, bn) * bn;
        const bool q = conv3_halo_packing(true, OCRVI_F16X2, C, Co, 3, 1, Np);
        taken = q && conv3_halo_eligible(halo_conv_params((const void*)256, (const void*)256, (void*)256, N, C, H, W, Co, Np, ACT_RELU, q), AM_CONV3,
                                         OCRVI_F16X2);
        if (!(Np == 64 || Np == 128 || Np == 256)) return OCRVI_OK;   // (not taken, and no tiling to describe)
    }   // kind 1: launch_bneck_tail (64 -> 64 -> 256 (-> 64) whatever C and Co say); every shape takes it
    const HaloPlan pl = conv3_halo_plan(N, H, W, Np, n_cu);
    plan[0] = taken ? 1 : 0;
    plan[1] = pl.nc; plan[2] = pl.nct; plan[3] = pl.tiles_x; plan[4] = pl.tiles_y; plan[5] = pl.grid; plan[6] = pl.tiles_min; plan[7] = pl.tiles_max;
    return OCRVI_OK;
}

// The fused ResNet-50 layer1 chain (bneck_tail.h), f16x2: t1 [N,64,H,W] -> conv2 3x3 + ReLU -> conv3 1x1 + identity [N,256,H,W] + ReLU = y
// -> (unless no_phase_c) the next block's conv1 1x1 + ReLU = t1n [N,64,H,W].  Weights as the detector's loader packs them.
// y_raw, t1n_raw: the caller's own device output buffers (NHWC f16x2 [>= N H W][256] / [64], ocrvi_test_bneck_tail_raw), or null for ones of
// exactly N H W rows allocated here
static int test_bneck_tail(int device, const float* t1, const float* identity, const float* w2_host, const float* b2_host, const float* w3_host,
                           const float* b3_host, const float* w1_host, const float* b1_host, int N, int H, int W, int no_phase_c, void* y_raw,
                           void* t1n_raw, float* y_out, float* t1n_out, int iters, float* avg_ms) {
    OCRVI_CHECK(t1 && identity && w2_host && w3_host && y_out && N > 0 && H > 0 && W > 0, OCRVI_EINVAL, "test_bneck_tail: bad argument");
    OCRVI_CHECK(no_phase_c || (w1_host && t1n_out), OCRVI_EINVAL, "test_bneck_tail: phase C needs the next conv1's weights and an output");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int dt = OCRVI_F16X2;
    DeviceStore st;
    ConvLayer L2;
    PackedConv pc = pack_conv(w2_host, b2_host, 64, 64, 3, 3, 1, AM_CONV3, dt, true);
    OCRVI_CHECK(pc.quartets, OCRVI_EINVAL, "test_bneck_tail: conv2 is not packed for conv3_halo (OCRVI_CONV3_HALO=0?)");
    OCRVI_TRY(upload_packed(st, pc, AM_CONV3, &L2));
    PackedBneckTail pt = pack_bneck_tail(w3_host, b3_host, no_phase_c ? nullptr : w1_host, no_phase_c ? nullptr : b1_host);
    void* wt = nullptr;
    float* bt = nullptr;
    OCRVI_TRY(st.upload(pt.stream.data(), pt.stream.size(), &wt));
    OCRVI_TRY(st.upload_f32(pt.bias, &bt));
    const size_t P = (size_t)N * H * W;
    void *xn = nullptr, *in = nullptr, *yn = y_raw, *tn = no_phase_c ? nullptr : t1n_raw;
    OCRVI_TRY(sc.alloc(P * 64 * 4, &xn));
    OCRVI_TRY(sc.alloc(P * 256 * 4, &in));
    if (!yn) OCRVI_TRY(sc.alloc(P * 256 * 4, &yn));
    if (!no_phase_c && !tn) OCRVI_TRY(sc.alloc(P * 64 * 4, &tn));
    OCRVI_TRY(to_nhwc(dt, t1, xn, N, 64, H * W, sc.s));
    OCRVI_TRY(to_nhwc(dt, identity, in, N, 256, H * W, sc.s));
    BneckTailParams p;
    p.x = xn; p.w2 = L2.w; p.wt = wt; p.bias2 = L2.bias; p.bias_t = bt; p.idn = in; p.y = yn; p.t1n = tn;
    p.n_img = N; p.H = H; p.W = W;
    p.ws2 = L2.wscale; p.ws3 = pt.ws3; p.ws1 = pt.ws1;
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return launch_bneck_tail(p, sc.s); }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dt, yn, y_out, N, H, W, 256, 256, 0, sc.s));
    if (!no_phase_c) OCRVI_TRY(k_nhwc_to_nchw_f32(dt, tn, t1n_out, N, H, W, 64, 64, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_bneck_tail(int device, const float* t1, const float* identity, const float* w2_host, const float* b2_host,
                                     const float* w3_host, const float* b3_host, const float* w1_host, const float* b1_host, int N, int H, int W,
                                     int no_phase_c, float* y_out, float* t1n_out, int iters, float* avg_ms) {
    return test_bneck_tail(device, t1, identity, w2_host, b2_host, w3_host, b3_host, w1_host, b1_host, N, H, W, no_phase_c, nullptr, nullptr, y_out,
                           t1n_out, iters, avg_ms);
}

extern "C" int ocrvi_test_bneck_tail_raw(int device, const float* t1, const float* identity, const float* w2_host, const float* b2_host,
                                         const float* w3_host, const float* b3_host, const float* w1_host, const float* b1_host, int N, int H,
                                         int W, int no_phase_c, void* y_raw, void* t1n_raw, float* y_out, float* t1n_out) {
    OCRVI_CHECK(y_raw && (no_phase_c || t1n_raw), OCRVI_EINVAL, "test_bneck_tail_raw: an output buffer is null");
    return test_bneck_tail(device, t1, identity, w2_host, b2_host, w3_host, b3_host, w1_host, b1_host, N, H, W, no_phase_c, y_raw, t1n_raw, y_out,
                           t1n_out, 0, nullptr);
}

// The DB head's tail (head.py:13-16 per branch: ConvTranspose2d(64,64,2,2) + BN + ReLU, ConvTranspose2d(64,1,2,2)) as det_model.hip builds and
// launches it: both branches' first deconvolutions packed as ONE grouped pixel-shuffle GEMM (group 0 = binarise, 1 = threshold), the second
// deconvolution's weights as [2][64][4] + 2 biases, the 64 -> 1 dot in the GEMM's epilogue.  groups = 2: the launch sees the whole pack,
// x is [N, 128, OH, OW] (channels 0..63 feed group 0, 64..127 group 1, as the 256 -> 128 head conv leaves them); groups = 1: the launch
// sees the one-group VIEW of the same pack that the binary-only forward takes (never a second pack), x is [N, 64, OH, OW].  binary_only:
// ST_DB_BIN (out = sigmoid of group 0's logits) instead of ST_DB_TAIL (out, out2 = the two logit maps).  Which (store mode, groups, out2)
// combinations are legal is launch_conv's to say: the hook hands them through.
extern "C" int ocrvi_test_db_tail(int device, int dtype, const float* x, const float* dc1_w_bin_host, const float* dc1_b_bin_host,
                                  const float* dc1_w_thr_host, const float* dc1_b_thr_host, const float* dc2_w_bin_host, const float* dc2_b_bin_host,
                                  const float* dc2_w_thr_host, const float* dc2_b_thr_host, int N, int OH, int OW, int groups, int binary_only,
                                  float* out, float* out2, int iters, float* avg_ms) {
    OCRVI_CHECK(x && dc1_w_bin_host && dc1_b_bin_host && dc1_w_thr_host && dc1_b_thr_host && dc2_w_bin_host && dc2_b_bin_host && dc2_w_thr_host &&
                    dc2_b_thr_host && out && N > 0 && OH > 0 && OW > 0 && dtype_valid(dtype),
                OCRVI_EINVAL, "test_db_tail: bad argument");
    OCRVI_CHECK(groups == 1 || groups == 2, OCRVI_EINVAL, "test_db_tail: groups = %d (2: the packed layer, 1: its binarise-branch view)", groups);
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    ConvLayer dc1;
    float* dc2_wb = nullptr;
    {   // det_model.hip, ocrvi_det_create: the head's deconvolutions
        const float* dw[2] = {dc1_w_bin_host, dc1_w_thr_host};
        const float* db[2] = {dc1_b_bin_host, dc1_b_thr_host};
        PackedConv both = pack_deconv2(dw, db, 2, 64, 64, dtype);
        OCRVI_TRY(upload_packed(st, both, AM_CONV1, &dc1));
        dc1.shuffle_co = 64;
        std::vector<float> w2(2 * 64 * 4);
        std::copy(dc2_w_bin_host, dc2_w_bin_host + 256, w2.begin());
        std::copy(dc2_w_thr_host, dc2_w_thr_host + 256, w2.begin() + 256);
        w2.push_back(dc2_b_bin_host[0]);
        w2.push_back(dc2_b_thr_host[0]);
        OCRVI_TRY(st.upload_f32(w2, &dc2_wb));
    }
    ConvLayer L = dc1;
    L.groups = groups;   // (1: det_run's `hdc`, the first group of the shared pack)
    const int Cx = 64 * groups;
    void* xn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * OH * OW * Cx * dtype_size(dtype), &xn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, Cx, OH * OW, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = OH; tx.w = OW; tx.c = Cx;
    Tensor lm; lm.p = out; lm.n = N; lm.h = 4 * OH; lm.w = 4 * OW; lm.c = 1; lm.f32 = true;
    ConvOpts o;
    o.store_mode = binary_only ? ST_DB_BIN : ST_DB_TAIL; o.out2 = binary_only ? nullptr : out2; o.offs = dc2_wb;
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, lm, o); }));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// The 27-channel offset / mask conv of DeformableConv2d on its own (dcn.py:42-46): 3x3, pad 1, stride 1 or 2; out = device float32
// [N, Ho, Wo, 32]: channels 0..17 offsets, 18..26 sigmoid(mask logits), 27..31 zero -- the layout the deformable conv kernels consume.
extern "C" int ocrvi_test_offset_conv(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int C,
                                      int H, int W, int stride, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && weight_host && bias_host && out && (stride == 1 || stride == 2) && N > 0 && C > 0, OCRVI_EINVAL, "test_offset_conv: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, 27, C, 3, 3, 1, AM_CONV3, dtype);
    OCRVI_TRY(upload_packed(st, pc, AM_CONV3, &L));
    void* xn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * dtype_size(dtype), &xn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = xn; tx.n = N; tx.h = H; tx.w = W; tx.c = C;
    Tensor ty; ty.p = out; ty.n = N; ty.h = Ho; ty.w = Wo; ty.c = 32; ty.f32 = true;
    ConvOpts o;
    o.sh = o.sw = stride; o.pad = 1; o.store_mode = ST_DCN_OFFS;
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, ty, o); }));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

namespace {
// out_raw: the caller's own device output buffer ([>= M][N] of the output's element type, ocrvi_test_gemm_raw), or null for one of exactly
// M rows allocated here
int test_gemm_impl(int device, int dtype, const float* a, const float* weight_host, const float* bias_host, const float* res, int M, int K, int N,
                   int act, int res_post, int out_f32, void* out_raw, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(a && weight_host && out && M > 0 && K > 0 && N > 0, OCRVI_EINVAL, "test_gemm: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const bool f32o = out_f32 || dtype == OCRVI_F32;   // (f16x2: its own 4-byte format unless out_f32)
    DeviceStore st;
    ConvLayer L;
    PackedConv pc = pack_conv(weight_host, bias_host, N, K, 1, 1, 1, AM_CONV1, dtype);
    OCRVI_TRY(upload_packed(st, pc, AM_CONV1, &L));
    void *an = nullptr, *yn = out_raw, *rn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)M * K * dtype_size(dtype), &an));
    if (!yn) OCRVI_TRY(sc.alloc((size_t)M * N * (f32o ? 4 : dtype_size(dtype)), &yn));
    OCRVI_TRY(k_cast_from_f32(dtype, a, an, (size_t)M * K, sc.s));
    Runner r(dtype, sc.s, (void*)256, 0);
    Tensor tx; tx.p = an; tx.n = 1; tx.h = 1; tx.w = M; tx.c = K;
    Tensor ty; ty.p = yn; ty.n = 1; ty.h = 1; ty.w = M; ty.c = N; ty.f32 = f32o;
    Tensor tr = ty;
    ConvOpts o;
    o.act = act;
    if (res) {  // the residual has the output's element type
        if (f32o) {
            rn = (void*)res;
        } else {
            OCRVI_TRY(sc.alloc((size_t)M * N * dtype_size(dtype), &rn));
            OCRVI_TRY(k_cast_from_f32(dtype, res, rn, (size_t)M * N, sc.s));
        }
        tr.p = rn;
        o.res = &tr; o.res_mode = RES_SAME; o.res_post = res_post;
    }
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return conv(r, L, tx, ty, o); }));
    if (f32o) OCRVI_HIP(hipMemcpyAsync(out, yn, (size_t)M * N * 4, hipMemcpyDeviceToDevice, sc.s));
    else OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, 1, 1, M * N, 1, 1, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}
}  // namespace

extern "C" int ocrvi_test_gemm(int device, int dtype, const float* a, const float* weight_host, const float* bias_host, const float* res, int M,
                               int K, int N, int act, int res_post, int out_f32, float* out, int iters, float* avg_ms) {
    return test_gemm_impl(device, dtype, a, weight_host, bias_host, res, M, K, N, act, res_post, out_f32, nullptr, out, iters, avg_ms);
}

extern "C" int ocrvi_test_gemm_raw(int device, int dtype, const float* a, const float* weight_host, const float* bias_host, const float* res,
                                   int M, int K, int N, int act, int res_post, int out_f32, void* out_raw, float* out) {
    OCRVI_CHECK(out_raw, OCRVI_EINVAL, "test_gemm_raw: out_raw is null");
    return test_gemm_impl(device, dtype, a, weight_host, bias_host, res, M, K, N, act, res_post, out_f32, out_raw, out, 0, nullptr);
}

// Host only: what launch_gemm_ring would do with a plain NHWC 1x1 (amode 0; K = C_in) or stride-1 3x3 (amode 1; K = 9 C_in) of M output
// pixels on a device of n_cu compute units.  No device is touched.
extern "C" int ocrvi_test_ring_plan(int dtype, int amode, int M, int K, int N, int out_f32, int has_res, int n_cu, int32_t plan[8]) {
    OCRVI_CHECK(plan && dtype_valid(dtype) && (amode == AM_CONV1 || amode == AM_CONV3) && M > 0 && K > 0 && N > 0 && n_cu > 0, OCRVI_EINVAL,
                "test_ring_plan: bad argument");
    OCRVI_CHECK(amode == AM_CONV1 || K % 9 == 0, OCRVI_EINVAL, "test_ring_plan: K = %d of a 3x3 is not a multiple of 9", K);
    const int bke = conv_bke(dtype), bn = conv_bn_for(N), taps = amode == AM_CONV3 ? 9 : 1;
    const bool f32o = out_f32 || dtype == OCRVI_F32;
    ConvParams p;   // as conv() fills it for pack_conv's layer; the pointers are only tested for alignment
    p.x = p.w = (const void*)256; p.out = (void*)256;
    p.n_img = 1; p.H = p.OH = 1; p.W = p.OW = M; p.M = M;
    p.KH = taps == 9 ? 3 : 1; p.PH = p.PW = taps == 9 ? 1 : 0;
    p.Cin = p.Cin_g = K / taps;
    p.N_g = N; p.Np = cdiv(N, bn) * bn; p.Kp = cdiv(K, bke) * bke;
    p.ldo = N; p.out_f32 = f32o ? 1 : 0;
    p.identity_pix = taps == 1 ? 1 : 0;
    if (has_res) { p.res = (const void*)256; p.res_mode = RES_SAME; p.ldr = N; p.res_f32 = f32o ? 1 : 0; }
    const RingPlan pl = ring_plan((int)dtype_size(dtype), dtype == OCRVI_F16X2, amode, M, p.Np, p.Kp, out_f32 != 0, n_cu);
    plan[0] = (gemm_ring_eligible(p, amode, dtype) && pl.ntiles <= n_cu) ? 1 : 0;
    plan[1] = pl.bm; plan[2] = pl.bn; plan[3] = pl.sps; plan[4] = pl.f32o ? 1 : 0;
    plan[5] = pl.grid; plan[6] = pl.tiles_min; plan[7] = pl.tiles_max;
    return OCRVI_OK;
}

extern "C" int ocrvi_test_attention(int device, int dtype, const float* qkv, int B, int N, int heads, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(qkv && out && B > 0 && N > 0 && heads > 0, OCRVI_EINVAL, "test_attention: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int D = heads * 32;
    const size_t nin = (size_t)B * N * 3 * D, nout = (size_t)B * N * D;
    void *q = nullptr, *o = nullptr;
    OCRVI_TRY(sc.alloc(nin * dtype_size(dtype), &q));
    OCRVI_TRY(sc.alloc(nout * dtype_size(dtype), &o));
    OCRVI_TRY(k_cast_from_f32(dtype, qkv, q, nin, sc.s));
    void* asc = nullptr;
    if (const size_t sb = attention_scratch_bytes(dtype, B, N, heads)) OCRVI_TRY(sc.alloc(sb, &asc));
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return k_attention(dtype, q, o, B, N, heads, sc.s, asc); }));
    // [B*N][D] T -> float32 (same layout): a C=1 "NHWC -> NCHW" copy is a plain cast
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, o, out, 1, 1, (int)nout, 1, 1, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

namespace {
// xn_raw: the caller's own device xn buffer ([>= M][D] of `dtype`, ocrvi_test_mlp_raw), or null for one of exactly M rows allocated here
int test_mlp_impl(int device, int dtype, float* x, const float* ln_g_host, const float* ln_b_host, const float* w1_host, const float* b1_host,
                  const float* w2_host, const float* b2_host, const float* next_g_host, const float* next_b_host, int want_xn, int M, int D,
                  void* xn_raw, float* xn_out, int iters, float* avg_ms) {
    OCRVI_CHECK(x && ln_g_host && ln_b_host && w1_host && b1_host && w2_host && b2_host && M > 0, OCRVI_EINVAL, "test_mlp: bad argument");
    OCRVI_CHECK(mlp_fused_eligible(dtype, D), OCRVI_EINVAL, "test_mlp: the fused MLP needs bf16, f16 or f16x2 and D in {128, 256, 384} (got dtype %d, D %d)", dtype, D);
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    std::vector<char> packed;
    pack_mlp_stream(w1_host, w2_host, D, dtype, packed);
    void* ws = nullptr;
    float *g = nullptr, *b = nullptr, *b1 = nullptr, *b2 = nullptr, *ng = nullptr, *nb = nullptr;
    OCRVI_TRY(st.upload(packed.data(), packed.size(), &ws));
    OCRVI_TRY(st.upload(ln_g_host, (size_t)D * 4, (void**)&g));
    OCRVI_TRY(st.upload(ln_b_host, (size_t)D * 4, (void**)&b));
    OCRVI_TRY(st.upload(b1_host, (size_t)4 * D * 4, (void**)&b1));
    OCRVI_TRY(st.upload(b2_host, (size_t)D * 4, (void**)&b2));
    if (next_g_host) {
        OCRVI_TRY(st.upload(next_g_host, (size_t)D * 4, (void**)&ng));
        OCRVI_TRY(st.upload(next_b_host, (size_t)D * 4, (void**)&nb));
    }
    void *xn = xn_raw, *x0 = nullptr;
    if (want_xn && !xn) OCRVI_TRY(sc.alloc((size_t)M * D * dtype_size(dtype), &xn));
    OCRVI_TRY(sc.alloc((size_t)M * D * 4, &x0));   // the kernel updates x in place: every timed repeat starts from the caller's x
    OCRVI_HIP(hipMemcpyAsync(x0, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, sc.s));
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() {
        return k_mlp_fused(dtype, (float*)x0, xn, g, b, ng, nb, ws, b1, b2, M, D, sc.s);
    }));
    // one clean application for the result
    OCRVI_TRY(k_mlp_fused(dtype, x, xn, g, b, ng, nb, ws, b1, b2, M, D, sc.s));
    if (want_xn && xn_out) OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, xn, xn_out, 1, 1, M * D, 1, 1, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}
}  // namespace

extern "C" int ocrvi_test_mlp(int device, int dtype, float* x, const float* ln_g_host, const float* ln_b_host, const float* w1_host, const float* b1_host,
                              const float* w2_host, const float* b2_host, const float* next_g_host, const float* next_b_host, int want_xn, int M, int D,
                              float* xn_out, int iters, float* avg_ms) {
    return test_mlp_impl(device, dtype, x, ln_g_host, ln_b_host, w1_host, b1_host, w2_host, b2_host, next_g_host, next_b_host, want_xn, M, D, nullptr,
                         xn_out, iters, avg_ms);
}

extern "C" int ocrvi_test_mlp_raw(int device, int dtype, float* x, const float* ln_g_host, const float* ln_b_host, const float* w1_host,
                                  const float* b1_host, const float* w2_host, const float* b2_host, const float* next_g_host, const float* next_b_host,
                                  int M, int D, void* xn_raw, float* xn_out, int iters, float* avg_ms) {
    OCRVI_CHECK(xn_raw, OCRVI_EINVAL, "test_mlp_raw: xn_raw is null");
    return test_mlp_impl(device, dtype, x, ln_g_host, ln_b_host, w1_host, b1_host, w2_host, b2_host, next_g_host, next_b_host, 1, M, D, xn_raw, xn_out,
                         iters, avg_ms);
}

// lin_x2_kernel alone (lin_x2.hip), the pattern of test_gemm_impl: fp32 in, cast on the device; out_raw: the caller's own output buffer or null
extern "C" int ocrvi_test_lin_x2(int device, const float* a, const float* weight_host, const float* bias_host, int M, int K, int N, int max_workgroups,
                                 void* out_raw, float* out, int iters, float* avg_ms) {
    OCRVI_CHECK(a && weight_host && out && M > 0, OCRVI_EINVAL, "test_lin_x2: bad argument");
    OCRVI_CHECK(lin_x2_eligible(OCRVI_F16X2, K, N), OCRVI_EINVAL, "test_lin_x2: needs K in {256, 384} and N %% 32 == 0, N <= 2048 (got K %d, N %d)", K, N);
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    std::vector<char> packed;
    pack_lin_x2_stream(weight_host, N, K, packed);
    void* ws = nullptr;
    float* b = nullptr;
    OCRVI_TRY(st.upload(packed.data(), packed.size(), &ws));
    if (bias_host) OCRVI_TRY(st.upload(bias_host, (size_t)N * 4, (void**)&b));
    void *an = nullptr, *yn = out_raw;
    OCRVI_TRY(sc.alloc((size_t)M * K * 4, &an));
    if (!yn) OCRVI_TRY(sc.alloc((size_t)M * N * 4, &yn));
    OCRVI_TRY(k_cast_from_f32(OCRVI_F16X2, a, an, (size_t)M * K, sc.s));
    OCRVI_TRY(timed(sc, iters, avg_ms, [&]() { return k_lin_x2(an, ws, b, yn, M, K, N, sc.s, max_workgroups); }));
    OCRVI_TRY(k_nhwc_to_nchw_f32(OCRVI_F16X2, yn, out, 1, 1, M * N, 1, 1, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

// Host only: the bytes a weight packer hands to its kernel (include/ocrvi.h lists the kinds).  No HIP call.
extern "C" int ocrvi_test_pack_stream(int kind, const float* w0, const float* w1, int d0, int d1, void* out, size_t cap, size_t* size,
                                      float scales[2]) {
    OCRVI_CHECK(w0 && size && scales, OCRVI_EINVAL, "test_pack_stream: null argument");
    std::vector<char> bytes;
    scales[0] = scales[1] = 1.f;
    if (kind == 0) {
        OCRVI_CHECK(lin_x2_eligible(OCRVI_F16X2, d1, d0), OCRVI_EINVAL, "test_pack_stream: lin_x2 needs K in {256, 384}, N %% 32 == 0 (N %d, K %d)", d0, d1);
        pack_lin_x2_stream(w0, d0, d1, bytes);
    } else if (kind == 1) {
        OCRVI_CHECK(w1 && mlp_fused_eligible(d1, d0), OCRVI_EINVAL, "test_pack_stream: no fused MLP for D %d, dtype %d", d0, d1);
        pack_mlp_stream(w0, w1, d0, d1, bytes);
    } else if (kind == 2) {
        PackedBneckTail pt = pack_bneck_tail(w0, nullptr, w1, nullptr);
        bytes.swap(pt.stream);
        scales[0] = pt.ws3;
        scales[1] = pt.ws1;
    } else if (kind == 3 || kind == 4) {
        OCRVI_CHECK(d0 > 0 && d1 > 0, OCRVI_EINVAL, "test_pack_stream: bad channel counts");
        PackedConv pc = pack_conv(w0, nullptr, d1, d0, 3, 3, 1, kind == 3 ? AM_CONV3 : AM_DCN, OCRVI_F16X2, kind == 3);
        OCRVI_CHECK(kind == 3 ? pc.quartets : dcn_pipe_packing(OCRVI_F16X2, d0), OCRVI_EINVAL, "test_pack_stream: %d -> %d is not packed as quartets", d0, d1);
        bytes.swap(pc.bytes);
        scales[0] = pc.wscale;
    } else {
        set_error("test_pack_stream: unknown kind %d", kind);
        return OCRVI_EINVAL;
    }
    *size = bytes.size();
    if (!out) return OCRVI_OK;
    OCRVI_CHECK(cap >= bytes.size(), OCRVI_EINVAL, "test_pack_stream: %zu bytes needed, %zu given", bytes.size(), cap);
    memcpy(out, bytes.data(), bytes.size());
    return OCRVI_OK;
}

// Host only: the two row swizzles as the packers call them (rows 0 .. 63), and the launchers' grid rule (common.h)
extern "C" int ocrvi_test_swizzles(int32_t swz128_rows[64], int32_t swz_halo_rows[64]) {
    OCRVI_CHECK(swz128_rows && swz_halo_rows, OCRVI_EINVAL, "test_swizzles: null out");
    for (int r = 0; r < 64; ++r) {
        swz128_rows[r] = swz128(r);
        swz_halo_rows[r] = swz_halo(r);
    }
    return OCRVI_OK;
}
extern "C" int ocrvi_test_persistent_grid(int ntile, int slots, int32_t* grid) {
    OCRVI_CHECK(grid && ntile > 0, OCRVI_EINVAL, "test_persistent_grid: bad argument");
    *grid = persistent_grid(ntile, slots);
    return OCRVI_OK;
}

// ---- the memory-bound kernels of kernels.hip, one hook each (no timing arguments: nothing benchmarks these)
namespace {
// [n] T -> float32 (same order): a C = 1 "NHWC -> NCHW" copy is a plain cast
int cast_to_f32(int dtype, const void* x, float* y, size_t n, hipStream_t s) {
    OCRVI_CHECK(n < ((size_t)1 << 31), OCRVI_EINVAL, "test hook: tensor too large");
    return k_nhwc_to_nchw_f32(dtype, x, y, 1, 1, (int)n, 1, 1, 0, s);
}
}  // namespace

extern "C" int ocrvi_test_layernorm(int device, int dtype, const float* x, int x_f32, int out_f32, const float* gamma_host, const float* beta_host,
                                    int rows, int D, float* out) {
    OCRVI_CHECK(x && gamma_host && beta_host && out && rows > 0 && D > 0 && dtype_valid(dtype), OCRVI_EINVAL, "test_layernorm: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    float *g = nullptr, *b = nullptr;
    OCRVI_TRY(st.upload(gamma_host, (size_t)D * 4, (void**)&g));
    OCRVI_TRY(st.upload(beta_host, (size_t)D * 4, (void**)&b));
    const size_t n = (size_t)rows * D;
    const void* xin = x;
    void* yo = out;
    if (!x_f32) {
        void* xt = nullptr;
        OCRVI_TRY(sc.alloc(n * dtype_size(dtype), &xt));
        OCRVI_TRY(k_cast_from_f32(dtype, x, xt, n, sc.s));
        xin = xt;
    }
    if (!out_f32) OCRVI_TRY(sc.alloc(n * dtype_size(dtype), &yo));
    OCRVI_TRY(k_layernorm(dtype, xin, x_f32, yo, out_f32, g, b, rows, D, sc.s));
    if (!out_f32) OCRVI_TRY(cast_to_f32(dtype, yo, out, n, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_frm_vertical(int device, int dtype, const float* kv, const float* vq_host, int B, int H, int W, int D, float* out) {
    OCRVI_CHECK(kv && vq_host && out && B > 0 && H > 0 && W > 0 && D > 0 && D % 4 == 0 && dtype_valid(dtype), OCRVI_EINVAL,
                "test_frm_vertical: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    float* vq = nullptr;
    OCRVI_TRY(st.upload(vq_host, (size_t)D * 4, (void**)&vq));
    const size_t nin = (size_t)B * H * W * 2 * D, nout = (size_t)B * W * D;
    void *kt = nullptr, *ot = nullptr;
    OCRVI_TRY(sc.alloc(nin * dtype_size(dtype), &kt));
    OCRVI_TRY(sc.alloc(nout * dtype_size(dtype), &ot));
    OCRVI_TRY(k_cast_from_f32(dtype, kv, kt, nin, sc.s));
    OCRVI_TRY(k_frm_vertical(dtype, kt, vq, ot, B, H, W, D, sc.s));
    OCRVI_TRY(cast_to_f32(dtype, ot, out, nout, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_asf(int device, int dtype, const float* p2, const float* p3, const float* p4, const float* p5, const float* w_host,
                              const float* b_host, int N, int H, int W, float* out) {
    OCRVI_CHECK(p2 && p3 && p4 && p5 && w_host && b_host && out && N > 0 && H >= 8 && W >= 8 && dtype_valid(dtype), OCRVI_EINVAL,
                "test_asf: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    DeviceStore st;
    float *w = nullptr, *b = nullptr;
    OCRVI_TRY(st.upload(w_host, (size_t)4 * 1024 * 4, (void**)&w));
    OCRVI_TRY(st.upload(b_host, (size_t)4 * 4, (void**)&b));
    const float* src[4] = {p2, p3, p4, p5};
    void* lv[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < 4; ++l) {
        const int hw = (H >> l) * (W >> l);
        OCRVI_TRY(sc.alloc((size_t)N * hw * 256 * dtype_size(dtype), &lv[l]));
        OCRVI_TRY(to_nhwc(dtype, src[l], lv[l], N, 256, hw, sc.s));
    }
    void *on = nullptr, *scr = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * 256 * dtype_size(dtype), &on));
    OCRVI_TRY(sc.alloc(asf_scratch_bytes(N, H, W), &scr));
    OCRVI_TRY(k_asf(dtype, lv[0], lv[1], lv[2], lv[3], w, b, (float*)scr, on, N, H, W, sc.s));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, on, out, N, H, W, 256, 256, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_maxpool(int device, int dtype, const float* x, int N, int C, int H, int W, float* out) {
    OCRVI_CHECK(x && out && N > 0 && C > 0 && C % 4 == 0 && H > 0 && W > 0 && dtype_valid(dtype), OCRVI_EINVAL, "test_maxpool: bad argument");
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    void *xn = nullptr, *yn = nullptr;
    OCRVI_TRY(sc.alloc((size_t)N * H * W * C * dtype_size(dtype), &xn));
    OCRVI_TRY(sc.alloc((size_t)N * OH * OW * C * dtype_size(dtype), &yn));
    OCRVI_TRY(to_nhwc(dtype, x, xn, N, C, H * W, sc.s));
    OCRVI_TRY(k_maxpool3x3s2(dtype, xn, yn, N, H, W, C, sc.s));
    OCRVI_TRY(k_nhwc_to_nchw_f32(dtype, yn, out, N, OH, OW, C, C, 0, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_db_maps(int device, const float* bin_logits, const float* thresh_logits, float k, float* binary, float* thresh,
                                  float* thresh_binary, size_t n) {
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    OCRVI_TRY(k_db_maps(bin_logits, thresh_logits, k, binary, thresh, thresh_binary, n, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_ctc_logsoftmax(int device, const float* logits, int ld, int B, int T, int C, float* log_probs, int32_t* argmax_ids) {
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    OCRVI_TRY(k_ctc_logsoftmax_argmax(logits, ld, log_probs, argmax_ids, B, T, C, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}

extern "C" int ocrvi_test_ctc_logsoftmax_conf(int device, const float* logits, int ld, int B, int T, int C, float* log_probs,
                                              int32_t* argmax_ids, float* best_lp) {
    OCRVI_HIP(hipSetDevice(device));
    Scratch sc;
    OCRVI_TRY(sc.init());
    OCRVI_TRY(k_ctc_logsoftmax_argmax_conf(logits, ld, log_probs, argmax_ids, best_lp, B, T, C, sc.s));
    OCRVI_HIP(hipStreamSynchronize(sc.s));
    return OCRVI_OK;
}
