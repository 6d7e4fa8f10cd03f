// Host-side plumbing shared by the detection and recognition graphs: device-resident packed weights,
// NHWC tensor views over the caller's workspace, and a conv() wrapper that fills ConvParams.
#pragma once
#include "conv_gemm.h"
#include "kernels.h"

namespace ocrvi {

struct DeviceStore {  // owns every hipMalloc'd weight buffer of a handle
    std::vector<void*> ptrs;
    ~DeviceStore() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    int upload(const void* host, size_t bytes, void** out) {
        void* d = nullptr;
        OCRVI_HIP(hipMalloc(&d, bytes ? bytes : 16));
        ptrs.push_back(d);
        if (bytes) OCRVI_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        *out = d;
        return OCRVI_OK;
    }
    int upload_f32(const std::vector<float>& v, float** out) { return upload(v.data(), v.size() * 4, (void**)out); }
};

struct ConvLayer {
    void* w = nullptr;
    float* bias = nullptr;
    int Np = 0, Kp = 0, N_g = 0, Cin_g = 0, groups = 1, KH = 1, amode = AM_CONV1;
    int shuffle_co = 0;
    float wscale = 1.f;   // f16x2 weight scale (PackedConv::wscale)
    bool quartets = false;   // PackedConv::quartets
};

int upload_packed(DeviceStore& st, const PackedConv& pc, int amode, ConvLayer* L);
// conv weight `name`.w [cout][cin_g][k][k] (+ `name`.b [cout] if has_bias) from the blob; `halo`: a 3x3 layer that only ever runs at
// stride 1 / pad 1 with a bias + ReLU / none epilogue (pack_conv)
int load_conv(DeviceStore& st, const Blob& blob, const std::string& name, int cout, int cin_g, int k, int groups, int amode, int dtype,
              bool has_bias, ConvLayer* L, const float* extra_bias = nullptr, bool halo = false);
int load_vec(DeviceStore& st, const Blob& blob, const std::string& name, int n, float** out);

struct Tensor {  // NHWC view
    void* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
    bool f32 = false;
    size_t pixels() const { return (size_t)n * h * w; }
};
// a view of memory the graph did not get from Runner::alloc: a caller's output map, a shared arena buffer under another shape
inline Tensor wrap(void* p, int n, int h, int w, int c, bool f32) {
    Tensor t;
    t.p = p; t.n = n; t.h = h; t.w = w; t.c = c; t.f32 = f32;
    return t;
}

struct Runner {
    int dtype;
    hipStream_t stream;
    Arena arena;
    Runner(int dt, hipStream_t s, void* ws, size_t bytes) : dtype(dt), stream(s), arena(ws, bytes) {}
    bool dry() const { return arena.planning(); }
    size_t esz(bool f32) const { return f32 ? 4 : dtype_size(dtype); }
    Tensor alloc(int n, int h, int w, int c, bool f32 = false) {
        return wrap(arena.alloc((size_t)n * h * w * c * esz(f32)), n, h, w, c, f32);
    }
};

struct ConvOpts {
    int sh = 1, sw = 1, pad = 0;
    int act = ACT_NONE;
    const Tensor* res = nullptr;
    int res_mode = RES_NONE;
    int res_post = 0;
    int store_mode = ST_NHWC;
    const float* offs = nullptr;  // AM_DCN offsets, or ST_DB_TAIL / ST_DB_BIN second-deconv weights [2][64][4] + biases [2]
    void* out2 = nullptr;         // ST_DB_TAIL: threshold-branch logit map
    int out_coff = 0;
    int cin_off = 0;
    int Hp = 0, Wp = 0;  // AM_ROWS padded input dims
};
// y must be pre-shaped (n,h,w,c, f32) and allocated; x likewise.
int conv(Runner& r, const ConvLayer& L, const Tensor& x, const Tensor& y, const ConvOpts& o);
// The two halves of conv() for callers that route a layer to a kernel of their own (rec_model.hip's LocalMixing convolutions, the test
// hooks): the ConvParams conv() launches with, and its checks of the activation type and the output shape.
ConvParams fill_conv_params(const ConvLayer& L, const Tensor& x, const Tensor& y, const ConvOpts& o);
int check_conv_shapes(const Runner& r, const ConvLayer& L, const Tensor& x, const ConvParams& p, const ConvOpts& o);

// ---------------------------------------------------------------- what every model handle's C entries share
// A handle has `device`, `cfg.dtype` and a RangeWatch `range`.  `check()` validates the handle and the shape; `run(Runner&)` walks the
// graph once: on a planning arena it only measures, on the caller's workspace it launches.  `what` prefixes the messages.

// The end of a *_create: the ring GEMM's scratch pages are allocated now, so that no forward (possibly under graph capture) ever
// allocates; an f16x2 handle gets its view of the device's range flag.  On the handle's device.
int finish_create(int dtype, RangeWatch& range);

// *_workspace_bytes: the peak of the graph's arena use.
template <typename Handle, typename Check, typename Run>
int plan_workspace(const char* what, const Handle* h, size_t* bytes, Check&& check, Run&& run) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "%s: null out", what);
    OCRVI_TRY(check());
    Runner r(h->cfg.dtype, nullptr, nullptr, 0);
    OCRVI_TRY(run(r));
    *bytes = r.arena.peak + 256;
    return OCRVI_OK;
}

// *_forward: `have_args` / `args_msg` is the entry's own null check, made after the shape check.
template <typename Handle, typename Check, typename Run>
int run_forward(const char* what, Handle* h, bool have_args, const char* args_msg, void* workspace, size_t workspace_bytes, void* stream,
                Check&& check, Run&& run) {
    OCRVI_TRY(check());
    OCRVI_CHECK(have_args, OCRVI_EINVAL, "%s: %s", what, args_msg);
    DeviceGuard dg(h->device);  // launches go to the handle's device whatever the caller's current device is
    OCRVI_HIP(dg.err);
    Runner plan(h->cfg.dtype, nullptr, nullptr, 0);
    OCRVI_TRY(run(plan));
    const size_t need = plan.arena.peak + 256;
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    OCRVI_CHECK(((uintptr_t)workspace & 255) == 0, OCRVI_EINVAL, "%s: workspace must be 256-byte aligned", what);
    Runner r(h->cfg.dtype, (hipStream_t)stream, workspace, workspace_bytes);
    OCRVI_TRY(run(r));
    OCRVI_CHECK(!r.arena.overflow, OCRVI_ENOMEM, "%s: workspace overflow", what);
    return h->range.snapshot((hipStream_t)stream);
}

}  // namespace ocrvi
