// DBNet++ inference graph (model/det/dbnet.py:13-17): ResNet-50 or ResNet-18 (backbone.py:12-31), with DCNv2 in layers 2-4
// (backbone.py:39-60, dcn.py:41-59) or plain 3x3 convolutions there, FPN + adaptive scale fusion (neck.py:26-79), DB head
// (head.py:32-48).  NHWC activations in the handle's compute dtype; eval-mode BatchNorm is pre-folded into the conv weights by
// the Python packer.
#include <algorithm>
#include <memory>

#include "model.h"

using namespace ocrvi;

namespace {
const int kBlocks50[4] = {3, 4, 6, 3}, kBlocks18[4] = {2, 2, 2, 2};
const int kWidth[4] = {64, 128, 256, 512};
// One residual block.  Bottleneck (ResNet-50): conv1 1x1, conv2 3x3 (the stride; deformable in layers 2-4), conv3 1x1 + identity.
// BasicBlock (ResNet-18, torchvision.models.resnet.BasicBlock): conv1 3x3 (the stride), conv2 3x3 stride 1 (deformable in layers 2-4,
// backbone.py:39-53 replaces every block's conv2) + identity; no conv3.
struct ResBlock {
    ConvLayer conv1, conv2, off, conv3, down;
    bool dcn = false, has_down = false;
    int stride = 1;
    // f16x2 layer1: conv2 + conv3 (+ the next block's conv1) as one launch (bneck_tail.h); tail_w = the packed stream (pack_bneck_tail)
    void* tail_w = nullptr;
    float* tail_bias = nullptr;
    float tail_ws3 = 1.f, tail_ws1 = 1.f;
    bool tail = false, tail_c = false;   // fused; ... including the next block's conv1
};
}  // namespace

struct ocrvi_det {
    int device = 0;
    ocrvi_det_cfg cfg{};
    DeviceStore store;
    ConvLayer stem;
    std::vector<ResBlock> layers[4];
    ConvLayer lat[4], fpn[4];
    float *asf_w = nullptr, *asf_b = nullptr;
    ConvLayer head_conv, head_dc1;
    float* dc2_wb = nullptr;  // [2][64][4] second-deconv weights followed by the 2 biases
    Tensor tap_c[4], tap_fused;
    bool basic = false;   // ResNet-18: BasicBlocks, no channel expansion
    int expansion = 4;    // block output channels / block width
    RangeWatch range;     // f16x2 only: the device's range flag as of the end of the last forward
};

extern "C" int ocrvi_det_create(int device, const void* blob_p, size_t blob_bytes, const ocrvi_det_cfg* cfg, ocrvi_det** out) {
    OCRVI_CHECK(cfg && out, OCRVI_EINVAL, "det_create: null argument");
    OCRVI_CHECK(dtype_valid(cfg->dtype), OCRVI_EINVAL, "det_create: bad dtype %d", cfg->dtype);
    OCRVI_CHECK(cfg->backbone == 0 || cfg->backbone == 1, OCRVI_EINVAL, "det_create: backbone %d (0 = ResNet-50, 1 = ResNet-18)", cfg->backbone);
    OCRVI_CHECK(cfg->no_dcn == 0 || cfg->no_dcn == 1, OCRVI_EINVAL, "det_create: no_dcn %d (0 or 1)", cfg->no_dcn);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    Blob blob;
    OCRVI_TRY(blob.parse(blob_p, blob_bytes));
    std::unique_ptr<ocrvi_det> h(new ocrvi_det);
    h->device = device;
    h->cfg = *cfg;
    const int dt = cfg->dtype;
    const bool basic = cfg->backbone == 1, use_dcn = cfg->no_dcn == 0;
    h->basic = basic;
    h->expansion = basic ? 1 : 4;
    {   // the blob must be of the architecture the cfg names: a Bottleneck has a conv3, a deformable conv2 its offset / mask conv
        const bool has3 = blob.find("layer1.0.conv3.w") != nullptr, has_off = blob.find("layer2.0.conv2.off.w") != nullptr;
        OCRVI_CHECK(basic || has3, OCRVI_EINVAL, "det_create: cfg.backbone = 0 (ResNet-50) but the blob has no tensor 'layer1.0.conv3.w'");
        OCRVI_CHECK(!basic || !has3, OCRVI_EINVAL,
                    "det_create: cfg.backbone = 1 (ResNet-18) but the blob holds the Bottleneck tensor 'layer1.0.conv3.w'");
        OCRVI_CHECK(!use_dcn || has_off, OCRVI_EINVAL, "det_create: cfg.no_dcn = 0 but the blob has no tensor 'layer2.0.conv2.off.w'");
        OCRVI_CHECK(use_dcn || !has_off, OCRVI_EINVAL,
                    "det_create: cfg.no_dcn = 1 but the blob holds the offset / mask tensor 'layer2.0.conv2.off.w'");
    }
    DeviceStore& st = h->store;
    OCRVI_TRY(load_conv(st, blob, "stem", 64, 3, 7, 1, AM_ROWS, dt, true, &h->stem));
    int inpl = 64;
    const int ex = h->expansion;
    for (int li = 0; li < 4; ++li) {
        const int w = kWidth[li];
        const int nblk = basic ? kBlocks18[li] : kBlocks50[li];
        h->layers[li].resize(nblk);
        for (int b = 0; b < nblk; ++b) {
            ResBlock& bk = h->layers[li][b];
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            bk.dcn = use_dcn && li >= 1;               // backbone.py:28-31: DCN in layer2..4
            bk.stride = (b == 0 && li >= 1) ? 2 : 1;   // torchvision Bottleneck v1.5: stride on the 3x3 (BasicBlock: on conv1)
            bk.has_down = b == 0 && (!basic || li >= 1);   // (ResNet-18's layer1 keeps 64 channels at stride 1: no downsample)
            // (the dense 3x3 layers that run at stride 1 without a residual ask for conv3_halo's weight form)
            if (basic) OCRVI_TRY(load_conv(st, blob, p + ".conv1", w, inpl, 3, 1, AM_CONV3, dt, true, &bk.conv1, nullptr, bk.stride == 1));
            else OCRVI_TRY(load_conv(st, blob, p + ".conv1", w, inpl, 1, 1, AM_CONV1, dt, true, &bk.conv1));
            OCRVI_TRY(load_conv(st, blob, p + ".conv2", w, w, 3, 1, bk.dcn ? AM_DCN : AM_CONV3, dt, true, &bk.conv2, nullptr, !basic && !bk.dcn && bk.stride == 1));
            if (bk.dcn) OCRVI_TRY(load_conv(st, blob, p + ".conv2.off", 27, w, 3, 1, AM_CONV3, dt, true, &bk.off));
            if (!basic) OCRVI_TRY(load_conv(st, blob, p + ".conv3", 4 * w, w, 1, 1, AM_CONV1, dt, true, &bk.conv3));
            if (bk.has_down) OCRVI_TRY(load_conv(st, blob, p + ".down", ex * w, inpl, 1, 1, AM_CONV1, dt, true, &bk.down));
            inpl = ex * w;
        }
        // The fused layer1 chain: by shape only (f16x2, conv2 64 -> 64 packed for conv3_halo, conv3 64 -> 256, the next conv1 256 -> 64);
        // a layer's last block has no successor in the layer (layer2.0.conv1 is 256 -> 128) and ends at y.
        for (int b = 0; b < nblk && !basic && dt == OCRVI_F16X2; ++b) {
            ResBlock& bk = h->layers[li][b];
            if (bk.dcn || bk.stride != 1 || !bk.conv2.quartets || w != 64 || bk.conv2.Np != 64 || bk.conv2.Cin_g != 64) continue;
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const std::string pn = "layer" + std::to_string(li + 1) + "." + std::to_string(b + 1);
            const BlobTensor *w3 = nullptr, *b3 = nullptr, *w1 = nullptr, *b1 = nullptr;
            OCRVI_TRY(blob.get(p + ".conv3.w", 256, 64, 1, 1, &w3));
            OCRVI_TRY(blob.get(p + ".conv3.b", 256, 0, 0, 0, &b3));
            if (b + 1 < nblk) {
                OCRVI_TRY(blob.get(pn + ".conv1.w", 64, 256, 1, 1, &w1));
                OCRVI_TRY(blob.get(pn + ".conv1.b", 64, 0, 0, 0, &b1));
            }
            PackedBneckTail pt = pack_bneck_tail(w3->data, b3->data, w1 ? w1->data : nullptr, b1 ? b1->data : nullptr);
            OCRVI_TRY(st.upload(pt.stream.data(), pt.stream.size(), &bk.tail_w));
            OCRVI_TRY(st.upload_f32(pt.bias, &bk.tail_bias));
            bk.tail_ws3 = pt.ws3; bk.tail_ws1 = pt.ws1;
            bk.tail = true; bk.tail_c = w1 != nullptr;
        }
    }
    for (int i = 0; i < 4; ++i) {
        OCRVI_TRY(load_conv(st, blob, "neck.lat" + std::to_string(i), 256, ex * kWidth[i], 1, 1, AM_CONV1, dt, true, &h->lat[i]));
        OCRVI_TRY(load_conv(st, blob, "neck.fpn" + std::to_string(i), 256, 256, 3, 1, AM_CONV3, dt, true, &h->fpn[i], nullptr, true));
    }
    {
        const BlobTensor *w = nullptr, *b = nullptr;
        OCRVI_TRY(blob.get("neck.asf.w", 4, 1024, 0, 0, &w));
        OCRVI_TRY(blob.get("neck.asf.b", 4, 0, 0, 0, &b));
        OCRVI_TRY(st.upload(w->data, 4096 * 4, (void**)&h->asf_w));
        OCRVI_TRY(st.upload(b->data, 16, (void**)&h->asf_b));
    }
    OCRVI_TRY(load_conv(st, blob, "head.conv", 128, 256, 3, 1, AM_CONV3, dt, true, &h->head_conv, nullptr, true));
    {   // two ConvTranspose2d(64,64,2,2)+BN+ReLU as ONE grouped pixel-shuffle GEMM (group 0 = binarise, 1 = threshold branch)
        std::vector<float> w2(2 * 64 * 4), b2(2);
        const char* names[2] = {"head.bin", "head.thr"};
        const float *dw[2] = {nullptr, nullptr}, *db[2] = {nullptr, nullptr};
        for (int br = 0; br < 2; ++br) {
            const BlobTensor *w = nullptr, *b = nullptr, *ww = nullptr, *bb = nullptr;
            OCRVI_TRY(blob.get(std::string(names[br]) + ".dc1.w", 64, 64, 2, 2, &w));
            OCRVI_TRY(blob.get(std::string(names[br]) + ".dc1.b", 64, 0, 0, 0, &b));
            dw[br] = w->data;
            db[br] = b->data;
            OCRVI_TRY(blob.get(std::string(names[br]) + ".dc2.w", 64, 1, 2, 2, &ww));
            OCRVI_TRY(blob.get(std::string(names[br]) + ".dc2.b", 1, 0, 0, 0, &bb));
            std::copy(ww->data, ww->data + 256, w2.begin() + br * 256);
            b2[br] = bb->data[0];
        }
        PackedConv both = pack_deconv2(dw, db, 2, 64, 64, dt);
        OCRVI_TRY(upload_packed(st, both, AM_CONV1, &h->head_dc1));
        h->head_dc1.shuffle_co = 64;
        w2.insert(w2.end(), b2.begin(), b2.end());
        OCRVI_TRY(st.upload_f32(w2, &h->dc2_wb));
    }
    OCRVI_TRY(finish_create(dt, h->range));
    *out = h.release();
    return OCRVI_OK;
}

extern "C" void ocrvi_det_destroy(ocrvi_det* h) {
    if (!h) return;
    DeviceGuard dg(h->device);
    delete h;
}

static int check_det_shape(const ocrvi_det* h, int N, int H, int W) {
    OCRVI_CHECK(h, OCRVI_EINVAL, "det: null handle");
    OCRVI_CHECK(N > 0 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0, OCRVI_EINVAL,
                "det: input (N=%d,3,%d,%d) needs H and W to be multiples of 32", N, H, W);
    // the stem's GEMM has N*(H/2)*(W/2) rows and the conv kernels index rows with 23 bits (magic-number division)
    OCRVI_CHECK((size_t)N * (H / 2) * (W / 2) < ((size_t)1 << 23), OCRVI_EINVAL,
                "det: batch of %d %dx%d images too large for one call (at most %zu pixels per call: chunk it)", N, H, W, ((size_t)1 << 25) - 1);
    return OCRVI_OK;
}

static ConvOpts conv_opts(int stride, int pad, int act) {
    ConvOpts o;
    o.sh = o.sw = stride; o.pad = pad; o.act = act;
    return o;
}

// ---- stem: conv 7x7/2 + BN + ReLU, maxpool 3x3/2 (torchvision resnet50 via backbone.py:34)
static int det_stem(const ocrvi_det& h, Runner& r, const float* x, int N, int H, int W, Tensor* out) {
    const int dt = h.cfg.dtype, Hp = H + 6, Wp = W + 8;
    Tensor xpad = r.alloc(N, Hp, Wp, 4);
    if (!r.dry()) OCRVI_TRY(k_nchw3_to_nhwc4_pad(dt, x, xpad.p, N, H, W, 3, 3, Hp, Wp, r.stream));
    if (stem_pool_eligible(dt, h.stem.N_g, h.stem.Kp, h.stem.KH, H, W)) {
        // f16x2: one kernel; the half-resolution 64-channel map (the detector's largest tensor) is never written (stem_pool.hip)
        *out = r.alloc(N, H / 4, W / 4, 64);
        if (!r.dry()) OCRVI_TRY(k_stem_pool(dt, xpad.p, h.stem.w, h.stem.bias, h.stem.wscale, out->p, N, H, W, Hp, Wp, r.stream));
        return OCRVI_OK;
    }
    Tensor s = r.alloc(N, H / 2, W / 2, 64);
    ConvOpts o = conv_opts(2, 3, ACT_RELU);
    o.Hp = Hp; o.Wp = Wp;
    OCRVI_TRY(conv(r, h.stem, xpad, s, o));
    *out = r.alloc(N, H / 4, W / 4, 64);
    if (!r.dry()) OCRVI_TRY(k_maxpool3x3s2(dt, s.p, out->p, N, H / 2, W / 2, 64, r.stream));
    return OCRVI_OK;
}

// ---- the pieces of a residual block.  Each block kind below allocates its temporaries in its own order, and the workspace size is the
// peak of that sequence: the order is part of what a block computes, not a detail to tidy.

// The identity branch: x itself, or the block's 1x1 downsample conv of it (the stride) into a fresh buffer of y's shape.
static int identity(Runner& r, const ResBlock& bk, const Tensor& x, const Tensor& y, Tensor* idn) {
    *idn = x;
    if (!bk.has_down) return OCRVI_OK;
    *idn = r.alloc(y.n, y.h, y.w, y.c);
    return conv(r, bk.down, x, *idn, conv_opts(bk.stride, 0, ACT_NONE));
}

// DeformableConv2d.forward (dcn.py:41-59), first half: 27-ch conv -> offsets (ch 0..17) + sigmoid mask (ch 18..26), 32 fp32 per output
// pixel in a fresh buffer; the deformable conv2 that reads them is the caller's.
static int dcn_offsets(Runner& r, const ResBlock& bk, const Tensor& x, int oh, int ow, int stride, const float** offs) {
    Tensor ot = wrap(r.arena.alloc((size_t)x.n * oh * ow * 32 * 4), x.n, oh, ow, 32, true);
    ConvOpts o = conv_opts(stride, 1, ACT_NONE);
    o.store_mode = ST_DCN_OFFS;
    OCRVI_TRY(conv(r, bk.off, x, ot, o));
    *offs = (const float*)ot.p;
    return OCRVI_OK;
}

// Bottleneck: t1, t2, the offsets, then the downsample output.
static int bottleneck(Runner& r, const ResBlock& bk, const Tensor& x, const Tensor& y, int w) {
    Tensor t1 = r.alloc(x.n, x.h, x.w, w);
    Tensor t2 = r.alloc(x.n, y.h, y.w, w);
    OCRVI_TRY(conv(r, bk.conv1, x, t1, conv_opts(1, 0, ACT_RELU)));
    ConvOpts o2 = conv_opts(bk.stride, 1, ACT_RELU);
    if (bk.dcn) OCRVI_TRY(dcn_offsets(r, bk, t1, y.h, y.w, bk.stride, &o2.offs));
    OCRVI_TRY(conv(r, bk.conv2, t1, t2, o2));
    Tensor idn;
    OCRVI_TRY(identity(r, bk, x, y, &idn));
    ConvOpts o3 = conv_opts(1, 0, ACT_RELU);
    o3.res = &idn; o3.res_mode = RES_SAME;
    return conv(r, bk.conv3, t2, y, o3);
}

// BasicBlock: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity); conv1 carries the stride and is never deformable, the residual and the
// final ReLU sit in conv2's epilogue (the pipelined deformable kernel's RES build in the 16-bit / f16x2 modes).  t1, the downsample
// output, then the offsets (conv2 runs at stride 1).
static int basic_block(Runner& r, const ResBlock& bk, const Tensor& x, const Tensor& y, int w) {
    Tensor t1 = r.alloc(x.n, y.h, y.w, w);
    OCRVI_TRY(conv(r, bk.conv1, x, t1, conv_opts(bk.stride, 1, ACT_RELU)));
    Tensor idn;
    OCRVI_TRY(identity(r, bk, x, y, &idn));
    ConvOpts o = conv_opts(1, 1, ACT_RELU);
    o.res = &idn; o.res_mode = RES_SAME;
    if (bk.dcn) OCRVI_TRY(dcn_offsets(r, bk, t1, y.h, y.w, 1, &o.offs));
    return conv(r, bk.conv2, t1, y, o);
}

// The fused layer1 Bottleneck (bneck_tail.h): conv2 + conv3 (+ the next block's conv1 into `t1_next`) as one launch.  `t1` belongs to the
// layer and is already written when the previous block's launch ended in this block's conv1 (`have_t1`); t2 is never allocated, so the
// downsample output is the only temporary.
static int fused_bottleneck(Runner& r, const ResBlock& bk, const Tensor& x, const Tensor& y, const Tensor& t1, bool have_t1,
                            const Tensor& t1_next) {
    if (!have_t1) OCRVI_TRY(conv(r, bk.conv1, x, t1, conv_opts(1, 0, ACT_RELU)));
    Tensor idn;
    OCRVI_TRY(identity(r, bk, x, y, &idn));
    OCRVI_CHECK(idn.c == 256 && y.c == 256 && t1.c == 64 && !idn.f32 && !y.f32, OCRVI_EINVAL, "det: fused layer1 chain on a foreign shape");
    if (r.dry()) return OCRVI_OK;
    BneckTailParams q;
    q.x = t1.p; q.w2 = bk.conv2.w; q.wt = bk.tail_w; q.bias2 = bk.conv2.bias; q.bias_t = bk.tail_bias;
    q.idn = idn.p; q.y = y.p; q.t1n = bk.tail_c ? t1_next.p : nullptr;
    q.n_img = x.n; q.H = y.h; q.W = y.w;
    q.ws2 = bk.conv2.wscale; q.ws3 = bk.tail_ws3; q.ws1 = bk.tail_ws1;
    return launch_bneck_tail(q, r.stream);
}

// ---- one of layers 1..4: *x is the layer's input on entry and its output (the c2..c5 tap, backbone.py:56-60) on return.  Block outputs
// ping-pong between two slots (sized for the layer's output); the last block writes a fresh buffer that stays live as the tap.
// Temporaries of a block are released when it ends, so a chunk of 16 pages keeps ~4 GB less live than with one buffer per block.
static int det_layer(const ocrvi_det& h, Runner& r, int li, Tensor* x) {
    const std::vector<ResBlock>& blocks = h.layers[li];
    Tensor cur = *x;
    const int N = cur.n, w = kWidth[li], cw = h.expansion * w, nb = (int)blocks.size();
    const int lh = cur.h / blocks[0].stride, lw = cur.w / blocks[0].stride;
    Tensor tap = r.alloc(N, lh, lw, cw);                          // the layer's final output
    const size_t slot_mark = r.arena.mark();
    Tensor slot[2] = {r.alloc(N, lh, lw, cw), r.alloc(N, lh, lw, cw)};
    // Fused chains (bneck_tail.h): block b reads t1 from t1pp[b & 1] and writes the next block's into the other one, so both live
    // outside the blocks' own marks (released with the slots).
    const bool fused_layer = !h.basic && blocks[0].tail;
    Tensor t1pp[2];
    if (fused_layer) { t1pp[0] = r.alloc(N, lh, lw, w); t1pp[1] = r.alloc(N, lh, lw, w); }
    bool have_t1 = false;   // the previous block's launch has written this block's t1
    for (int b = 0; b < nb; ++b) {
        const ResBlock& bk = blocks[b];
        Tensor y = b == nb - 1 ? tap : slot[b & 1];               // never the buffer `cur` lives in (slot[(b-1)&1] or the previous tap)
        const size_t block_mark = r.arena.mark();
        if (fused_layer && bk.tail) {
            OCRVI_TRY(fused_bottleneck(r, bk, cur, y, t1pp[b & 1], have_t1, t1pp[(b + 1) & 1]));
            have_t1 = bk.tail_c;
        } else if (h.basic) {
            OCRVI_TRY(basic_block(r, bk, cur, y, w));
        } else {
            OCRVI_TRY(bottleneck(r, bk, cur, y, w));
        }
        r.arena.release(block_mark);  // the block's temporaries are dead
        cur = y;
    }
    r.arena.release(slot_mark);  // both slots are dead once the layer's last block has written the tap
    *x = cur;
    return OCRVI_OK;
}

// ---- neck: FPN top-down (neck.py:26-41) and adaptive scale fusion (neck.py:57-79)
static int det_neck(const ocrvi_det& h, Runner& r, const Tensor* feats, Tensor* fused) {
    const int N = feats[0].n;
    Tensor inner[4], p[4];
    for (int i = 3; i >= 0; --i) {
        inner[i] = r.alloc(N, feats[i].h, feats[i].w, 256);
        ConvOpts o;
        if (i < 3) { o.res = &inner[i + 1]; o.res_mode = RES_UP2; }  // lateral + nearest-2x(last_inner)
        OCRVI_TRY(conv(r, h.lat[i], feats[i], inner[i], o));
        p[i] = r.alloc(N, feats[i].h, feats[i].w, 256);
        OCRVI_TRY(conv(r, h.fpn[i], inner[i], p[i], conv_opts(1, 1, ACT_RELU)));
    }
    *fused = r.alloc(N, p[0].h, p[0].w, 256);
    float* asf_scratch = (float*)r.arena.alloc(asf_scratch_bytes(N, p[0].h, p[0].w));
    if (!r.dry())
        OCRVI_TRY(k_asf(h.cfg.dtype, p[0].p, p[1].p, p[2].p, p[3].p, h.asf_w, h.asf_b, asf_scratch, fused->p, N, p[0].h, p[0].w, r.stream));
    return OCRVI_OK;
}

// the caller's (N,1,H,W) fp32 output maps; all but `binary` are optional
struct DetMaps { float *binary = nullptr, *thresh = nullptr, *tbin = nullptr, *blog = nullptr, *tlog = nullptr; };

// ---- DB head (head.py:32-48): both branches' 3x3 convs as one 256->128 conv, both deconv1 as one grouped pixel-shuffle GEMM
static int det_head(const ocrvi_det& h, Runner& r, const Tensor& fused, int H, int W, const DetMaps& m) {
    const int N = fused.n;
    Tensor hc = r.alloc(N, fused.h, fused.w, 128);
    OCRVI_TRY(conv(r, h.head_conv, fused, hc, conv_opts(1, 1, ACT_RELU)));
    // deconv1 (+BN+ReLU) and deconv2 (64 -> 1) of both branches in ONE GEMM: the 1.26 GB deconv1 activation is never materialised.
    // Planning counts both logit maps whatever the caller passes: the size does not depend on which outputs a forward asks for.
    const size_t map_elems = (size_t)N * H * W;
    float* bl = m.blog && !r.dry() ? m.blog : (float*)r.arena.alloc(map_elems * 4);
    float* tl = m.tlog && !r.dry() ? m.tlog : (float*)r.arena.alloc(map_elems * 4);
    ConvOpts o;
    o.store_mode = ST_DB_TAIL; o.out2 = tl; o.offs = h.dc2_wb;
    OCRVI_TRY(conv(r, h.head_dc1, hc, wrap(bl, N, H, W, 1, true), o));
    if (!r.dry()) OCRVI_TRY(k_db_maps(bl, tl, h.cfg.k, m.binary, m.thresh, m.tbin, map_elems, r.stream));
    return OCRVI_OK;
}

// ---- DB head, binarise branch only (head.py:34; the page loop reads preds['binary'] and nothing else, pipeline2.py:318): the head of
// ocrvi_det_forward_binary.  Both layers are VIEWS of the weights the two-branch head is packed into, not a second pack: fold_det puts the
// binarise branch's 64 output channels first, so the first 64 rows (and biases) of head_conv are its 3x3 conv, and group 0 of head_dc1 is
// its deconv1.  Same packed bits and same f16x2 layer scale as the five-map path, hence the same binary map.
static int det_head_binary(const ocrvi_det& h, Runner& r, const Tensor& fused, int H, int W, float* binary) {
    ConvLayer hconv = h.head_conv, hdc = h.head_dc1;
    hconv.N_g = hconv.Np = 64;
    hdc.groups = 1;
    Tensor hc1 = r.alloc(fused.n, fused.h, fused.w, 64);
    OCRVI_TRY(conv(r, hconv, fused, hc1, conv_opts(1, 1, ACT_RELU)));
    // deconv1 (+BN+ReLU), deconv2 (64 -> 1) and the sigmoid in ONE GEMM: neither the deconv1 activation nor a logit map is written
    ConvOpts o;
    o.store_mode = ST_DB_BIN; o.offs = h.dc2_wb;
    return conv(r, hdc, hc1, wrap(binary, fused.n, H, W, 1, true), o);
}

// Backbone, FPN and ASF are the same launches with either head.
static int det_run(ocrvi_det* h, Runner& r, const float* x, int N, int H, int W, const DetMaps& m, bool binary_head) {
    Tensor cur, fused;
    OCRVI_TRY(det_stem(*h, r, x, N, H, W, &cur));
    for (int li = 0; li < 4; ++li) {
        OCRVI_TRY(det_layer(*h, r, li, &cur));
        h->tap_c[li] = cur;
    }
    OCRVI_TRY(det_neck(*h, r, h->tap_c, &fused));
    h->tap_fused = fused;
    return binary_head ? det_head_binary(*h, r, fused, H, W, m.binary) : det_head(*h, r, fused, H, W, m);
}

static int det_plan(const char* what, const ocrvi_det* h, int N, int H, int W, bool binary_head, size_t* bytes) {
    return plan_workspace(what, h, bytes, [&] { return check_det_shape(h, N, H, W); },
                          [&](Runner& r) { return det_run(const_cast<ocrvi_det*>(h), r, nullptr, N, H, W, DetMaps{}, binary_head); });
}
static int det_forward(const char* what, ocrvi_det* h, const float* x, int N, int H, int W, const DetMaps& m, bool binary_head, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return run_forward(what, h, x && m.binary && workspace, "x, binary and workspace are required", workspace, workspace_bytes, stream,
                       [&] { return check_det_shape(h, N, H, W); }, [&](Runner& r) { return det_run(h, r, x, N, H, W, m, binary_head); });
}

extern "C" int ocrvi_det_workspace_bytes(const ocrvi_det* h, int N, int H, int W, size_t* bytes) {
    return det_plan("det_workspace_bytes", h, N, H, W, false, bytes);
}

extern "C" int ocrvi_det_forward(ocrvi_det* h, const float* x, int N, int H, int W, float* binary, float* thresh, float* thresh_binary,
                                 float* bin_logits, float* thresh_logits, void* workspace, size_t workspace_bytes, void* stream) {
    DetMaps m;
    m.binary = binary; m.thresh = thresh; m.tbin = thresh_binary; m.blog = bin_logits; m.tlog = thresh_logits;
    return det_forward("det_forward", h, x, N, H, W, m, false, workspace, workspace_bytes, stream);
}

extern "C" int ocrvi_det_binary_workspace_bytes(const ocrvi_det* h, int N, int H, int W, size_t* bytes) {
    return det_plan("det_binary_workspace_bytes", h, N, H, W, true, bytes);
}

extern "C" int ocrvi_det_forward_binary(ocrvi_det* h, const float* x, int N, int H, int W, float* binary, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    DetMaps m;
    m.binary = binary;
    return det_forward("det_forward_binary", h, x, N, H, W, m, true, workspace, workspace_bytes, stream);
}

extern "C" int ocrvi_det_status(const ocrvi_det* h) {
    OCRVI_CHECK(h, OCRVI_EINVAL, "det_status: null handle");
    return h->range.status("det");
}

extern "C" int ocrvi_det_debug_features(ocrvi_det* h, int N, int H, int W, float* c2, float* c3, float* c4, float* c5, float* fused,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_TRY(check_det_shape(h, N, H, W));
    OCRVI_CHECK(h->tap_fused.p, OCRVI_EINVAL, "det_debug_features: no forward has run");
    DeviceGuard dg(h->device);
    OCRVI_HIP(dg.err);
    (void)workspace; (void)workspace_bytes;
    float* outs[4] = {c2, c3, c4, c5};
    for (int i = 0; i < 4; ++i) {
        const Tensor& t = h->tap_c[i];
        if (outs[i]) OCRVI_TRY(k_nhwc_to_nchw_f32(h->cfg.dtype, t.p, outs[i], t.n, t.h, t.w, t.c, t.c, 0, (hipStream_t)stream));
    }
    const Tensor& f = h->tap_fused;
    if (fused) OCRVI_TRY(k_nhwc_to_nchw_f32(h->cfg.dtype, f.p, fused, f.n, f.h, f.w, f.c, f.c, 0, (hipStream_t)stream));
    return OCRVI_OK;
}
