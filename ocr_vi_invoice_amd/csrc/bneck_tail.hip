// The fused ResNet-50 layer1 chain (bneck_tail.h): its translation unit and host launcher.
#include "bneck_tail.h"
namespace ocrvi {
OCRVI_RANGE_FLAG_TU()   // binds this unit's f16x2 range-flag pointer (common.h)

int launch_bneck_tail(const BneckTailParams& p, hipStream_t stream) {
    OCRVI_CHECK(p.x && p.w2 && p.wt && p.idn && p.y && p.n_img > 0 && p.H > 0 && p.W > 0, OCRVI_EINVAL, "bneck_tail: bad argument");
    OCRVI_CHECK((((uintptr_t)p.x | (uintptr_t)p.w2 | (uintptr_t)p.wt | (uintptr_t)p.idn | (uintptr_t)p.y | (uintptr_t)p.t1n) & 15) == 0, OCRVI_EINVAL,
                "bneck_tail: operands must be 16-byte aligned");
    char tag[128];
    double flops = 0, bytes = 0;
    if (prof_enabled()) {
        static const bool detail = getenv("OCRVI_PROF_DETAIL") != nullptr;
        const double M = (double)p.n_img * p.H * p.W;
        const bool c = p.t1n != nullptr;
        flops = 2.0 * M * (64.0 * 576 + 256.0 * 64 + (c ? 64.0 * 256 : 0.0));
        bytes = 4.0 * (M * (64 + 256 + 256 + (c ? 64 : 0)) + 64.0 * 576 + 256.0 * 64 + (c ? 64.0 * 256 : 0.0));
        if (detail) snprintf(tag, sizeof(tag), "bneck_tail_f16x2 M%d %s", (int)M, c ? "y+t1" : "y");
        else snprintf(tag, sizeof(tag), "bneck_tail_f16x2");
    }
    ProfScope ps(tag, flops, bytes, stream);
    return p.t1n ? launch_bneck_tail_t<true>(p, stream) : launch_bneck_tail_t<false>(p, stream);
}
}  // namespace ocrvi
