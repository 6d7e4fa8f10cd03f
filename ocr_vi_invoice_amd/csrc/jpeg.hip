// Baseline JPEG decode (include/ocrvi.h, "JPEG decode"): the C ABI of the host parser (jpeg_parse.h) and the two device kernels behind
// ocrvi_jpeg_decode_pages -- jpeg_idct_kernel (sparse records -> dequantise -> 8 x 8 slow-integer IDCT -> component planes) and
// jpeg_rgb_kernel (planes -> chroma upsampling -> YCbCr to RGB -> orientation -> interleaved RGB in the destination).
#include <string.h>

#include <algorithm>

#include "common.h"
#include "jpeg_parse.h"

namespace ocrvi {
namespace {

constexpr int JE = OCRVI_JPEG_ENTRY;
constexpr int TP = 72;          // words per block of the LDS tile: 64 + 8, so the four blocks of a 32-lane group start 8 banks apart (ds_read_b32
                                // and ds_write_b32 of one tile row by lane = block * 8 + column are conflict-free under the mod-32 bank rule)
constexpr int SAT = 16384;      // saturation of dequantised coefficients and of pass-1 results: [-SAT, SAT - 1]

struct JpegGeom {
    const uint32_t* off;        // nblocks + 1 record offsets
    const uint32_t* rec;
    const uint16_t* quant;      // [3][64], natural order
    int nblocks, W, H, nc, hs, vs, orient, mcus_x, mcus_y;
    unsigned nrec;
    size_t pitch0, plane1, plane2, pitch1;   // byte offsets of the chroma planes inside the page's workspace
    uint8_t* ws;                // the page's planes
    long long dst_off, dst_stride;
};

// Decodes and validates table entry `e`; false (the page is skipped, nothing of it is dereferenced) when a field is out of range or the
// planes do not fit the workspace.
__device__ __forceinline__ bool jpeg_geom(const int64_t* e, const uint32_t* records, uint8_t* ws, unsigned long long ws_bytes, JpegGeom& g) {
    const long long soff = e[0], nb = e[1], nr = e[2], W = e[3], H = e[4], nc = e[5], hs = e[6], vs = e[7], orient = e[8], woff = e[11];
    if (soff < 0 || (soff & 3) || W < 1 || W > 65500 || H < 1 || H > 65500 || (nc != 1 && nc != 3) || nr < 0 || nr > 0xffffffffll) return false;
    if (!((hs == 1 && vs == 1) || (nc == 3 && hs == 2 && (vs == 1 || vs == 2))) || orient < 1 || orient > 8 || woff < 0 || (woff & 7)) return false;
    g.W = (int)W; g.H = (int)H; g.nc = (int)nc; g.hs = (int)hs; g.vs = (int)vs; g.orient = (int)orient;
    g.mcus_x = (g.W + 8 * g.hs - 1) / (8 * g.hs);
    g.mcus_y = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    const long long blocks = (long long)g.mcus_x * g.mcus_y * (nc == 1 ? 1 : hs * vs + 2);
    if (nb != blocks || blocks > 0x7fffffffll) return false;
    g.nblocks = (int)blocks;
    g.nrec = (unsigned)nr;
    g.pitch0 = (size_t)g.mcus_x * g.hs * 8;
    g.pitch1 = (size_t)g.mcus_x * 8;
    g.plane1 = g.pitch0 * ((size_t)g.mcus_y * g.vs * 8);
    g.plane2 = g.plane1 + g.pitch1 * ((size_t)g.mcus_y * 8);
    const size_t total = nc == 1 ? g.plane1 : g.plane2 + (g.plane2 - g.plane1);
    if ((unsigned long long)woff > ws_bytes || total > ws_bytes - (unsigned long long)woff) return false;
    g.ws = ws + woff;
    g.off = records + (soff >> 2);
    g.rec = g.off + blocks + 1;
    g.quant = (const uint16_t*)(e + 16);
    g.dst_off = e[9];
    g.dst_stride = e[10];
    return true;
}

// One pass of the slow-integer IDCT (include/ocrvi.h).  Unsigned arithmetic: the sums wrap modulo 2^32 on the way and the result is exact
// because, with inputs inside [-SAT, SAT - 1], every output's true value is below 2^13 * 7.5 * 2^14 < 2^31.
template <int SHIFT> __device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8]) {
    typedef unsigned U;
    const U i0 = in[0], i1 = in[1], i2 = in[2], i3 = in[3], i4 = in[4], i5 = in[5], i6 = in[6], i7 = in[7];
    U z1 = (i2 + i6) * 4433u;
    const U t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const U t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    U o0 = i7, o1 = i5, o2 = i3, o3 = i1;
    z1 = o0 + o3;
    U z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const U z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u; z3 = z5 - z3 * 16069u; z4 = z5 - z4 * 3196u;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    const U r = 1u << (SHIFT - 1);
    out[0] = (int)(t10 + o3 + r) >> SHIFT; out[7] = (int)(t10 - o3 + r) >> SHIFT;
    out[1] = (int)(t11 + o2 + r) >> SHIFT; out[6] = (int)(t11 - o2 + r) >> SHIFT;
    out[2] = (int)(t12 + o1 + r) >> SHIFT; out[5] = (int)(t12 - o1 + r) >> SHIFT;
    out[3] = (int)(t13 + o0 + r) >> SHIFT; out[4] = (int)(t13 - o0 + r) >> SHIFT;
}

// Block d of the scan -> its component and its block coordinates inside that component's plane.
__device__ __forceinline__ void block_place(const JpegGeom& g, int d, int& comp, int& bx, int& by) {
    if (g.nc == 1) {
        comp = 0; bx = d % g.mcus_x; by = d / g.mcus_x;
        return;
    }
    const int nl = g.hs * g.vs, bpm = nl + 2;
    const int mcu = d / bpm, r = d - mcu * bpm;
    const int mx = mcu % g.mcus_x, my = mcu / g.mcus_x;
    if (r < nl) {
        comp = 0; bx = mx * g.hs + (r % g.hs); by = my * g.vs + (r / g.hs);
    } else {
        comp = r - nl + 1; bx = mx; by = my;
    }
}

// A wave owns eight consecutive blocks of the scan: lane = block * 8 + column.  grid (x, page); the workgroups of a page stride over its
// groups of 4 x 8 blocks, every wave of a workgroup making the same number of trips (the barriers are uniform).
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint32_t* __restrict__ records, const int64_t* __restrict__ table, uint8_t* __restrict__ ws,
                                                        unsigned long long ws_bytes) {
    __shared__ __attribute__((aligned(16))) int tile[4][8 * TP];
    JpegGeom g;
    if (!jpeg_geom(table + (size_t)blockIdx.y * JE, records, ws, ws_bytes, g)) return;    // uniform over the workgroup
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane >> 3, col = lane & 7;
    int* t = tile[wave];
    const int ngroups = (g.nblocks + 7) >> 3;
    for (int g0 = blockIdx.x * 4; g0 < ngroups; g0 += gridDim.x * 4) {
        const int grp = g0 + wave, d0 = grp * 8;
        const int nb = grp < ngroups ? min(8, g.nblocks - d0) : 0;
        for (int i = lane; i < 8 * TP; i += 64) t[i] = 0;
        __syncthreads();
        if (nb > 0) {
            unsigned o[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) o[j] = min(g.off[d0 + min(j, nb)], g.nrec);
            for (unsigned i = o[0] + lane; i < o[8]; i += 64) {
                int b = 0;
#pragma unroll
                for (int j = 1; j < 8; ++j) b += (i >= o[j]) ? 1 : 0;
                int comp, bx, by;
                block_place(g, d0 + min(b, nb - 1), comp, bx, by);
                const unsigned r = g.rec[i];
                const int pos = (r >> 16) & 63;
                const int dq = (int)(short)(r & 0xffffu) * (int)g.quant[comp * 64 + pos];     // |int16| * uint16 fits int32
                t[min(b, nb - 1) * TP + pos] = max(-SAT, min(SAT - 1, dq));
            }
        }
        __syncthreads();
        int a[8], c[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) a[r] = t[blk * TP + r * 8 + col];
        idct8<11>(a, c);                                       // pass 1: down the column
#pragma unroll
        for (int r = 0; r < 8; ++r) t[blk * TP + r * 8 + col] = max(-SAT, min(SAT - 1, c[r]));   // (the words this lane has just read)
        __syncthreads();
        const int4 lo = *(const int4*)&t[blk * TP + col * 8], hi = *(const int4*)&t[blk * TP + col * 8 + 4];   // now lane = block * 8 + row
        const int w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        idct8<18>(w, c);                                       // pass 2: along the row
        if (blk < nb) {
            unsigned px[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) px[k] = (unsigned)max(0, min(255, c[k] + 128));
            int comp, bx, by;
            block_place(g, d0 + blk, comp, bx, by);
            const size_t pitch = comp == 0 ? g.pitch0 : g.pitch1;
            uint8_t* plane = g.ws + (comp == 0 ? 0 : (comp == 1 ? g.plane1 : g.plane2));
            *(uint2*)(plane + ((size_t)by * 8 + col) * pitch + (size_t)bx * 8) =
                make_uint2(px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24), px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24));
        }
        __syncthreads();                                       // the tile is zeroed again next trip
    }
}

// One chroma sample at full resolution, from a plane of cw x ch real samples (the block padding beyond them is never read).
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, size_t pitch, int cw, int ch, int hs, int vs, int sy, int sx) {
    if (hs == 1) return p[(size_t)sy * pitch + sx];
    const int j = sx >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (size_t)sy * pitch;
        const int c = row[j];
        if (cw <= 2) return c;                                 // too narrow for the triangle filter: replicated
        if (sx & 1) return j == cw - 1 ? c : (3 * c + row[j + 1] + 2) >> 2;
        return j == 0 ? c : (3 * c + row[j - 1] + 1) >> 2;
    }
    const int i = sy >> 1;
    const uint8_t* near = p + (size_t)i * pitch;
    if (cw <= 2) return near[j];
    const int fi = (sy & 1) ? min(i + 1, ch - 1) : max(i - 1, 0);
    const uint8_t* far = p + (size_t)fi * pitch;
    const int t = 3 * near[j] + far[j];
    if (sx & 1) return j == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[j + 1] + far[j + 1] + 7) >> 4;
    return j == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[j - 1] + far[j - 1] + 8) >> 4;
}

// A thread owns four consecutive pixels of a destination row (12 bytes: three words when the row is word-aligned).
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const int64_t* __restrict__ table, const uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                       uint8_t* __restrict__ dst_base) {
    JpegGeom g;
    if (!jpeg_geom(table + (size_t)blockIdx.y * JE, nullptr, const_cast<uint8_t*>(ws), ws_bytes, g)) return;
    const int oh = g.orient >= 5 ? g.W : g.H, ow = g.orient >= 5 ? g.H : g.W;
    if (g.dst_stride < 3ll * ow) return;
    uint8_t* dst = dst_base + g.dst_off;
    const bool words = (((uintptr_t)dst | (uintptr_t)g.dst_stride) & 3) == 0;
    const int gw = (ow + 3) >> 2;
    const size_t total = (size_t)oh * gw;
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
    const uint8_t *yp = g.ws, *cbp = g.ws + g.plane1, *crp = g.ws + g.plane2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int oy = (int)(i / gw), ox0 = (int)(i - (size_t)oy * gw) * 4;
        uint8_t px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = min(ox0 + k, ow - 1);
            int sy, sx;
            switch (g.orient) {
                case 2: sy = oy; sx = g.W - 1 - ox; break;
                case 3: sy = g.H - 1 - oy; sx = g.W - 1 - ox; break;
                case 4: sy = g.H - 1 - oy; sx = ox; break;
                case 5: sy = ox; sx = oy; break;
                case 6: sy = g.H - 1 - ox; sx = oy; break;
                case 7: sy = g.H - 1 - ox; sx = g.W - 1 - oy; break;
                case 8: sy = ox; sx = g.W - 1 - oy; break;
                default: sy = oy; sx = ox; break;
            }
            const int Y = yp[(size_t)sy * g.pitch0 + sx];
            int R = Y, G = Y, B = Y;
            if (g.nc == 3) {
                const int cb = chroma_at(cbp, g.pitch1, cw, ch, g.hs, g.vs, sy, sx) - 128;
                const int cr = chroma_at(crp, g.pitch1, cw, ch, g.hs, g.vs, sy, sx) - 128;
                R = Y + ((91881 * cr + 32768) >> 16);
                G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
                B = Y + ((116130 * cb + 32768) >> 16);
            }
            px[3 * k] = (uint8_t)max(0, min(255, R));
            px[3 * k + 1] = (uint8_t)max(0, min(255, G));
            px[3 * k + 2] = (uint8_t)max(0, min(255, B));
        }
        uint8_t* q = dst + (long long)oy * g.dst_stride + 3ll * ox0;
        if (words && ox0 + 4 <= ow) {
            uint32_t* q4 = (uint32_t*)q;
            q4[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
            q4[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
            q4[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
        } else {
            const int nbytes = 3 * min(4, ow - ox0);
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < nbytes) q[b] = px[b];
        }
    }
}

void fill_info(const jpeg::Header& h, ocrvi_jpeg_info_t* info) {
    info->width = h.width; info->height = h.height; info->components = h.ncomp;
    for (int c = 0; c < 3; ++c) { info->h_samp[c] = c < h.ncomp ? h.hs[c] : 0; info->v_samp[c] = c < h.ncomp ? h.vs[c] : 0; }
    info->restart_interval = h.restart_interval;
    info->orientation = h.orientation;
    const bool swap = h.orientation >= 5;
    info->out_height = swap ? h.width : h.height;
    info->out_width = swap ? h.height : h.width;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_jpeg_info(const void* data, size_t n, ocrvi_jpeg_info_t* info) {
    OCRVI_CHECK(info, OCRVI_EINVAL, "jpeg_info: info is null");
    memset(info, 0, sizeof(*info));
    info->orientation = 1;
    jpeg::Header h;
    const int rc = jpeg::parse_headers((const uint8_t*)data, data ? n : 0, h);
    if (h.have_sof) fill_info(h, info);
    if (rc != jpeg::J_OK) {
        snprintf(info->reason, sizeof(info->reason), "%s", h.msg);
        set_error("%s", h.msg);
        return rc;
    }
    info->blocks = h.blocks;
    info->stream_bytes = jpeg::stream_bound(h, n);
    info->workspace_bytes = align_up((size_t)jpeg::plane_bytes(h), 256);
    for (int c = 0; c < h.ncomp; ++c) memcpy(info->quant[c], h.quant[h.tq[c]], sizeof(info->quant[c]));
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_parse(const void* data, size_t n, void* out, size_t cap, size_t* used) {
    OCRVI_CHECK(out && used && ((uintptr_t)out & 3) == 0, OCRVI_EINVAL, "jpeg_parse: out (4-byte aligned) and used must be given");
    *used = 0;
    jpeg::Header h;
    int rc = jpeg::parse_headers((const uint8_t*)data, data ? n : 0, h);
    if (rc == jpeg::J_OK) rc = jpeg::parse_scan((const uint8_t*)data, n, h, out, cap, used);
    if (rc != jpeg::J_OK) set_error("%s", h.msg);
    return rc;
}

extern "C" int ocrvi_jpeg_table_entry(const ocrvi_jpeg_info_t* info, size_t used, int64_t stream_offset, int64_t dst_offset, int64_t dst_stride,
                                      int64_t workspace_offset, int64_t* entry) {
    OCRVI_CHECK(info && entry, OCRVI_EINVAL, "jpeg_table_entry: null argument");
    OCRVI_CHECK(info->blocks > 0 && used % 4 == 0 && used / 4 >= (size_t)info->blocks + 1, OCRVI_EINVAL,
                "jpeg_table_entry: used = %zu does not hold the offsets of %lld blocks", used, (long long)info->blocks);
    OCRVI_CHECK(stream_offset >= 0 && stream_offset % 4 == 0 && workspace_offset >= 0 && workspace_offset % 8 == 0, OCRVI_EINVAL,
                "jpeg_table_entry: the stream offset must be a multiple of 4 and the workspace offset of 8");
    OCRVI_CHECK(dst_stride >= 3ll * info->out_width, OCRVI_EINVAL, "jpeg_table_entry: row stride %lld is below the %d bytes of a row",
                (long long)dst_stride, 3 * info->out_width);
    memset(entry, 0, sizeof(int64_t) * JE);
    entry[0] = stream_offset;
    entry[1] = info->blocks;
    entry[2] = (int64_t)(used / 4) - (info->blocks + 1);
    entry[3] = info->width; entry[4] = info->height; entry[5] = info->components;
    entry[6] = info->h_samp[0]; entry[7] = info->v_samp[0]; entry[8] = info->orientation;
    entry[9] = dst_offset; entry[10] = dst_stride; entry[11] = workspace_offset;
    memcpy(entry + 16, info->quant, sizeof(info->quant));
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_decode_pages(int device, const void* records_dev, const int64_t* table_dev, int n_pages, void* dst_base, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(records_dev && table_dev && dst_base && workspace && n_pages > 0 && n_pages <= 65535, OCRVI_EINVAL,
                "jpeg_decode_pages: bad argument (1 <= n_pages <= 65535)");
    OCRVI_CHECK(((uintptr_t)records_dev & 3) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)table_dev & 7) == 0, OCRVI_EINVAL,
                "jpeg_decode_pages: records must be 4-byte, table and workspace 8-byte aligned");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    // the page sizes live in device memory: a fixed number of workgroups per page strides over whatever the table holds when the kernels run
    // (the profiler's byte counts stay 0: the sizes are in the table, on the device; tools/jpeg_bench.py knows them)
    {
        ProfScope ps("jpeg_idct", 0.0, 0.0, (hipStream_t)stream);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(256, n_pages), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)records_dev, table_dev,
                           (uint8_t*)workspace, (unsigned long long)workspace_bytes);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_rgb", 0.0, 0.0, (hipStream_t)stream);
        hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(512, n_pages), dim3(256), 0, (hipStream_t)stream, table_dev, (const uint8_t*)workspace,
                           (unsigned long long)workspace_bytes, (uint8_t*)dst_base);
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
