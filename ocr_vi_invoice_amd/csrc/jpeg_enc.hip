// Baseline JPEG encode (include/ocrvi.h, "JPEG encode"): the host entries (quantisation tables, header, sizes, table entry) and the six
// device kernels behind ocrvi_jpeg_encode_pages --
//   jpeg_fdct_kernel     pixels -> colour conversion, chroma down-sampling, edge replication, 8 x 8 slow-integer forward DCT out of an LDS
//                        tile, quantisation -> zigzag coefficients, absolute DC values and the AC bit count of every block
//   jpeg_bits_kernel     DC differences (dummy blocks resolved), bits per block, exclusive prefix sum -> every block's bit offset
//   jpeg_pack_kernel     a wave per block: one Huffman symbol per lane, a prefix sum of their lengths, OR into an LDS stage, words out
//   jpeg_ffcount_kernel, jpeg_ffscan_kernel, jpeg_stuff_kernel   FF bytes per 4096-byte segment, their prefix sum, the scatter that puts
//                        00 after every FF
// The host encodes no Huffman code and computes no DCT.  Every result is integer arithmetic; the only atomics are integer ORs on zeroed
// words, so a page's bytes are the same on every run.
#include <string.h>

#include <algorithm>

#include "common.h"

namespace ocrvi {
namespace {

constexpr int EE = OCRVI_JPEG_ENC_ENTRY;
constexpr int TP = 72;                  // words per block of the LDS tile, as in jpeg.hip: the eight blocks of a wave start 8 banks apart
constexpr int BLOCK_BITS = 1660;        // the most bits one block adds to the scan (include/ocrvi.h derives it)
constexpr int BLOCK_BYTES = 208;
constexpr int SEG = 4096;               // bytes of one stuffing segment: 256 threads x 16
#ifndef OCRVI_JPEG_ENC_FDCT_GRID         // workgroups per page of jpeg_fdct_kernel and jpeg_pack_kernel (overridden only to measure)
#define OCRVI_JPEG_ENC_FDCT_GRID 256
#endif
#ifndef OCRVI_JPEG_ENC_PACK_GRID
#define OCRVI_JPEG_ENC_PACK_GRID 256
#endif
constexpr int STAGE = 56;               // words of a wave's packing stage: (31 + BLOCK_BITS + 31) / 32 = 53, rounded up

#define OCRVI_ZIGZAG                                                                                                                        \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, \
        43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
constexpr uint8_t kZigzag[64] = {OCRVI_ZIGZAG};      // zigzag position -> natural (row * 8 + column) index

// Annex K.1
constexpr uint8_t kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: the number of codes of each length 1..16, then the symbols in code order.
struct HuffSpec {
    uint8_t bits[16];
    int n;
    uint8_t vals[162];
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// What the kernels look up: entry = (code length << 16) | code, by symbol (Annex C); 0 for a symbol the table lacks.
struct EncTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t zigzag_inv[64];             // natural index -> zigzag position
};
constexpr void fill_codes(const HuffSpec& s, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}
constexpr EncTables make_tables() {
    EncTables t = {};
    fill_codes(kDcLuma, t.dc[0]);
    fill_codes(kDcChroma, t.dc[1]);
    fill_codes(kAcLuma, t.ac[0]);
    fill_codes(kAcChroma, t.ac[1]);
    for (int i = 0; i < 64; ++i) t.zigzag_inv[kZigzag[i]] = (uint8_t)i;
    return t;
}
__constant__ const EncTables kTabs = make_tables();

__host__ __device__ inline unsigned long long a16(unsigned long long v) { return (v + 15ull) & ~15ull; }

// Byte offsets of a page's regions inside its workspace (include/ocrvi.h states them); o[8] = the page's workspace bytes.
__host__ __device__ inline void enc_layout(long long nb, unsigned long long* o) {
    const unsigned long long n = (unsigned long long)nb;
    o[0] = 0;                                                   // coef     int16 [nb][64]
    o[1] = 128ull * n;                                          // dcabs    int16 [nb]
    o[2] = o[1] + a16(2ull * n);                                // dcdiff   int16 [nb]
    o[3] = o[2] + a16(2ull * n);                                // bits     uint32 [nb]
    o[4] = o[3] + a16(4ull * n);                                // bitoff   uint64 [nb + 1]
    o[5] = o[4] + a16(8ull * (n + 1));                          // packed   the scan before stuffing
    const unsigned long long packed = a16((unsigned long long)BLOCK_BYTES * n) + 16;
    o[6] = o[5] + packed;                                       // seg      uint32 [packed / SEG + 1]
    o[7] = o[6] + a16(4ull * (packed / SEG + 1));               // info     uint64 [2]: the scan's bytes before stuffing
    o[8] = (o[7] + 16 + 255ull) & ~255ull;
}

__host__ __device__ inline long long enc_blocks(long long W, long long H, int nc, int hs) {
    const long long mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * hs - 1) / (8 * hs);
    return mx * my * (nc == 1 ? 1 : hs * hs + 2);
}

struct EncGeom {
    const uint8_t* src;
    long long stride;
    int W, H, nc, hs, mcus_x, bw, bh, bpm;      // bw x bh: the real luma blocks; bpm: blocks per MCU
    long long nblocks;
    const uint16_t* quant;                      // [2][64], natural order
    int16_t *coef, *dcabs, *dcdiff;
    uint32_t *bits, *packed, *seg;
    unsigned long long *bitoff, *info;
    uint8_t* out;
    unsigned long long cap, packed_words;
};

// Decodes and validates table entry `e`; false (the page is skipped, nothing of it is dereferenced) when a field is out of range or a
// region does not fit.
__device__ __forceinline__ bool enc_geom(const int64_t* e, const uint8_t* src_base, uint8_t* out_base, uint8_t* ws, unsigned long long ws_bytes, EncGeom& g) {
    const long long stride = e[1], W = e[2], H = e[3], nc = e[4], hs = e[5], cap = e[7], woff = e[8];
    if (W < 1 || W > 65500 || H < 1 || H > 65500 || (nc != 1 && nc != 3) || (hs != 1 && hs != 2) || (nc == 1 && hs != 1)) return false;
    if (stride < W * nc || woff < 0 || (woff & 255) || cap < 0) return false;
    const long long nb = enc_blocks(W, H, (int)nc, (int)hs);
    unsigned long long o[9];
    enc_layout(nb, o);
    if ((unsigned long long)woff > ws_bytes || o[8] > ws_bytes - (unsigned long long)woff) return false;
    if ((unsigned long long)cap < 2ull * BLOCK_BYTES * (unsigned long long)nb + 16) return false;
    g.src = src_base + e[0];
    g.stride = stride;
    g.W = (int)W; g.H = (int)H; g.nc = (int)nc; g.hs = (int)hs;
    g.mcus_x = (int)((W + 8 * hs - 1) / (8 * hs));
    g.bw = (int)((W + 7) / 8); g.bh = (int)((H + 7) / 8);
    g.bpm = nc == 1 ? 1 : (int)(hs * hs + 2);
    g.nblocks = nb;
    g.quant = (const uint16_t*)(e + 16);
    uint8_t* p = ws + woff;
    g.coef = (int16_t*)(p + o[0]); g.dcabs = (int16_t*)(p + o[1]); g.dcdiff = (int16_t*)(p + o[2]);
    g.bits = (uint32_t*)(p + o[3]); g.bitoff = (unsigned long long*)(p + o[4]); g.packed = (uint32_t*)(p + o[5]);
    g.seg = (uint32_t*)(p + o[6]); g.info = (unsigned long long*)(p + o[7]);
    g.out = out_base + e[6];
    g.cap = (unsigned long long)cap;
    g.packed_words = (o[6] - o[5]) >> 2;
    return true;
}

// Block d of the scan -> its component, its block coordinates inside that component's plane and whether it is a dummy block (a luma
// block of the last MCU column or row that lies beyond the image).
__device__ __forceinline__ void enc_place(const EncGeom& g, long long d, int& comp, int& bx, int& by, bool& dummy) {
    dummy = false;
    if (g.bpm == 1) {
        comp = 0; bx = (int)(d % g.mcus_x); by = (int)(d / g.mcus_x);
        return;
    }
    const long long mcu = d / g.bpm;
    const int r = (int)(d - mcu * g.bpm), nl = g.bpm - 2;
    const int mx = (int)(mcu % g.mcus_x), my = (int)(mcu / g.mcus_x);
    if (r < nl) {
        comp = 0; bx = mx * g.hs + (r % g.hs); by = my * g.hs + (r / g.hs);
        dummy = bx >= g.bw || by >= g.bh;
    } else {
        comp = r - nl + 1; bx = mx; by = my;
    }
}

// The DC value block d codes: its own, or for a dummy block that of the block coded just before it in the same MCU (a chain that ends
// at the MCU's first block, which is never a dummy).
__device__ __forceinline__ int enc_dc(const EncGeom& g, long long d) {
    int comp, bx, by;
    bool dummy;
    enc_place(g, d, comp, bx, by, dummy);
    while (dummy) enc_place(g, --d, comp, bx, by, dummy);
    return g.dcabs[d];
}

// The block of d's component coded before it, -1 for the first.
__device__ __forceinline__ long long enc_prev(const EncGeom& g, long long d) {
    if (g.bpm == 1) return d - 1;
    const long long mcu = d / g.bpm;
    const int r = (int)(d - mcu * g.bpm), nl = g.bpm - 2;
    if (r < nl) return r > 0 ? d - 1 : (mcu > 0 ? d - g.bpm + nl - 1 : -1);
    return mcu > 0 ? d - g.bpm : -1;
}

// One pass of the slow-integer forward DCT (include/ocrvi.h).  FIRST: along a row, outputs scaled by 4; else down a column.
template <bool FIRST> __device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8]) {
    constexpr int SH = FIRST ? 11 : 15, R = 1 << (SH - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        o[0] = (t10 + t11) * 4; o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2; o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + R) >> SH;
    o[6] = (z1 - t12 * 15137 + R) >> SH;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + R) >> SH;
    o[5] = (a5 + z2 + z4 + R) >> SH;
    o[3] = (a6 + z2 + z3 + R) >> SH;
    o[1] = (a7 + z1 + z4 + R) >> SH;
}

__device__ __forceinline__ int rgb_y(const uint8_t* p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16; }
__device__ __forceinline__ int rgb_c(const uint8_t* p, int comp) {
    return comp == 1 ? (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + 8388608 + 32767) >> 16
                     : (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + 8388608 + 32767) >> 16;
}

// The AC symbol a lane codes: lane k holds coefficient k of the block in zigzag order, `nz` is the ballot of the non-zero ones.  A
// non-zero coefficient carries the ZRLs of the run before it, its (run, size) code and its low bits -- at most 3 x 11 + 16 + 10 = 59
// bits; lane 63 carries the EOB when coefficient 63 is zero.  val is right-aligned, n its bits.
__device__ __forceinline__ void ac_symbol(int v, int lane, unsigned long long nz, const uint32_t* ac, unsigned long long& val, int& n) {
    val = 0; n = 0;
    if (lane >= 1 && v != 0) {
        const unsigned long long below = (nz | 1ull) & ((1ull << lane) - 1ull);
        const int run = lane - (63 - __clzll((long long)below)) - 1;
        const int size = 32 - __clz(abs(v));                                    // 1..10: |v| <= 1023
        const uint32_t e = ac[((run & 15) << 4) | size];
        val = ((unsigned long long)(e & 0xffffu) << size) | (unsigned)((v > 0 ? v : v - 1) & ((1 << size) - 1));
        n = (int)(e >> 16) + size;
        const uint32_t z = ac[0xF0];
        for (int i = run >> 4; i > 0; --i) {
            val |= (unsigned long long)(z & 0xffffu) << n;
            n += (int)(z >> 16);
        }
    } else if (lane == 63 && v == 0) {
        val = ac[0] & 0xffffu; n = (int)(ac[0] >> 16);
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ __forceinline__ unsigned wave_scan(unsigned v, int lane) {      // inclusive
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned u = __shfl_up(v, s);
        if (lane >= s) v += u;
    }
    return v;
}

__device__ __forceinline__ void load_ac_tables(uint32_t (*s_ac)[256]) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_ac[i >> 8][i & 255] = kTabs.ac[i >> 8][i & 255];
}

// A wave owns eight consecutive blocks of the scan: lane = block * 8 + row for the load and pass 1, block * 8 + column for pass 2.
// grid (x, page); the workgroups of a page stride over its groups of 4 x 8 blocks, every wave of a workgroup making the same number of
// trips (the barriers are uniform).
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const uint8_t* __restrict__ src_base, const int64_t* __restrict__ table, uint8_t* __restrict__ ws,
                                                        unsigned long long ws_bytes) {
    __shared__ __attribute__((aligned(16))) int tile[4][8 * TP];
    __shared__ uint32_t s_ac[2][256];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, src_base, nullptr, ws, ws_bytes, g)) return;    // uniform over the workgroup
    load_ac_tables(s_ac);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane >> 3, j = lane & 7;
    int* t = tile[wave];
    const long long ngroups = (g.nblocks + 7) >> 3;
    const int ch = (g.H + 1) >> 1;
    for (long long g0 = (long long)blockIdx.x * 4; g0 < ngroups; g0 += (long long)gridDim.x * 4) {
        const long long grp = g0 + wave, d0 = grp * 8;
        const int nb = grp < ngroups ? (int)min(8ll, g.nblocks - d0) : 0;
        const long long d = d0 + blk;
        int comp = 0, bx = 0, by = 0;
        bool dummy = false;
        int s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a[8];
        if (blk < nb) enc_place(g, d, comp, bx, by, dummy);
        if (blk < nb && !dummy) {
            if (comp == 0 || g.hs == 1) {
                const uint8_t* row = g.src + (long long)min(by * 8 + j, g.H - 1) * g.stride;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint8_t* p = row + (long long)min(bx * 8 + k, g.W - 1) * g.nc;
                    s[k] = (g.nc == 1 ? (int)p[0] : (comp == 0 ? rgb_y(p) : rgb_c(p, comp))) - 128;
                }
            } else {
                const int cy = min(by * 8 + j, ch - 1);
                const uint8_t *r0 = g.src + (long long)(2 * cy) * g.stride, *r1 = g.src + (long long)min(2 * cy + 1, g.H - 1) * g.stride;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int cx = bx * 8 + k;
                    const long long x0 = 3ll * min(2 * cx, g.W - 1), x1 = 3ll * min(2 * cx + 1, g.W - 1);
                    s[k] = ((rgb_c(r0 + x0, comp) + rgb_c(r0 + x1, comp) + rgb_c(r1 + x0, comp) + rgb_c(r1 + x1, comp) + 1 + (k & 1)) >> 2) - 128;
                }
            }
        }
        fdct8<true>(s, a);                                     // pass 1: along the row this lane holds
        *(int4*)&t[blk * TP + j * 8] = make_int4(a[0], a[1], a[2], a[3]);
        *(int4*)&t[blk * TP + j * 8 + 4] = make_int4(a[4], a[5], a[6], a[7]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) s[r] = t[blk * TP + r * 8 + j];   // now lane = block * 8 + column
        fdct8<false>(s, a);                                    // pass 2: down the column
        const uint16_t* q = g.quant + (comp ? 64 : 0);
        int zpos[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int dq = 8 * max(1, (int)q[r * 8 + j]);
            const int m = (abs(a[r]) + (dq >> 1)) / dq;
            zpos[r] = kTabs.zigzag_inv[r * 8 + j];
            a[r] = a[r] < 0 ? -m : m;
            if (r + j > 0) a[r] = max(-1023, min(1023, a[r]));   // never reached from 8-bit samples: the AC magnitude stays below 2^10
        }
        __syncthreads();                                       // every lane has read its column
#pragma unroll
        for (int r = 0; r < 8; ++r) t[blk * TP + zpos[r]] = a[r];
        __syncthreads();
        if (blk < nb) {
            const int4 lo = *(const int4*)&t[blk * TP + j * 8], hi = *(const int4*)&t[blk * TP + j * 8 + 4];
            *(uint4*)(g.coef + d * 64 + j * 8) = make_uint4((lo.x & 0xffff) | ((unsigned)lo.y << 16), (lo.z & 0xffff) | ((unsigned)lo.w << 16),
                                                             (hi.x & 0xffff) | ((unsigned)hi.y << 16), (hi.z & 0xffff) | ((unsigned)hi.w << 16));
            if (j == 0 && !dummy) g.dcabs[d] = (int16_t)lo.x;
        }
        for (int b = 0; b < nb; ++b) {                         // the AC bits of each block: lane = zigzag position
            const int v = t[b * TP + lane];
            const unsigned long long nz = __ballot(lane >= 1 && v != 0);
            const int r = g.bpm == 1 ? 0 : (int)((d0 + b) % g.bpm);
            unsigned long long val;
            int n;
            ac_symbol(v, lane, nz, s_ac[r >= g.bpm - 2 && g.bpm > 1 ? 1 : 0], val, n);
            n = wave_sum(n);
            if (lane == 0) g.bits[d0 + b] = (unsigned)n;
        }
        __syncthreads();                                       // the tile is written again next trip
    }
}

// One workgroup per page walks the blocks in chunks of 1024: the DC difference of every block, its DC bits added to its AC bits, and
// the exclusive prefix sum of the totals.  It also zeroes every word of `packed` in which a block starts or the scan ends (the only
// words jpeg_pack_kernel ORs into), sets the 1-bits that pad the last byte and stores the scan's byte count.
__global__ __launch_bounds__(1024) void jpeg_bits_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned long long carry;
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, nullptr, nullptr, ws, ws_bytes, g)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < g.nblocks; c0 += 1024) {
        const long long d = c0 + threadIdx.x;
        unsigned bits = 0;
        if (d < g.nblocks) {
            const long long p = enc_prev(g, d);
            const int diff = max(-2047, min(2047, enc_dc(g, d) - (p >= 0 ? enc_dc(g, p) : 0)));
            const int cat = 32 - __clz(abs(diff));             // __clz(0) = 32
            const int r = (int)(d % g.bpm);
            bits = g.bits[d] + (kTabs.dc[g.bpm > 1 && r >= g.bpm - 2 ? 1 : 0][cat] >> 16) + cat;
            g.dcdiff[d] = (int16_t)diff;
            g.bits[d] = bits;
        }
        const unsigned inc = wave_scan(bits, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        const unsigned long long off = carry + before + (inc - bits);
        if (d < g.nblocks) {
            g.bitoff[d] = off;
            g.packed[off >> 5] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long total = carry;
        g.bitoff[g.nblocks] = total;
        const int pad = (int)((0 - total) & 7), rel = (int)(total & 31);
        // the word the scan ends in: zeroed above (before the last barrier) if the last block starts in it, else here
        if ((g.bitoff[g.nblocks - 1] >> 5) != (total >> 5)) g.packed[total >> 5] = 0;
        if (pad) atomicOr(&g.packed[total >> 5], __builtin_bswap32(((1u << pad) - 1u) << (32 - rel - pad)));
        g.info[0] = (total + 7) >> 3;
    }
}

// A wave per block and trip.  Lane 0 codes the DC difference, lane k >= 1 the symbol of coefficient k (ac_symbol); an exclusive prefix
// sum of the lengths places each in the wave's LDS stage (big-endian words, ORed: lanes share words), and the stage goes out word by word
// -- the word a block starts in and the word the next block starts in, which neighbours share, by atomic OR into words jpeg_bits_kernel
// zeroed, the others stored.
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes) {
    __shared__ uint32_t stage[4][STAGE];
    __shared__ uint32_t s_ac[2][256];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, nullptr, nullptr, ws, ws_bytes, g)) return;
    load_ac_tables(s_ac);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* st = stage[wave];
    for (long long d0 = (long long)blockIdx.x * 4; d0 < g.nblocks; d0 += (long long)gridDim.x * 4) {
        const long long d = d0 + wave;
        const bool have = d < g.nblocks;
        if (lane < STAGE) st[lane] = 0;
        __syncthreads();                                       // (also orders the table load before its first use)
        unsigned long long off = 0;
        unsigned total = 0;
        if (have) {
            const int v = g.coef[d * 64 + lane];
            const unsigned long long nz = __ballot(lane >= 1 && v != 0);
            const int tab = g.bpm > 1 && (int)(d % g.bpm) >= g.bpm - 2 ? 1 : 0;
            unsigned long long val;
            int n;
            ac_symbol(v, lane, nz, s_ac[tab], val, n);
            if (lane == 0) {
                const int diff = g.dcdiff[d];
                const int cat = 32 - __clz(abs(diff));
                const uint32_t e = kTabs.dc[tab][cat];
                val = ((unsigned long long)(e & 0xffffu) << cat) | (unsigned)((diff > 0 ? diff : diff - 1) & ((1 << cat) - 1));
                n = (int)(e >> 16) + cat;
            }
            const unsigned inc = wave_scan((unsigned)n, lane);
            total = __shfl(inc, 63);
            off = g.bitoff[d];
            if (n > 0 && total <= (unsigned)BLOCK_BITS) {
                const unsigned rel = (unsigned)(off & 31) + inc - (unsigned)n;
                const unsigned w = rel >> 5, sh = rel & 31;
                const unsigned long long x = val << (64 - n);  // left-aligned
                const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
                const uint32_t w0 = hi >> sh, w1 = sh ? (hi << (32 - sh)) | (lo >> sh) : lo, w2 = sh ? lo << (32 - sh) : 0u;
                if (w0) atomicOr(&st[w], w0);
                if (w1) atomicOr(&st[w + 1], w1);
                if (w2) atomicOr(&st[w + 2], w2);
            }
        }
        __syncthreads();
        if (have && total <= (unsigned)BLOCK_BITS) {
            const int nw = (int)(((unsigned)(off & 31) + total + 31) >> 5);
            if (lane < nw && (off >> 5) + lane < g.packed_words) {
                uint32_t* dst = g.packed + (off >> 5) + lane;
                const uint32_t word = __builtin_bswap32(st[lane]);
                // (a last word the block fills to its end is its own: nobody zeroed it, so it is stored)
                if (lane == 0 || (lane == nw - 1 && ((off + total) & 31) != 0)) {
                    if (word) atomicOr(dst, word);
                } else {
                    *dst = word;
                }
            }
        }
        __syncthreads();                                       // the stage is zeroed again next trip
    }
}

__device__ __forceinline__ int ff_count16(const uint4& v, long long first, unsigned long long n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int c = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c += ((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == 0xffu && (unsigned long long)(first + i) < n ? 1 : 0;
    return c;
}

// FF bytes of every 4096-byte segment of the scan; a thread reads 16 bytes.
__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes) {
    __shared__ int wsum[4];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, nullptr, nullptr, ws, ws_bytes, g)) return;
    const unsigned long long n = g.info[0];
    const long long nseg = (long long)((n + SEG - 1) / SEG);
    for (long long s = blockIdx.x; s < nseg; s += gridDim.x) {
        const long long first = s * SEG + threadIdx.x * 16;
        int c = 0;
        if ((unsigned long long)first < n) c = ff_count16(*(const uint4*)((const uint8_t*)g.packed + first), first, n);
        c = wave_sum(c);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) g.seg[s] = (uint32_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        __syncthreads();
    }
}

// Exclusive prefix sum of the segment counts, in place; the page's stuffed length.  One workgroup per page; a skipped page gets length 0.
__global__ __launch_bounds__(1024) void jpeg_ffscan_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                          int64_t* __restrict__ lengths) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned long long carry;
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, nullptr, nullptr, ws, ws_bytes, g)) {
        if (threadIdx.x == 0) lengths[blockIdx.y] = 0;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long n = g.info[0];
    const long long nseg = (long long)((n + SEG - 1) / SEG);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < nseg; c0 += 1024) {
        const long long s = c0 + threadIdx.x;
        const unsigned c = s < nseg ? g.seg[s] : 0u;
        const unsigned inc = wave_scan(c, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        // (a page's FF bytes stay below 2^32 only for scans below 4 GiB; the segment offsets are 32-bit, so larger scans are refused on the host)
        if (s < nseg) g.seg[s] = (uint32_t)(carry + before + (inc - c));
        __syncthreads();
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) lengths[blockIdx.y] = (int64_t)(n + carry);
}

// The scatter: byte i of segment s goes to i + the FF bytes before it, each FF followed by 00.
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                         uint8_t* __restrict__ out_base) {
    __shared__ unsigned wsum[4];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EE, nullptr, out_base, ws, ws_bytes, g)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long n = g.info[0];
    const long long nseg = (long long)((n + SEG - 1) / SEG);
    for (long long s = blockIdx.x; s < nseg; s += gridDim.x) {
        const long long first = s * SEG + threadIdx.x * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        int c = 0;
        if ((unsigned long long)first < n) {
            v = *(const uint4*)((const uint8_t*)g.packed + first);
            c = ff_count16(v, first, n);
        }
        const unsigned inc = wave_scan((unsigned)c, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        unsigned long long pos = (unsigned long long)first + g.seg[s] + before + (inc - (unsigned)c);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if ((unsigned long long)(first + i) < n) {
                const uint8_t b = (uint8_t)(w4[i >> 2] >> (8 * (i & 3)));
                if (pos < g.cap) g.out[pos] = b;
                ++pos;
                if (b == 0xff) {
                    if (pos < g.cap) g.out[pos] = 0;
                    ++pos;
                }
            }
        }
        __syncthreads();
    }
}

int check_geometry(const char* who, int width, int height, int components, int subsampling) {
    OCRVI_CHECK(width >= 1 && width <= 65500 && height >= 1 && height <= 65500, OCRVI_EINVAL, "%s: sides %d x %d outside 1..65500", who, height, width);
    OCRVI_CHECK(components == 1 || components == 3, OCRVI_EINVAL, "%s: %d components (1 = grey or 3 = RGB)", who, components);
    OCRVI_CHECK(subsampling == 1 || subsampling == 2, OCRVI_EINVAL, "%s: luma sampling factor %d (2 = 4:2:0 or 1 = 4:4:4)", who, subsampling);
    return OCRVI_OK;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma) {
    OCRVI_CHECK(luma && chroma, OCRVI_EINVAL, "jpeg_quant_tables: null argument");
    OCRVI_CHECK(quality >= 1 && quality <= 100, OCRVI_EINVAL, "jpeg_quant_tables: quality %d outside 1..100", quality);
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        luma[i] = (uint16_t)std::max(1, std::min(255, (kStdLuma[i] * s + 50) / 100));
        chroma[i] = (uint16_t)std::max(1, std::min(255, (kStdChroma[i] * s + 50) / 100));
    }
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_encode_header(int width, int height, int components, int subsampling, int quality, void* out, size_t cap, size_t* used) {
    OCRVI_CHECK(out && used, OCRVI_EINVAL, "jpeg_encode_header: null argument");
    *used = 0;
    OCRVI_TRY(check_geometry("jpeg_encode_header", width, height, components, components == 1 ? 1 : subsampling));
    uint16_t qt[2][64];
    OCRVI_TRY(ocrvi_jpeg_quant_tables(quality, qt[0], qt[1]));
    uint8_t buf[OCRVI_JPEG_HEADER_MAX];
    size_t n = 0;
    auto put = [&](int v) { buf[n++] = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    put16(0xFFD8);
    put16(0xFFE0); put16(16);
    for (char c : {'J', 'F', 'I', 'F', '\0'}) put(c);
    put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
    const int ntab = components == 1 ? 1 : 2;
    for (int t = 0; t < ntab; ++t) {
        put16(0xFFDB); put16(67); put(t);
        for (int i = 0; i < 64; ++i) put(qt[t][kZigzag[i]]);
    }
    put16(0xFFC0); put16(8 + 3 * components); put(8); put16(height); put16(width); put(components);
    for (int c = 0; c < components; ++c) {
        put(c + 1); put(c == 0 && components == 3 && subsampling == 2 ? 0x22 : 0x11); put(c ? 1 : 0);
    }
    const HuffSpec* specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 2 * ntab; ++t) {
        put16(0xFFC4); put16(19 + specs[t]->n); put(ids[t]);
        for (int i = 0; i < 16; ++i) put(specs[t]->bits[i]);
        for (int i = 0; i < specs[t]->n; ++i) put(specs[t]->vals[i]);
    }
    put16(0xFFDA); put16(6 + 2 * components); put(components);
    for (int c = 0; c < components; ++c) { put(c + 1); put(c ? 0x11 : 0x00); }
    put(0); put(63); put(0);
    OCRVI_CHECK(n <= cap, OCRVI_ENOMEM, "jpeg_encode_header: %zu bytes do not fit cap = %zu", n, cap);
    memcpy(out, buf, n);
    *used = n;
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_encode_sizes(int width, int height, int components, int subsampling, int64_t* blocks, uint64_t* workspace_bytes,
                                       uint64_t* scan_capacity, uint64_t* offsets) {
    OCRVI_TRY(check_geometry("jpeg_encode_sizes", width, height, components, components == 1 ? 1 : subsampling));
    const long long nb = enc_blocks(width, height, components, components == 1 ? 1 : subsampling);
    unsigned long long o[9];
    enc_layout(nb, o);
    // the stuffing kernels keep 32-bit segment offsets
    OCRVI_CHECK((unsigned long long)BLOCK_BYTES * nb < 0xffffffffull, OCRVI_EINVAL, "jpeg_encode_sizes: %d x %d has %lld blocks, above the %llu one page may have",
                height, width, nb, 0xffffffffull / BLOCK_BYTES);
    if (blocks) *blocks = nb;
    if (workspace_bytes) *workspace_bytes = o[8];
    if (scan_capacity) *scan_capacity = 2ull * BLOCK_BYTES * (unsigned long long)nb + 16;
    if (offsets)
        for (int i = 0; i < 8; ++i) offsets[i] = o[i];
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_encode_table_entry(int width, int height, int components, int subsampling, int quality, int64_t src_offset, int64_t src_stride,
                                             int64_t out_offset, int64_t out_capacity, int64_t workspace_offset, int64_t* entry) {
    OCRVI_CHECK(entry, OCRVI_EINVAL, "jpeg_encode_table_entry: null argument");
    const int hs = components == 1 ? 1 : subsampling;
    uint64_t cap = 0;
    OCRVI_TRY(ocrvi_jpeg_encode_sizes(width, height, components, hs, nullptr, nullptr, &cap, nullptr));
    OCRVI_CHECK(src_stride >= (int64_t)width * components, OCRVI_EINVAL, "jpeg_encode_table_entry: row stride %lld is below the %lld bytes of a row",
                (long long)src_stride, (long long)width * components);
    OCRVI_CHECK(workspace_offset >= 0 && workspace_offset % 256 == 0, OCRVI_EINVAL, "jpeg_encode_table_entry: the workspace offset must be a multiple of 256");
    OCRVI_CHECK(out_capacity >= 0 && (uint64_t)out_capacity >= cap, OCRVI_EINVAL, "jpeg_encode_table_entry: capacity %lld is below the scan capacity %llu",
                (long long)out_capacity, (unsigned long long)cap);
    memset(entry, 0, sizeof(int64_t) * EE);
    OCRVI_TRY(ocrvi_jpeg_quant_tables(quality, (uint16_t*)(entry + 16), (uint16_t*)(entry + 16) + 64));
    entry[0] = src_offset; entry[1] = src_stride; entry[2] = width; entry[3] = height; entry[4] = components; entry[5] = hs;
    entry[6] = out_offset; entry[7] = out_capacity; entry[8] = workspace_offset; entry[9] = quality;
    return OCRVI_OK;
}

extern "C" int ocrvi_jpeg_encode_pages(int device, const void* src_base, const int64_t* table_dev, int n_pages, void* out_base, int64_t* lengths_dev,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(src_base && table_dev && out_base && lengths_dev && workspace && n_pages > 0 && n_pages <= 65535, OCRVI_EINVAL,
                "jpeg_encode_pages: bad argument (1 <= n_pages <= 65535)");
    OCRVI_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)lengths_dev & 7) == 0, OCRVI_EINVAL,
                "jpeg_encode_pages: the workspace must be 16-byte, table and lengths 8-byte aligned");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    const unsigned long long wb = workspace_bytes;
    // the page sizes live in device memory: a fixed number of workgroups per page strides over whatever the table holds when the kernels run
    {
        ProfScope ps("jpeg_fdct", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(OCRVI_JPEG_ENC_FDCT_GRID, n_pages), dim3(256), 0, st, (const uint8_t*)src_base, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_bits", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_bits_kernel, dim3(1, n_pages), dim3(1024), 0, st, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_pack", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3(OCRVI_JPEG_ENC_PACK_GRID, n_pages), dim3(256), 0, st, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_ffcount", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_ffcount_kernel, dim3(64, n_pages), dim3(256), 0, st, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_ffscan", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_ffscan_kernel, dim3(1, n_pages), dim3(1024), 0, st, table_dev, ws, wb, lengths_dev);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("jpeg_stuff", 0.0, 0.0, st);
        hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(64, n_pages), dim3(256), 0, st, table_dev, ws, wb, (uint8_t*)out_base);
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
