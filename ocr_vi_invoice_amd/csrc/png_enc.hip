// PNG encode (include/ocrvi.h, "PNG encode"): the host entries (sizes, table entry) and the six device kernels behind
// ocrvi_png_encode_pages --
//   png_filter_kernel    a workgroup per row: the five row filters on raw bytes, libpng's cost, the choice, the filtered stream
//   png_analyse_kernel   a workgroup per deflate block: the run tokens, their histogram, the two length-limited codes (build_lengths),
//                        the code-length tokens, the bits of the block as fixed and as dynamic, its Adler partial
//   png_scan_kernel      a workgroup per page: block types and bit offsets (a stored block's padding depends on where it starts, so this
//                        walk is serial), Adler-32, the words blocks share zeroed, signature .. zlib header and the Adler bytes written
//   png_pack_kernel      a workgroup per deflate block: header and tokens ORed into an LDS stage at their bit offsets, the stage out in words
//   png_crc_kernel, png_finish_kernel   raw CRC partials of 4096-byte segments, combined by x^(8 n); CRC, IEND and the file's length
// The host builds no code and sees no histogram.  Every result is integer arithmetic; the atomics are integer adds into LDS histograms
// and integer ORs into zeroed words, so a page's bytes are the same on every run.
#include <string.h>

#include <algorithm>

#include "common.h"

namespace ocrvi {
namespace {

constexpr int EP = OCRVI_PNG_ENC_ENTRY;
constexpr int BLK = OCRVI_PNG_ENC_BLOCK;
constexpr int NT = 256;                         // threads of every workgroup here
constexpr int CHUNK = BLK / NT;                 // stream positions one thread tokenises
constexpr int HIST = 288, LENS = 320;           // words / bytes of one block's histogram / code lengths (include/ocrvi.h)
constexpr int STAGE_WORDS = BLK / 4 + 8;        // (31 + 3 + 7 + 32 + 8 BLK + 31) / 32 words, rounded up
constexpr int SEG = 4096;                       // bytes of one CRC segment: 256 threads x 16
constexpr int HEAD = 43;                        // signature + IHDR (33), IDAT length and type (8), zlib header (2)
constexpr uint32_t POLY = 0xEDB88320u;
constexpr int ADLER = 65521;
constexpr int NO_BREAK = 0x7fffffff;
#ifndef OCRVI_PNG_ENC_GRID                      // workgroups per page of the filter, analyse and pack kernels
#define OCRVI_PNG_ENC_GRID 128
#endif

// match length -> its symbol, the number of its extra bits and their value (RFC 1951, 3.2.5)
struct LenTable {
    uint16_t sym[259];
    uint8_t ebits[259], eval[259];
};
constexpr LenTable make_len_table() {
    LenTable t = {};
    const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    for (int k = 0; k < 29; ++k) {
        const int e = k < 8 || k == 28 ? 0 : (k - 4) / 4;
        for (int l = base[k]; l < base[k] + (1 << e) && l <= 258; ++l) {
            if (l == 258 && k != 28) continue;
            t.sym[l] = (uint16_t)(257 + k); t.ebits[l] = (uint8_t)e; t.eval[l] = (uint8_t)(l - base[k]);
        }
    }
    return t;
}
__constant__ const LenTable kLen = make_len_table();
__constant__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__host__ __device__ inline unsigned long long a16(unsigned long long v) { return (v + 15ull) & ~15ull; }
__host__ __device__ inline int len_extra_bits(int s) { return s < 265 || s == 285 ? 0 : (s - 261) >> 2; }
__host__ __device__ inline int fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

struct PageSizes {
    unsigned long long stream, blocks, cap, nseg;
};
__host__ __device__ inline PageSizes page_sizes(long long W, long long H, int nc) {
    PageSizes s;
    s.stream = (unsigned long long)H * (1ull + (unsigned long long)W * nc);
    s.blocks = (s.stream + BLK - 1) / BLK;
    s.cap = 33 + 12 + 2 + 5 * s.blocks + s.stream + 4 + 12;
    s.nseg = s.cap / SEG + 2;
    return s;
}

// Byte offsets of a page's regions inside its workspace (include/ocrvi.h states them); o[9] = the page's workspace bytes.
__host__ __device__ inline void enc_layout(long long H, const PageSizes& s, unsigned long long* o) {
    const unsigned long long nb = s.blocks;
    o[0] = 0;                                           // filter of every row  uint8 [H]
    o[1] = a16((unsigned long long)H);                  // filtered stream      uint8 [stream]
    o[2] = o[1] + a16(s.stream) + 16;                   // histograms           uint32 [nb][288]
    o[3] = o[2] + 4ull * HIST * nb;                     // code lengths         uint8 [nb][320]
    o[4] = o[3] + (unsigned long long)LENS * nb;        // code-length tokens   uint16 [nb][320]
    o[5] = o[4] + 2ull * LENS * nb;                     // block records        uint32 [nb][8]
    o[6] = o[5] + 32ull * nb;                           // bit offsets          uint64 [nb + 1]
    o[7] = o[6] + a16(8ull * (nb + 1));                 // CRC partials         uint32 [nseg]
    o[8] = o[7] + a16(4ull * s.nseg);                   // info                 uint64 [4]
    o[9] = (o[8] + 32 + 255ull) & ~255ull;
}

struct EncGeom {
    const uint8_t* src;
    long long stride;
    int W, H, nc, filter;
    long long rb;                                       // bytes of a raw row
    unsigned long long stream, nblocks, cap;
    uint8_t *ftype, *s, *lens, *out;
    uint32_t *hist, *rec, *seg;
    uint16_t* cltok;
    unsigned long long *bitoff, *info;
};

// Decodes and validates table entry `e`; false (the page is skipped, nothing of it is dereferenced) when a field is out of range or a
// region does not fit.
__device__ __forceinline__ bool enc_geom(const int64_t* e, const uint8_t* src_base, uint8_t* out_base, uint8_t* ws, unsigned long long ws_bytes, EncGeom& g) {
    const long long stride = e[1], W = e[2], H = e[3], nc = e[4], filter = e[5], ooff = e[6], cap = e[7], woff = e[8];
    if (W < 1 || W > 65500 || H < 1 || H > 65500 || (nc != 1 && nc != 3) || filter < 0 || filter > 5) return false;
    if (stride < W * nc || woff < 0 || (woff & 255) || cap < 0 || (ooff & 15)) return false;
    const PageSizes s = page_sizes(W, H, (int)nc);
    if (6 + 5 * s.blocks + s.stream > 0x7fffffffull || (unsigned long long)cap < s.cap) return false;
    unsigned long long o[10];
    enc_layout(H, s, o);
    if ((unsigned long long)woff > ws_bytes || o[9] > ws_bytes - (unsigned long long)woff) return false;
    g.src = src_base + e[0];
    g.stride = stride;
    g.W = (int)W; g.H = (int)H; g.nc = (int)nc; g.filter = (int)filter;
    g.rb = W * nc;
    g.stream = s.stream; g.nblocks = s.blocks; g.cap = (unsigned long long)cap;
    uint8_t* p = ws + woff;
    g.ftype = p + o[0]; g.s = p + o[1]; g.hist = (uint32_t*)(p + o[2]); g.lens = p + o[3]; g.cltok = (uint16_t*)(p + o[4]);
    g.rec = (uint32_t*)(p + o[5]); g.bitoff = (unsigned long long*)(p + o[6]); g.seg = (uint32_t*)(p + o[7]);
    g.info = (unsigned long long*)(p + o[8]);
    g.out = out_base + ooff;
    return true;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ __forceinline__ unsigned wave_xor(unsigned v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v ^= __shfl_xor(v, s);
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
// The sum of v over the workgroup's 256 threads, to every thread; `tmp` is 4 words of LDS, free again on return.
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* tmp) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned r = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int q = a + b - c, pa = abs(q - a), pb = abs(q - b), pc = abs(q - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int filtered(int ft, int x, int a, int b, int c) {
    const int p = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - p) & 255;
}
__device__ __forceinline__ unsigned cost_of(int v) { return (unsigned)(v < 128 ? v : 256 - v); }

// grid (x, page): the workgroups of a page stride over its rows.
__global__ __launch_bounds__(NT) void png_filter_kernel(const uint8_t* __restrict__ src_base, const int64_t* __restrict__ table, uint8_t* __restrict__ ws,
                                                       unsigned long long ws_bytes) {
    __shared__ unsigned tmp[4];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, src_base, nullptr, ws, ws_bytes, g)) return;    // uniform over the workgroup
    const int bpp = g.nc;
    for (int y = blockIdx.x; y < g.H; y += gridDim.x) {
        const uint8_t* cur = g.src + (long long)y * g.stride;
        const uint8_t* up = cur - g.stride;                    // read only when y > 0
        int ft = g.filter;
        if (ft == 5) {
            unsigned c[5] = {0, 0, 0, 0, 0};
            for (long long i = threadIdx.x; i < g.rb; i += NT) {
                const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0, b = y ? up[i] : 0, cc = (y && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
                for (int f = 0; f < 5; ++f) c[f] += cost_of(filtered(f, x, a, b, cc));
            }
            unsigned best = 0;
            ft = 0;
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const unsigned t = block_sum(c[f], tmp);
                if (f == 0 || t < best) { best = t; ft = f; }  // a tie keeps the lower filter number
            }
        }
        uint8_t* row = g.s + (unsigned long long)y * (1ull + (unsigned long long)g.rb);
        if (threadIdx.x == 0) {
            row[0] = (uint8_t)ft;
            g.ftype[y] = (uint8_t)ft;
        }
        for (long long i = threadIdx.x; i < g.rb; i += NT) {
            const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0, b = y ? up[i] : 0, cc = (y && i >= bpp) ? up[i - bpp] : 0;
            row[1 + i] = (uint8_t)filtered(ft, x, a, b, cc);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- code construction
struct CodeScratch {
    uint32_t cnt[HIST];
    uint32_t w[2 * HIST];
    uint16_t parent[2 * HIST], depth[2 * HIST], order[HIST];
    int nl[16];
    int m;
};

// The length-limited code of include/ocrvi.h for counts[0 .. n), n <= 288, limit <= 15: lengths to len[0 .. n).  Called by the whole
// workgroup (256 threads); counts and len are LDS.  The sort is a rank count over all threads; the tree, the repair and the dealing
// out of lengths run on one lane.
__device__ void build_lengths(const uint32_t* counts, int n, int limit, uint8_t* len, CodeScratch& sc) {
    const int tid = threadIdx.x;
    for (int s = tid; s < n; s += NT) {
        sc.cnt[s] = counts[s];
        len[s] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        int used = 0;
        for (int s = 0; s < n; ++s) used += sc.cnt[s] != 0;
        for (int s = 0; used < 2 && s < n; ++s)
            if (!sc.cnt[s]) { sc.cnt[s] = 1; ++used; }
        sc.m = used;
    }
    __syncthreads();
    for (int s = tid; s < n; s += NT) {
        const uint32_t c = sc.cnt[s];
        if (c) {
            int rank = 0;
            for (int t = 0; t < n; ++t) {
                const uint32_t d = sc.cnt[t];
                rank += d && (d < c || (d == c && t < s));
            }
            sc.order[rank] = (uint16_t)s;
            sc.w[rank] = c;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int m = sc.m;
        int li = 0, ni = m;
        for (int node = m; node < 2 * m - 1; ++node) {
            int pick[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) pick[k] = (li < m && (ni >= node || sc.w[li] <= sc.w[ni])) ? li++ : ni++;
            sc.w[node] = sc.w[pick[0]] + sc.w[pick[1]];
            sc.parent[pick[0]] = sc.parent[pick[1]] = (uint16_t)node;
        }
        sc.depth[2 * m - 2] = 0;
        for (int node = 2 * m - 3; node >= 0; --node) sc.depth[node] = (uint16_t)(sc.depth[sc.parent[node]] + 1);
        for (int k = 0; k < 16; ++k) sc.nl[k] = 0;
        for (int leaf = 0; leaf < m; ++leaf) sc.nl[min((int)sc.depth[leaf], limit)]++;
        long long total = 0;
        for (int k = 1; k <= limit; ++k) total += (long long)sc.nl[k] << (limit - k);
        while (total > (1ll << limit)) {
            sc.nl[limit]--;
            for (int k = limit - 1; k > 0; --k)
                if (sc.nl[k]) { sc.nl[k]--; sc.nl[k + 1] += 2; break; }
            --total;
        }
        int k = 0;
        for (int bits = limit; bits > 0; --bits)
            for (int c = sc.nl[bits]; c > 0 && k < m; --c) len[sc.order[k++]] = (uint8_t)bits;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------- tokens
struct BlockLds {
    __attribute__((aligned(16))) uint8_t b[BLK];
    int last_break[NT], first_break[NT];
    int eq0;
};

// Loads block k of the page's stream and finds, per thread, the breaks (positions with eq = 0) of its chunk.  n: the block's bytes.
__device__ __forceinline__ void load_block(const EncGeom& g, unsigned long long k, int n, BlockLds& L) {
    const int tid = threadIdx.x;
    const uint8_t* base = g.s + k * BLK;                       // 16-byte aligned; the region is padded by 16 bytes
    for (int v = tid; v * 16 < n; v += NT) *(uint4*)&L.b[v * 16] = *(const uint4*)(base + v * 16);
    if (tid == 0) L.eq0 = k > 0 && base[0] == base[-1];
    __syncthreads();
    const int lo = tid * CHUNK, hi = min(lo + CHUNK, n);
    int last = -1, first = NO_BREAK;
    for (int i = lo; i < hi; ++i) {
        const bool eq = i ? L.b[i] == L.b[i - 1] : L.eq0 != 0;
        if (!eq) {
            last = i;
            if (first == NO_BREAK) first = i;
        }
    }
    L.last_break[tid] = last;
    L.first_break[tid] = first;
    __syncthreads();
}

// The tokens that start in this thread's chunk, in stream order: f(position, 0) for a literal, f(position, length) for a match.
template <class F> __device__ __forceinline__ void walk_tokens(const BlockLds& L, int n, F&& f) {
    const int tid = threadIdx.x;
    const int lo = tid * CHUNK, hi = min(lo + CHUNK, n);
    if (lo >= hi) return;
    int prev = -1, next = n;
    for (int u = tid - 1; u >= 0; --u)
        if (L.last_break[u] >= 0) { prev = L.last_break[u]; break; }
    for (int u = tid + 1; u < NT; ++u)
        if (L.first_break[u] != NO_BREAK) { next = L.first_break[u]; break; }
    int i = lo, a = prev + 1;                                  // a: where the run that position i lies in starts
    while (i < hi) {
        const bool eq = i ? L.b[i] == L.b[i - 1] : L.eq0 != 0;
        if (!eq) {
            f(i, 0);
            a = ++i;
            continue;
        }
        int e = i + 1;
        while (e < hi && L.b[e] == L.b[e - 1]) ++e;
        if (e == hi) e = next;                                 // the run goes on into later chunks (next >= hi)
        const int run = e - a, full = run / 258 * 258, rem = run - full, stop = min(e, hi);
        for (int j = (i - a + 257) / 258 * 258; j < full && a + j < stop; j += 258) f(a + j, 258);
        if (rem >= 3) {
            if (a + full >= i && a + full < stop) f(a + full, rem);
        } else {
            for (int p = max(i, a + full); p < stop; ++p) f(p, 0);
        }
        i = stop;
    }
}

// grid (x, page): the workgroups of a page stride over its deflate blocks.
__global__ __launch_bounds__(NT) void png_analyse_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes) {
    __shared__ BlockLds L;
    __shared__ CodeScratch sc;
    __shared__ uint32_t s_hist[HIST], s_clhist[19];
    __shared__ uint8_t s_len[LENS];
    __shared__ uint16_t s_cltok[LENS];
    __shared__ unsigned tmp[4];
    __shared__ int s_hlit, s_ntok, s_hclen, s_clbits;
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, nullptr, nullptr, ws, ws_bytes, g)) return;
    const int tid = threadIdx.x;
    for (unsigned long long k = blockIdx.x; k < g.nblocks; k += gridDim.x) {
        const int n = (int)min((unsigned long long)BLK, g.stream - k * BLK);
        for (int s = tid; s < HIST; s += NT) s_hist[s] = 0;
        for (int s = tid; s < LENS; s += NT) { s_len[s] = 0; s_cltok[s] = 0; }
        load_block(g, k, n, L);                                // (its barriers order the zeroing above too)
        unsigned sa = 0;
        unsigned long long sb = 0;
        {
            const int lo = tid * CHUNK, hi = min(lo + CHUNK, n);
            for (int i = lo; i < hi; ++i) {
                sa += L.b[i];
                sb += (unsigned long long)(n - i) * L.b[i];
            }
        }
        walk_tokens(L, n, [&](int p, int len) {
            if (len) {
                atomicAdd(&s_hist[kLen.sym[len]], 1u);
                atomicAdd(&s_hist[286], 1u);
            } else {
                atomicAdd(&s_hist[L.b[p]], 1u);
            }
        });
        if (tid == 0) atomicAdd(&s_hist[256], 1u);
        const unsigned adler_a = block_sum(sa, tmp) % ADLER;   // (the barriers inside also complete the histogram)
        const unsigned adler_b = block_sum((unsigned)(sb % ADLER), tmp) % ADLER;
        build_lengths(s_hist, 286, 15, s_len, sc);
        if (tid == 0) {
            int hlit = 286;
            while (hlit > 257 && s_len[hlit - 1] == 0) --hlit;
            for (int s = 0; s < 19; ++s) s_clhist[s] = 0;
            // the HLIT + 2 lengths as one sequence, cut into runs of equal values
            const int total = hlit + 2;
            int i = 0, nt = 0;
            while (i < total) {
                const int v = i < hlit ? s_len[i] : 1;
                int e = i + 1;
                while (e < total && (e < hlit ? s_len[e] : 1) == v) ++e;
                int left = e - i;
                i = e;
                if (v == 0) {
                    while (left) {
                        const int c = min(left, 138);
                        if (c >= 11) { s_cltok[nt++] = (uint16_t)(18 | ((c - 11) << 8)); s_clhist[18]++; }
                        else if (c >= 3) { s_cltok[nt++] = (uint16_t)(17 | ((c - 3) << 8)); s_clhist[17]++; }
                        else for (int r = 0; r < c; ++r) { s_cltok[nt++] = 0; s_clhist[0]++; }
                        left -= c;
                    }
                } else {
                    s_cltok[nt++] = (uint16_t)v; s_clhist[v]++;
                    --left;
                    while (left >= 3) {
                        const int c = min(left, 6);
                        s_cltok[nt++] = (uint16_t)(16 | ((c - 3) << 8)); s_clhist[16]++;
                        left -= c;
                    }
                    for (; left > 0; --left) { s_cltok[nt++] = (uint16_t)v; s_clhist[v]++; }
                }
            }
            s_hlit = hlit; s_ntok = nt;
        }
        __syncthreads();
        build_lengths(s_clhist, 19, 7, s_len + HIST, sc);
        if (tid == 0) {
            int hclen = 19;
            while (hclen > 4 && s_len[HIST + kClOrder[hclen - 1]] == 0) --hclen;
            int bits = 0;
            for (int s = 0; s < 19; ++s) bits += (int)s_clhist[s] * (s_len[HIST + s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
            s_hclen = hclen; s_clbits = bits;
        }
        unsigned fb = 0, db = 0;
        for (int s = tid; s < 286; s += NT) {
            const unsigned c = s_hist[s], x = (unsigned)len_extra_bits(s);
            fb += c * (fixed_len(s) + x);
            db += c * (s_len[s] + x);
        }
        const unsigned fixed_bits = 3 + block_sum(fb, tmp) + 5 * s_hist[286];
        const unsigned dyn_body = block_sum(db, tmp);          // (its barriers publish s_hclen and s_clbits)
        for (int s = tid; s < HIST; s += NT) g.hist[k * HIST + s] = s_hist[s];
        for (int s = tid; s < LENS; s += NT) {
            g.lens[k * LENS + s] = s_len[s];
            g.cltok[k * LENS + s] = s_cltok[s];
        }
        if (tid == 0) {
            uint32_t* r = g.rec + k * 8;
            r[0] = (uint32_t)n; r[1] = fixed_bits; r[2] = 3 + 14 + 3 * s_hclen + s_clbits + dyn_body + s_hist[286];
            r[3] = (uint32_t)s_hlit; r[4] = (uint32_t)s_hclen; r[5] = (uint32_t)s_ntok; r[6] = 0; r[7] = adler_a | (adler_b << 16);
        }
        __syncthreads();                                       // the LDS is written again next trip
    }
}

__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t v) {
    crc ^= v;
#pragma unroll
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (POLY & (0u - (crc & 1u)));
    return crc;
}
// The product of two polynomials mod the CRC polynomial, reflected: bit 31 is x^0.
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        r ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return r;
}
__device__ __forceinline__ uint32_t crc_xpow8(unsigned long long n) {          // x^(8 n)
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// One workgroup per page walks the blocks in chunks of 256: lane 0 picks every block's type at its position, the others store the types
// and offsets and zero the word each block starts in (the only words png_pack_kernel ORs into, with the word the stream ends in).
__global__ __launch_bounds__(NT) void png_scan_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                     uint8_t* __restrict__ out_base) {
    __shared__ uint32_t s_n[NT], s_fixed[NT], s_dyn[NT], s_ad[NT], s_type[NT];
    __shared__ unsigned long long s_off[NT];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, nullptr, out_base, ws, ws_bytes, g)) return;
    const int tid = threadIdx.x;
    uint32_t* out32 = (uint32_t*)g.out;
    unsigned long long pos = 0;                                // lane 0's state
    uint32_t a1 = 1, a2 = 0;
    for (unsigned long long c0 = 0; c0 < g.nblocks; c0 += NT) {
        const unsigned long long k = c0 + tid;
        if (k < g.nblocks) {
            const uint32_t* r = g.rec + k * 8;
            s_n[tid] = r[0]; s_fixed[tid] = r[1]; s_dyn[tid] = r[2]; s_ad[tid] = r[7];
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = (int)min((unsigned long long)NT, g.nblocks - c0);
            for (int j = 0; j < cnt; ++j) {
                const uint32_t n = s_n[j];
                const uint32_t stored = 3 + (uint32_t)((0 - (pos + 3)) & 7) + 32 + 8 * n;
                uint32_t bits = stored, type = 0;
                if (s_fixed[j] < bits) { bits = s_fixed[j]; type = 1; }
                if (s_dyn[j] < bits) { bits = s_dyn[j]; type = 2; }
                s_type[j] = type;
                s_off[j] = pos;
                pos += bits;
                a2 = (uint32_t)((a2 + (unsigned long long)n * a1 + (s_ad[j] >> 16)) % ADLER);
                a1 = (a1 + (s_ad[j] & 0xffffu)) % ADLER;
            }
        }
        __syncthreads();
        if (k < g.nblocks) {
            g.rec[k * 8 + 6] = s_type[tid];
            g.bitoff[k] = s_off[tid];
            out32[(8ull * HEAD + s_off[tid]) >> 5] = 0;
        }
        __syncthreads();
    }
    if (tid == 0) out32[(8ull * HEAD + pos) >> 5] = 0;        // the word the stream ends in (inside the file: the Adler bytes follow)
    __syncthreads();
    if (tid == 0) {
        g.bitoff[g.nblocks] = pos;
        const unsigned long long E = (pos + 7) >> 3;           // bytes of the deflate stream
        uint8_t* o = g.out;
        const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
        for (int i = 0; i < 16; ++i) o[i] = sig[i];
        put_be32(o + 16, (uint32_t)g.W);
        put_be32(o + 20, (uint32_t)g.H);
        o[24] = 8; o[25] = g.nc == 3 ? 2 : 0; o[26] = 0; o[27] = 0; o[28] = 0;
        uint32_t crc = 0xffffffffu;
        for (int i = 12; i < 29; ++i) crc = crc_byte(crc, o[i]);
        put_be32(o + 29, ~crc);
        put_be32(o + 33, (uint32_t)(2 + E + 4));
        o[37] = 'I'; o[38] = 'D'; o[39] = 'A'; o[40] = 'T'; o[41] = 0x78; o[42] = 0x01;
        const uint32_t adler = (a2 << 16) | a1;
        put_be32(o + HEAD + E, adler);
        g.info[0] = E; g.info[1] = adler; g.info[2] = 0; g.info[3] = 63 + E;
    }
}

// val (n <= 32 bits, nothing above them) into the stage at bit `bit`, least significant bit first.
__device__ __forceinline__ void put_bits(uint32_t* stage, unsigned bit, uint32_t val, int n) {
    if (n <= 0) return;
    const unsigned w = bit >> 5, sh = bit & 31;
    if (w < (unsigned)STAGE_WORDS && (val << sh)) atomicOr(&stage[w], val << sh);
    if (sh + n > 32 && w + 1 < (unsigned)STAGE_WORDS && (val >> (32 - sh))) atomicOr(&stage[w + 1], val >> (32 - sh));
}

// Canonical codes (RFC 1951, 3.2.2) of len[0 .. n), bit-reversed, as code | length << 16; by the whole workgroup.  cnt: 17 words of LDS.
__device__ void canonical_codes(const uint8_t* len, int n, uint32_t* code, uint32_t* cnt) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        uint32_t c[16];
        for (int b = 0; b < 16; ++b) c[b] = 0;
        for (int s = 0; s < n; ++s) c[len[s]]++;
        c[0] = 0;
        uint32_t v = 0;
        cnt[0] = 0;
        for (int b = 1; b < 16; ++b) {
            v = (v + c[b - 1]) << 1;
            cnt[b] = v;                                        // the first code of length b
        }
    }
    __syncthreads();
    for (int s = tid; s < n; s += NT) {
        const int l = len[s];
        uint32_t e = 0;
        if (l) {
            uint32_t v = cnt[l];
            for (int t = 0; t < s; ++t) v += len[t] == l;
            e = (__brev(v) >> (32 - l)) | ((uint32_t)l << 16);
        }
        code[s] = e;
    }
    __syncthreads();
}

// grid (x, page): the workgroups of a page stride over its deflate blocks.  A block's bits are ORed into an LDS stage that starts at the
// word the block starts in; the stage goes out word by word -- the word the block starts in and, unless the block fills it, the word
// it ends in by atomic OR into words png_scan_kernel zeroed (neighbours share them), the others stored.
__global__ __launch_bounds__(NT) void png_pack_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                     uint8_t* __restrict__ out_base) {
    __shared__ BlockLds L;
    __shared__ uint32_t stage[STAGE_WORDS];
    __shared__ uint32_t s_code[HIST], s_clcode[19], s_cnt[17];
    __shared__ uint8_t s_len[LENS];
    __shared__ unsigned s_wsum[4];
    __shared__ unsigned s_head;
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, nullptr, out_base, ws, ws_bytes, g)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* out32 = (uint32_t*)g.out;
    const unsigned long long cap_words = g.cap >> 2;
    for (unsigned long long k = blockIdx.x; k < g.nblocks; k += gridDim.x) {
        const uint32_t* r = g.rec + k * 8;
        const int n = (int)r[0], type = (int)r[6], hlit = (int)r[3], hclen = (int)r[4], ntok = (int)r[5];
        const unsigned long long off = 8ull * HEAD + g.bitoff[k];
        const unsigned total = (unsigned)(g.bitoff[k + 1] - g.bitoff[k]), rel = (unsigned)(off & 31);
        const unsigned final_bit = k + 1 == g.nblocks ? 1u : 0u;
        const int nw = min((int)((rel + total + 31) >> 5), STAGE_WORDS);
        for (int w = tid; w < nw; w += NT) stage[w] = 0;
        load_block(g, k, n, L);
        if (type == 0) {
            const unsigned pad = (0u - (rel + 3u)) & 7u;
            if (tid == 0) {
                put_bits(stage, rel, final_bit, 3);
                put_bits(stage, rel + 3 + pad, (uint32_t)n | ((uint32_t)(n ^ 0xffff) << 16), 32);
            }
            __syncthreads();                                   // the header's last word may hold the first data bytes
            uint8_t* sb8 = (uint8_t*)stage + ((rel + 3 + pad + 32) >> 3);
            const int lo = tid * CHUNK, hi = min(lo + CHUNK, n);
            for (int i = lo; i < hi; ++i) sb8[i] = L.b[i];
        } else {
            for (int s = tid; s < LENS; s += NT) s_len[s] = type == 1 ? (s < HIST ? (uint8_t)fixed_len(s) : 0) : g.lens[k * LENS + s];
            __syncthreads();
            canonical_codes(s_len, HIST, s_code, s_cnt);
            if (type == 2) canonical_codes(s_len + HIST, 19, s_clcode, s_cnt);
            if (tid == 0) {
                unsigned b = rel;
                put_bits(stage, b, final_bit | ((unsigned)type << 1), 3); b += 3;
                if (type == 2) {
                    put_bits(stage, b, (unsigned)(hlit - 257) | (1u << 5) | ((unsigned)(hclen - 4) << 10), 14); b += 14;
                    for (int i = 0; i < hclen; ++i) { put_bits(stage, b, s_len[HIST + kClOrder[i]], 3); b += 3; }
                    const uint16_t* tok = g.cltok + k * LENS;
                    for (int i = 0; i < ntok && i < LENS; ++i) {
                        const int sym = tok[i] & 255, ev = tok[i] >> 8;
                        const uint32_t e = s_clcode[sym < 19 ? sym : 0];
                        const int cl = (int)(e >> 16), xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                        put_bits(stage, b, (e & 0xffffu) | ((uint32_t)ev << cl), cl + xb);
                        b += cl + xb;
                    }
                }
                s_head = b;
            }
            const int dist_bits = type == 1 ? 5 : 1;
            unsigned mine = 0;
            walk_tokens(L, n, [&](int p, int len) {
                mine += len ? (s_code[kLen.sym[len]] >> 16) + kLen.ebits[len] + dist_bits : s_code[L.b[p]] >> 16;
            });
            const unsigned inc = wave_scan(mine, lane);
            if (lane == 63) s_wsum[wave] = inc;
            __syncthreads();                                   // (publishes s_head too)
            unsigned before = 0, all = 0;
            for (int w = 0; w < 4; ++w) {
                before += w < wave ? s_wsum[w] : 0;
                all += s_wsum[w];
            }
            unsigned b = s_head + before + inc - mine;
            walk_tokens(L, n, [&](int p, int len) {
                if (len) {
                    const uint32_t e = s_code[kLen.sym[len]];
                    const int cl = (int)(e >> 16), xb = kLen.ebits[len];
                    put_bits(stage, b, (e & 0xffffu) | ((uint32_t)kLen.eval[len] << cl), cl + xb + dist_bits);
                    b += cl + xb + dist_bits;
                } else {
                    const uint32_t e = s_code[L.b[p]];
                    put_bits(stage, b, e & 0xffffu, (int)(e >> 16));
                    b += e >> 16;
                }
            });
            if (tid == 0) put_bits(stage, s_head + all, s_code[256] & 0xffffu, (int)(s_code[256] >> 16));
        }
        __syncthreads();
        for (int w = tid; w < nw; w += NT) {
            const unsigned long long idx = (off >> 5) + w;
            if (idx >= cap_words) continue;
            const uint32_t word = stage[w];
            if (w == 0 || (w == nw - 1 && ((off + total) & 31) != 0)) {
                if (word) atomicOr(&out32[idx], word);
            } else {
                out32[idx] = word;
            }
        }
        __syncthreads();                                       // the stage is zeroed again next trip
    }
}

// Raw CRC partials (register 0 at the start, no inversion) of the 4096-byte segments of the FILE that IDAT's type, data and Adler bytes
// touch: file bytes [37, 37 + n).  The first four bytes are inverted, which is the CRC's initial value.  A thread reads 16 bytes and
// multiplies its partial by x^(8 x the bytes after them in the segment).
__global__ __launch_bounds__(NT) void png_crc_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                    uint8_t* __restrict__ out_base) {
    __shared__ unsigned tmp[4];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, nullptr, out_base, ws, ws_bytes, g)) return;
    const unsigned long long begin = 37, end = 37 + 4 + 2 + g.info[0] + 4;
    const unsigned long long nseg = (end + SEG - 1) / SEG;
    for (unsigned long long s = blockIdx.x; s < nseg; s += gridDim.x) {
        const unsigned long long first = s * SEG + threadIdx.x * 16ull, seg_end = min((s + 1) * SEG, end);
        const unsigned long long lo = max(first, begin), hi = min(first + 16, seg_end);
        uint32_t crc = 0;
        if (lo < hi) {
            for (unsigned long long i = lo; i < hi; ++i) crc = crc_byte(crc, (uint32_t)g.out[i] ^ (i < begin + 4 ? 0xffu : 0u));
            crc = crc_mul(crc, crc_xpow8(seg_end - hi));
        }
        crc = wave_xor(crc);
        if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = crc;
        __syncthreads();
        if (threadIdx.x == 0) g.seg[s] = tmp[0] ^ tmp[1] ^ tmp[2] ^ tmp[3];
        __syncthreads();
    }
}

// One workgroup per page: the partials, each multiplied by x^(8 x the bytes after its segment), XORed and inverted; the CRC, IEND and
// the file's length.  A skipped page gets length 0.
__global__ __launch_bounds__(NT) void png_finish_kernel(const int64_t* __restrict__ table, uint8_t* __restrict__ ws, unsigned long long ws_bytes,
                                                       uint8_t* __restrict__ out_base, int64_t* __restrict__ lengths) {
    __shared__ unsigned tmp[4];
    EncGeom g;
    if (!enc_geom(table + (size_t)blockIdx.y * EP, nullptr, out_base, ws, ws_bytes, g)) {
        if (threadIdx.x == 0) lengths[blockIdx.y] = 0;
        return;
    }
    const unsigned long long E = g.info[0], end = 37 + 4 + 2 + E + 4;
    const unsigned long long nseg = (end + SEG - 1) / SEG;
    uint32_t crc = 0;
    for (unsigned long long s = threadIdx.x; s < nseg; s += NT) crc ^= crc_mul(g.seg[s], crc_xpow8(end - min((s + 1) * SEG, end)));
    crc = wave_xor(crc);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = crc;
    __syncthreads();
    if (threadIdx.x == 0) {
        crc = ~(tmp[0] ^ tmp[1] ^ tmp[2] ^ tmp[3]);
        uint8_t* o = g.out + end;
        put_be32(o, crc);
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) o[4 + i] = iend[i];
        g.info[2] = crc;
        lengths[blockIdx.y] = (int64_t)(63 + E);
    }
}

// grid (code): counts [n] -> lengths [n] through build_lengths.
__global__ __launch_bounds__(NT) void png_test_lengths_kernel(const uint32_t* __restrict__ counts, int n, int limit, uint8_t* __restrict__ lengths) {
    __shared__ CodeScratch sc;
    __shared__ uint32_t s_cnt[HIST];
    __shared__ uint8_t s_len[HIST];
    for (int s = threadIdx.x; s < n; s += NT) s_cnt[s] = counts[(size_t)blockIdx.x * n + s];
    __syncthreads();
    build_lengths(s_cnt, n, limit, s_len, sc);
    for (int s = threadIdx.x; s < n; s += NT) lengths[(size_t)blockIdx.x * n + s] = s_len[s];
}

int check_geometry(const char* who, int width, int height, int components) {
    OCRVI_CHECK(width >= 1 && width <= 65500 && height >= 1 && height <= 65500, OCRVI_EINVAL, "%s: sides %d x %d outside 1..65500", who, height, width);
    OCRVI_CHECK(components == 1 || components == 3, OCRVI_EINVAL, "%s: %d components (1 = grey or 3 = RGB)", who, components);
    const PageSizes s = page_sizes(width, height, components);
    OCRVI_CHECK(6 + 5 * s.blocks + s.stream <= 0x7fffffffull, OCRVI_EINVAL, "%s: %d x %d x %d may need an IDAT chunk of %llu bytes, above 2^31 - 1", who, height,
                width, components, 6 + 5 * s.blocks + s.stream);
    return OCRVI_OK;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_png_encode_sizes(int width, int height, int components, uint64_t* stream_bytes, int64_t* blocks, uint64_t* workspace_bytes,
                                      uint64_t* out_capacity, uint64_t* offsets) {
    OCRVI_TRY(check_geometry("png_encode_sizes", width, height, components));
    const PageSizes s = page_sizes(width, height, components);
    unsigned long long o[10];
    enc_layout(height, s, o);
    if (stream_bytes) *stream_bytes = s.stream;
    if (blocks) *blocks = (int64_t)s.blocks;
    if (workspace_bytes) *workspace_bytes = o[9];
    if (out_capacity) *out_capacity = s.cap;
    if (offsets)
        for (int i = 0; i < 9; ++i) offsets[i] = o[i];
    return OCRVI_OK;
}

extern "C" int ocrvi_png_encode_table_entry(int width, int height, int components, int filter, int64_t src_offset, int64_t src_stride, int64_t out_offset,
                                            int64_t out_capacity, int64_t workspace_offset, int64_t* entry) {
    OCRVI_CHECK(entry, OCRVI_EINVAL, "png_encode_table_entry: null argument");
    uint64_t cap = 0;
    OCRVI_TRY(ocrvi_png_encode_sizes(width, height, components, nullptr, nullptr, nullptr, &cap, nullptr));
    OCRVI_CHECK(filter >= 0 && filter <= 5, OCRVI_EINVAL, "png_encode_table_entry: filter %d (0..4 = none, sub, up, average, paeth on every row; 5 = adaptive)", filter);
    OCRVI_CHECK(src_stride >= (int64_t)width * components, OCRVI_EINVAL, "png_encode_table_entry: row stride %lld is below the %lld bytes of a row",
                (long long)src_stride, (long long)width * components);
    OCRVI_CHECK(workspace_offset >= 0 && workspace_offset % 256 == 0, OCRVI_EINVAL, "png_encode_table_entry: the workspace offset must be a multiple of 256");
    OCRVI_CHECK(out_offset % 16 == 0, OCRVI_EINVAL, "png_encode_table_entry: the output offset must be a multiple of 16");
    OCRVI_CHECK(out_capacity >= 0 && (uint64_t)out_capacity >= cap, OCRVI_EINVAL, "png_encode_table_entry: capacity %lld is below the output capacity %llu",
                (long long)out_capacity, (unsigned long long)cap);
    memset(entry, 0, sizeof(int64_t) * EP);
    entry[0] = src_offset; entry[1] = src_stride; entry[2] = width; entry[3] = height; entry[4] = components; entry[5] = filter;
    entry[6] = out_offset; entry[7] = out_capacity; entry[8] = workspace_offset;
    return OCRVI_OK;
}

extern "C" int ocrvi_png_encode_pages(int device, const void* src_base, const int64_t* table_dev, int n_pages, void* out_base, int64_t* lengths_dev,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(src_base && table_dev && out_base && lengths_dev && workspace && n_pages > 0 && n_pages <= 65535, OCRVI_EINVAL,
                "png_encode_pages: bad argument (1 <= n_pages <= 65535)");
    OCRVI_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out_base & 15) == 0 && ((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)lengths_dev & 7) == 0,
                OCRVI_EINVAL, "png_encode_pages: the workspace and the output must be 16-byte, table and lengths 8-byte aligned");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t*)workspace, *out = (uint8_t*)out_base;
    const unsigned long long wb = workspace_bytes;
    // the page sizes live in device memory: a fixed number of workgroups per page strides over whatever the table holds when the kernels run
    {
        ProfScope ps("png_filter", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_filter_kernel, dim3(OCRVI_PNG_ENC_GRID, n_pages), dim3(NT), 0, st, (const uint8_t*)src_base, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("png_analyse", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_analyse_kernel, dim3(OCRVI_PNG_ENC_GRID, n_pages), dim3(NT), 0, st, table_dev, ws, wb);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("png_scan", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_scan_kernel, dim3(1, n_pages), dim3(NT), 0, st, table_dev, ws, wb, out);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("png_pack", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_pack_kernel, dim3(OCRVI_PNG_ENC_GRID, n_pages), dim3(NT), 0, st, table_dev, ws, wb, out);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("png_crc", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_crc_kernel, dim3(64, n_pages), dim3(NT), 0, st, table_dev, ws, wb, out);
    }
    OCRVI_HIP(hipGetLastError());
    {
        ProfScope ps("png_finish", 0.0, 0.0, st);
        hipLaunchKernelGGL(png_finish_kernel, dim3(1, n_pages), dim3(NT), 0, st, table_dev, ws, wb, out, lengths_dev);
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_test_png_code_lengths(int device, const uint32_t* counts_dev, int n_codes, int n_symbols, int limit, uint8_t* lengths_dev, void* stream) {
    OCRVI_CHECK(counts_dev && lengths_dev && n_codes > 0 && n_codes <= 65535, OCRVI_EINVAL, "test_png_code_lengths: bad argument (1 <= n_codes <= 65535)");
    OCRVI_CHECK(n_symbols >= 2 && n_symbols <= 288 && limit >= 1 && limit <= 15 && n_symbols <= (1 << limit), OCRVI_EINVAL,
                "test_png_code_lengths: %d symbols at limit %d (2..288 symbols, limit 1..15, symbols <= 2^limit)", n_symbols, limit);
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    hipLaunchKernelGGL(png_test_lengths_kernel, dim3(n_codes), dim3(NT), 0, (hipStream_t)stream, counts_dev, n_symbols, limit, lengths_dev);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
