// PNG decode (include/ocrvi.h, "PNG decode"): the C ABI of the host half (png_parse.h: chunks, CRC, inflate) and the device kernel behind
// ocrvi_png_decode_pages -- png_unfilter_kernel: the page's filtered scanlines -> row filters undone -> bits unpacked, palette looked up,
// alpha dropped, 16 -> 8 bit -> interleaved RGB in the destination.
//
// Sub, Average and Paeth are recurrences along a row, Up, Average and Paeth need the row above: the parallelism is a skewed wavefront.
// One workgroup owns a page and walks it in bands of BR rows, thread = row.  At step s thread t reconstructs chunk s - t of its row (CB
// bytes: the least common multiple of every bytes-per-pixel 1 2 3 4 6 8, so a chunk holds whole pixels and the left / above-left bytes of
// its first pixel are the tail of the previous chunk, kept in registers).  The chunk of the row above was finished one step earlier and
// comes down through a double-buffered LDS slot; one barrier per step.  The raw bytes of the next step are loaded before this step's
// arithmetic.  The chunks finished in a step are converted and stored at once, out of their slots and by all threads together (four pixels
// an item): the rows that are active in a step are few when rows are short, and a bilevel chunk holds 192 pixels.  The last row of a band
// goes to the page's line in the workspace as well, where thread 0 of the next band finds its row above.  No workgroup waits for another.
#include <string.h>

#include "common.h"
#include "png_parse.h"

namespace ocrvi {
namespace {

constexpr int PE = OCRVI_PNG_ENTRY;
constexpr int BR = png::kBandRows;       // rows of a band = threads of the workgroup
constexpr int CB = png::kChunkBytes;     // bytes of a chunk
constexpr int CWORDS = CB / 4;
constexpr int SP = 7;                    // words between the slots of neighbouring rows: odd, so ds_write_b32 / ds_read_b32 of word k by lane = row
                                         // fall on 32 different banks in each 32-lane half (6 would put rows r and r + 16 on one bank)
constexpr int PALW = 256;                // words of the palette in LDS, ahead of the slots

struct PngGeom {
    const uint8_t* pal;                  // 256 x (R, G, B, 0), colour type 3 only
    const uint8_t* rows;                 // H x (1 + row_bytes)
    int W, H, depth, colour, bpp, bits_pp, chunks;
    unsigned row_bytes;
    uint8_t* dst;
    long long stride;
    uint32_t* line;                      // chunks x CWORDS words, pages of more than one band only
};

// Decodes and validates table entry `e`; false (the page is skipped, nothing of it is dereferenced) when a field is out of range or the
// fields contradict each other.
__device__ __forceinline__ bool png_geom(const int64_t* e, const uint8_t* streams, uint8_t* dst_base, uint8_t* ws, unsigned long long ws_bytes,
                                         PngGeom& g) {
    const long long soff = e[0], sbytes = e[1], W = e[2], H = e[3], depth = e[4], colour = e[5], npal = e[6], doff = e[7], stride = e[8], woff = e[9];
    if (soff < 0 || (soff & 3) || W < 1 || W > png::kMaxSide || H < 1 || H > png::kMaxSide) return false;
    int ch;
    switch (colour) {
        case 0: if (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16) return false; ch = 1; break;
        case 3: if (depth != 1 && depth != 2 && depth != 4 && depth != 8) return false; ch = 1; break;
        case 2: if (depth != 8 && depth != 16) return false; ch = 3; break;
        case 4: if (depth != 8 && depth != 16) return false; ch = 2; break;
        case 6: if (depth != 8 && depth != 16) return false; ch = 4; break;
        default: return false;
    }
    if (npal < 0 || npal > 256 || (colour == 3 && npal < 1)) return false;
    const long long rb = (W * ch * depth + 7) >> 3;
    const long long palb = colour == 3 ? (long long)png::kPaletteBytes : 0;
    if (sbytes != palb + H * (1 + rb) || stride < 3 * W) return false;
    g.W = (int)W; g.H = (int)H; g.depth = (int)depth; g.colour = (int)colour;
    g.bits_pp = ch * (int)depth;
    g.bpp = g.bits_pp >= 8 ? g.bits_pp >> 3 : 1;
    g.row_bytes = (unsigned)rb;
    g.chunks = (int)((rb + CB - 1) / CB);
    g.line = nullptr;
    if (H > BR) {                        // the line between bands
        const unsigned long long need = ((unsigned long long)g.chunks * CB + 255) / 256 * 256;
        if (!ws || woff < 0 || (woff & 3) || (unsigned long long)woff > ws_bytes || need > ws_bytes - (unsigned long long)woff) return false;
        g.line = (uint32_t*)(ws + woff);
    }
    g.pal = streams + soff;
    g.rows = streams + soff + palb;
    g.dst = dst_base + doff;
    g.stride = stride;
    return true;
}

// The bytes [0, CB) of chunk j of row r, as words; a byte past the end of the page's rows is read from the last byte instead (only the
// last chunk of the last row can reach there, and what it reads beyond its row is never stored).
__device__ __forceinline__ void load_raw(const PngGeom& g, int r, int j, uint32_t (&w)[CWORDS]) {
    const unsigned long long start = (unsigned long long)r * (1ull + g.row_bytes) + 1ull + (unsigned long long)j * CB;
    const unsigned long long total = (unsigned long long)g.H * (1ull + g.row_bytes);
    const unsigned lim = (unsigned)min((unsigned long long)(CB - 1), total - 1 - start);
    const uint8_t* p = g.rows + start;
#pragma unroll
    for (int k = 0; k < CWORDS; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) v |= (uint32_t)p[min((unsigned)(4 * k + i), lim)] << (8 * i);
        w[k] = v;
    }
}

template <int BPP>
__device__ __forceinline__ void png_page(const PngGeom& g, uint32_t* lds) {
    const int t = threadIdx.x;
    uint32_t* palw = lds;
    uint32_t* slots = lds + PALW;
    const uint8_t* slot_bytes = (const uint8_t*)slots;
    const bool words = (((uintptr_t)g.dst | (uintptr_t)g.stride) & 3) == 0;
    const int bands = (g.H + BR - 1) / BR;
    const int ppc = (CB * 8) / g.bits_pp;              // pixels of a whole chunk
    const int gpr = (ppc & 3) == 0 ? ppc >> 2 : (ppc + 6) >> 2;   // conversion items of a chunk: its groups of four pixels, split at multiples of 4
    const int gstep = (g.colour & 2) && g.colour != 3 ? g.depth >> 3 : 0;   // bytes from a pixel's red sample to its green one (0: grey)
    const int vmask = (1 << g.depth) - 1;
    const int scale = g.depth == 1 ? 255 : g.depth == 2 ? 85 : g.depth == 4 ? 17 : 1;

    for (int band = 0; band < bands; ++band) {
        const int rows_in = min(BR, g.H - band * BR);
        const bool row_on = t < rows_in;
        const int r = band * BR + min(t, rows_in - 1);
        const int nsteps = g.chunks + rows_in - 1;
        int ft = g.rows[(unsigned long long)r * (1ull + g.row_bytes)];
        if (ft > 4) ft = 0;                            // (the host refuses such files; see ocrvi.h)
        const bool from_line = t == 0 && band > 0, to_line = t == rows_in - 1 && band + 1 < bands;
        int lt[BPP], at[BPP];                          // the tails of the previous chunk: this row's (left) and the row above's (above-left)
#pragma unroll
        for (int i = 0; i < BPP; ++i) { lt[i] = 0; at[i] = 0; }
        uint32_t nxt[CWORDS], nxt_above[CWORDS];
#pragma unroll
        for (int k = 0; k < CWORDS; ++k) { nxt[k] = 0; nxt_above[k] = 0; }
        if (t == 0) {
            load_raw(g, r, 0, nxt);
            if (from_line) {
#pragma unroll
                for (int k = 0; k < CWORDS; ++k) nxt_above[k] = g.line[k];
            }
        }
        for (int s = 0; s < nsteps; ++s) {
            const int j = s - t;
            const bool on = row_on && j >= 0 && j < g.chunks;
            uint32_t raw[CWORDS], abv[CWORDS];
#pragma unroll
            for (int k = 0; k < CWORDS; ++k) { raw[k] = nxt[k]; abv[k] = nxt_above[k]; }
            if (row_on && j + 1 >= 0 && j + 1 < g.chunks) {        // the next step's bytes: nothing of the recurrence is in their way
                load_raw(g, r, j + 1, nxt);
                if (from_line) {
#pragma unroll
                    for (int k = 0; k < CWORDS; ++k) nxt_above[k] = g.line[(size_t)(j + 1) * CWORDS + k];
                }
            }
            if (on) {
                if (t > 0) {
                    const uint32_t* up = slots + ((size_t)((s - 1) & 1) * BR + (t - 1)) * SP;
#pragma unroll
                    for (int k = 0; k < CWORDS; ++k) abv[k] = up[k];
                }
                int cur[CB];
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    const int x = (raw[i >> 2] >> (8 * (i & 3))) & 255;
                    const int b = (abv[i >> 2] >> (8 * (i & 3))) & 255;
                    const int a = i >= BPP ? cur[i >= BPP ? i - BPP : 0] : lt[i < BPP ? i : 0];
                    const int c = i >= BPP ? (int)((abv[(i >= BPP ? i - BPP : 0) >> 2] >> (8 * ((i >= BPP ? i - BPP : 0) & 3))) & 255) : at[i < BPP ? i : 0];
                    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    const int p = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
                    cur[i] = (x + p) & 255;
                }
#pragma unroll
                for (int i = 0; i < BPP; ++i) {
                    lt[i] = cur[CB - BPP + i];
                    at[i] = (abv[(CB - BPP + i) >> 2] >> (8 * ((CB - BPP + i) & 3))) & 255;
                }
                uint32_t* mine = slots + ((size_t)(s & 1) * BR + t) * SP;
#pragma unroll
                for (int k = 0; k < CWORDS; ++k) {
                    const uint32_t v = (uint32_t)cur[4 * k] | ((uint32_t)cur[4 * k + 1] << 8) | ((uint32_t)cur[4 * k + 2] << 16) | ((uint32_t)cur[4 * k + 3] << 24);
                    mine[k] = v;
                    if (to_line) g.line[(size_t)j * CWORDS + k] = v;
                }
            }
            __syncthreads();
            // ---- the chunks finished in this step (rows t_lo .. t_hi, one each) are converted out of their slots by the whole workgroup:
            //      an item is up to four pixels whose first one is a multiple of 4 (three words of a word-aligned destination row).  The
            //      slots of this parity are written again two steps on, behind the next step's barrier.
            const int t_lo = max(0, s - g.chunks + 1), t_hi = min(rows_in - 1, s);
            const int items = (t_hi - t_lo + 1) * gpr;
            for (int it = t; it < items; it += BR) {
                const int rr = it / gpr, gi = it - rr * gpr;
                const int tt = t_lo + rr, jj = s - tt;
                const int px0 = jj * ppc, pend = min(px0 + ppc, g.W);
                const int A = (px0 & ~3) + 4 * gi;
                const int P = max(A, px0), n = min(A + 4, pend) - P;
                if (n <= 0) continue;
                const uint8_t* sb = slot_bytes + ((size_t)(s & 1) * BR + tt) * (SP * 4);
                uint8_t px[12];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = min(P + k, pend - 1) - px0;      // pixel of the chunk
                    int R, G, B;
                    if (g.depth < 8) {
                        const int bit = q * g.depth;
                        const int v = (sb[bit >> 3] >> (8 - g.depth - (bit & 7))) & vmask;
                        if (g.colour == 3) { const uint32_t e = palw[v]; R = e & 255; G = (e >> 8) & 255; B = (e >> 16) & 255; }
                        else R = G = B = v * scale;
                    } else {
                        const int o = q * BPP;
                        const int v = sb[o];
                        if (g.colour == 3) { const uint32_t e = palw[v]; R = e & 255; G = (e >> 8) & 255; B = (e >> 16) & 255; }
                        else { R = v; G = sb[o + gstep]; B = sb[o + 2 * gstep]; }
                    }
                    px[3 * k] = (uint8_t)R; px[3 * k + 1] = (uint8_t)G; px[3 * k + 2] = (uint8_t)B;
                }
                uint8_t* q8 = g.dst + (long long)(band * BR + tt) * g.stride + 3ll * P;
                if (words && n == 4) {
                    uint32_t* q4 = (uint32_t*)q8;
                    q4[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
                    q4[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
                    q4[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
                } else {
#pragma unroll
                    for (int b = 0; b < 12; ++b)
                        if (b < 3 * n) q8[b] = px[b];
                }
            }
        }
        __syncthreads();                                   // the band's last conversions, before the next band writes the slots
    }
}

__global__ __launch_bounds__(BR) void png_unfilter_kernel(const uint8_t* __restrict__ streams, const int64_t* __restrict__ table, uint8_t* dst_base,
                                                          uint8_t* ws, unsigned long long ws_bytes) {
    __shared__ uint32_t lds[PALW + 2 * BR * SP];
    PngGeom g;
    if (!png_geom(table + (size_t)blockIdx.x * PE, streams, dst_base, ws, ws_bytes, g)) return;    // uniform over the workgroup
    if (g.colour == 3) lds[threadIdx.x] = ((const uint32_t*)g.pal)[threadIdx.x];
    __syncthreads();
    switch (g.bpp) {
        case 1: png_page<1>(g, lds); break;
        case 2: png_page<2>(g, lds); break;
        case 3: png_page<3>(g, lds); break;
        case 4: png_page<4>(g, lds); break;
        case 6: png_page<6>(g, lds); break;
        default: png_page<8>(g, lds); break;
    }
}

void fill_info(const png::Header& h, ocrvi_png_info_t* info) {
    info->width = h.width; info->height = h.height; info->bit_depth = h.depth; info->colour_type = h.colour;
    info->channels = h.channels; info->row_bytes = (int32_t)h.row_bytes;
    info->out_height = h.height; info->out_width = h.width;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_png_info(const void* data, size_t n, ocrvi_png_info_t* info) {
    OCRVI_CHECK(info, OCRVI_EINVAL, "png_info: info is null");
    memset(info, 0, sizeof(*info));
    png::Header h;
    const int rc = png::parse_headers((const uint8_t*)data, data ? n : 0, h, false);
    if (h.have_ihdr) fill_info(h, info);
    if (rc != png::P_OK) {
        snprintf(info->reason, sizeof(info->reason), "%s", h.msg);
        set_error("%s", h.msg);
        return rc;
    }
    info->palette_entries = h.palette_entries;
    info->idat_bytes = h.idat_bytes;
    info->stream_bytes = h.stream_bytes;
    info->workspace_bytes = h.workspace_bytes;
    return OCRVI_OK;
}

extern "C" int ocrvi_png_parse(const void* data, size_t n, void* out, size_t cap, size_t* used) {
    OCRVI_CHECK(out && used, OCRVI_EINVAL, "png_parse: out and used must be given");
    *used = 0;
    png::Header h;
    int rc = png::parse_headers((const uint8_t*)data, data ? n : 0, h, true);
    if (rc == png::P_OK) rc = png::parse_stream((const uint8_t*)data, n, h, out, cap, used);
    if (rc != png::P_OK) set_error("%s", h.msg);
    return rc;
}

extern "C" int ocrvi_png_table_entry(const ocrvi_png_info_t* info, size_t used, int64_t stream_offset, int64_t dst_offset, int64_t dst_stride,
                                     int64_t workspace_offset, int64_t* entry) {
    OCRVI_CHECK(info && entry, OCRVI_EINVAL, "png_table_entry: null argument");
    OCRVI_CHECK(info->stream_bytes > 0 && used == info->stream_bytes, OCRVI_EINVAL, "png_table_entry: used = %zu is not the stream's %llu bytes", used,
                (unsigned long long)info->stream_bytes);
    OCRVI_CHECK(stream_offset >= 0 && stream_offset % 4 == 0 && workspace_offset >= 0 && workspace_offset % 4 == 0, OCRVI_EINVAL,
                "png_table_entry: the stream offset and the workspace offset must be multiples of 4");
    OCRVI_CHECK(dst_stride >= 3ll * info->out_width, OCRVI_EINVAL, "png_table_entry: row stride %lld is below the %d bytes of a row",
                (long long)dst_stride, 3 * info->out_width);
    memset(entry, 0, sizeof(int64_t) * PE);
    entry[0] = stream_offset; entry[1] = (int64_t)info->stream_bytes;
    entry[2] = info->width; entry[3] = info->height; entry[4] = info->bit_depth; entry[5] = info->colour_type;
    entry[6] = info->palette_entries;
    entry[7] = dst_offset; entry[8] = dst_stride; entry[9] = workspace_offset;
    return OCRVI_OK;
}

extern "C" int ocrvi_png_plan(const ocrvi_png_info_t* info, int* band_rows, int* chunk_bytes, int* bands, int* steps) {
    OCRVI_CHECK(info && info->height > 0 && info->row_bytes > 0, OCRVI_EINVAL, "png_plan: info of a parsed file must be given");
    png::plan(info->height, (uint64_t)info->row_bytes, band_rows, chunk_bytes, bands, steps);
    return OCRVI_OK;
}

extern "C" int ocrvi_png_decode_pages(int device, const void* streams_dev, const int64_t* table_dev, int n_pages, void* dst_base, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(streams_dev && table_dev && dst_base && n_pages > 0 && n_pages <= 65535, OCRVI_EINVAL,
                "png_decode_pages: bad argument (1 <= n_pages <= 65535)");
    OCRVI_CHECK(workspace || workspace_bytes == 0, OCRVI_EINVAL, "png_decode_pages: workspace is null with workspace_bytes = %zu", workspace_bytes);
    OCRVI_CHECK(((uintptr_t)streams_dev & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)table_dev & 7) == 0, OCRVI_EINVAL,
                "png_decode_pages: streams and workspace must be 4-byte, the table 8-byte aligned");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    // (the profiler's byte counts stay 0: the sizes are in the table, on the device; tools/png_bench.py knows them)
    {
        ProfScope ps("png_unfilter", 0.0, 0.0, (hipStream_t)stream);
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(n_pages), dim3(BR), 0, (hipStream_t)stream, (const uint8_t*)streams_dev, table_dev,
                           (uint8_t*)dst_base, (uint8_t*)workspace, (unsigned long long)workspace_bytes);
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
