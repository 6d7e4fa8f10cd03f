// What the document finder (docfind.hip) shares with the skew estimate (skew.hip): the bounds of the working image, the page-table lookup
// and the grey stage -- the area-averaged luminance at work_h rows (include/ocrvi.h, "Document finder", `grey`).
#pragma once
#include "common.h"

namespace ocrvi {

constexpr int DOC_MAX_SIDE = 16384;      // page sides: a box of the downscale then sums to less than 2^31
constexpr int DOC_MIN_WW = 8, DOC_MAX_WW = 8192, DOC_MIN_WORK_H = 8, DOC_MAX_WORK_H = 512;

// Where a kernel's pages come from: a page table in device memory (read when the kernel runs), or, table == nullptr, one image given
// directly (the per-stage entries): ptr / h / w its pixels and size, ww its working width.
struct Pages {
    const int64_t* table;
    const uint8_t* ptr;
    int h, w, ww;
};
struct Geom {
    const uint8_t* ptr;
    int H, W, ww;
};

__host__ __device__ inline int working_width(int H, int W, int work_h) {
    const double ratio = (double)H / (double)work_h;       // scanner.py:85-86: ratio = height / 500.0, int(width / ratio)
    const double v = (double)W / ratio;
    return v >= 1e9 ? 1000000000 : (int)v;
}

// false: the page is not processed (an invalid table entry, a side above DOC_MAX_SIDE, a working width outside [8, ww_cap])
__device__ inline bool page_geom(const Pages& p, int page, int work_h, int ww_cap, Geom& g) {
    if (!p.table) {
        g = Geom{p.ptr, p.h, p.w, p.ww};
        return true;
    }
    const int64_t* e = p.table + (size_t)page * OCRVI_PAGE_ENTRY;
    const int64_t a = e[0], h = e[1], w = e[2];
    if (a == 0 || h <= 0 || w <= 0 || h > DOC_MAX_SIDE || w > DOC_MAX_SIDE) return false;
    const int ww = working_width((int)h, (int)w, work_h);
    if (ww < DOC_MIN_WW || ww > ww_cap) return false;
    g = Geom{(const uint8_t*)(uintptr_t)a, (int)h, (int)w, ww};
    return true;
}

// docfind.hip.  check_work: device >= 0, work_h and ww within the bounds above.  launch_grey: page i's grey image, row-major [work_h][its
// own ww], at out + i * stride; a page that is not processed leaves its plane untouched.
int check_work(const char* what, int device, int work_h, int ww);
int launch_grey(const Pages& p, int n, int work_h, int ww_cap, uint8_t* out, size_t stride, hipStream_t st);

}  // namespace ocrvi
