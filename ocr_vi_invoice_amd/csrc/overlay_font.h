// The stroke font of the overlay's region numbers (include/ocrvi.h, "Result overlay"): seven strokes per digit cell, integer endpoints
// relative to the digit's origin (its bottom-left corner, y grows downwards).  Pure data: ocrvi_overlay_segments turns it into segments,
// the kernel never sees it, so another font replaces this table and nothing else.  tests/overlay_ref.py carries its own copy.
#pragma once
#include <stdint.h>

namespace ocrvi {

constexpr int OVERLAY_DIGIT_ADVANCE = 10;   // digit k of a label has its origin at (text_pos.x + 10 k, text_pos.y)
constexpr int OVERLAY_STROKES = 7;
// stroke s = (from.x, from.y, to.x, to.y); s = 0..6 are the strokes A..G, emitted in this order
constexpr int8_t OVERLAY_STROKE[OVERLAY_STROKES][4] = {
    {0, -10, 6, -10},   // A  top
    {6, -10, 6, -5},    // B  upper right
    {6, -5, 6, 0},      // C  lower right
    {0, 0, 6, 0},       // D  bottom
    {0, -5, 0, 0},      // E  lower left
    {0, -10, 0, -5},    // F  upper left
    {0, -5, 6, -5},     // G  middle
};
// bit s of OVERLAY_DIGIT[k]: stroke s belongs to digit k   (0 ABCDEF, 1 BC, 2 ABDEG, 3 ABCDG, 4 BCFG, 5 ACDFG, 6 ACDEFG, 7 ABC, 8 all, 9 ABCDFG)
constexpr uint8_t OVERLAY_DIGIT[10] = {0x3f, 0x06, 0x5b, 0x4f, 0x66, 0x6d, 0x7d, 0x07, 0x7f, 0x6f};

}  // namespace ocrvi
