// Pillow's Image.resize with a filter (ImagingResample, Resample.c) for 8-bit images: the coefficient tables of one axis and the rule on
// the host.  Host-only unit (hg_resample.cpp, built by g++ with contraction off): nothing here may need a HIP header.  The device path
// (hg_resample.hip) uploads these tables and runs the two integer passes.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/higsfa.h"

namespace hg {

// The tables of one axis: output pixel xx reads `bounds[2 xx + 1]` source pixels from `bounds[2 xx]` on, weighted by
// k[xx * ksize + x] / 2^22 (int32, Pillow's PRECISION_BITS = 32 - 8 - 2).  Entries of a row past its count are 0.
struct ResampleAxis {
    int in = 0, out = 0, filter = 0, ksize = 0;
    std::vector<int32_t> bounds, k;
    size_t bytes() const { return (bounds.size() + k.size()) * sizeof(int32_t); }
};

// nullptr, or why the call is refused (sizes <= 0, an unknown code or NEAREST, tables beyond HG_RESAMPLE_MAX_TABLE_BYTES)
const char* resample_axis(int in, int out, int filter, ResampleAxis& ax);

// What every resize entry refuses before it does anything (the device entry too): nullptr, or why.
const char* resize_check(int filter, const void* src, int format, int h, int w, int64_t ld_bytes, int out_format, const void* dst, int out_h, int out_w,
                         int64_t dst_ld_bytes);

// Image.resize's exception for very tall images (h > 100 w and the height shrinks): the vertical pass runs first, at full width
bool resize_vertical_first(int h, int w, int out_h);

// hg_frame_resize_host (include/higsfa.h)
const char* frame_resize_host(int filter, const void* src, int format, int h, int w, int64_t ld_bytes, int out_format, void* dst, int out_h, int out_w,
                              int64_t dst_ld_bytes);

}  // namespace hg
