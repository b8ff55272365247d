// Pose-normalised face crops (include/higsfa.h, "normalize_image"): the per-face geometry and the whole pixel rule on the host.
// Host-only unit (hg_normalize.cpp, built by g++ with contraction off): nothing here may need a HIP header.  The device path
// (hg_normalize.hip) reads the same geoms and shares the checks.
#pragma once
#include <cstdint>

#include "../../include/higsfa.h"

namespace hg {

// At most this many staged pixels per face unless staging is forced: the taps of the final cut, 16 per output pixel
inline int64_t normalize_stage_limit(int out_w, int out_h) { return (int64_t)16 * out_w * out_h; }

// hg_normalize_geometry_host: nullptr, or why the call is refused
const char* normalize_geometry_host(const double* eyes, int64_t n, int frame_w, int frame_h, const hg_norm_consts* consts, hg_norm_geom* geoms_out);

// What both pixel entries refuse before they do anything: nullptr, or why
const char* normalize_check(const void* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                            const void* out, int64_t ldo);

// hg_normalize_faces_host
const char* normalize_faces_host(const uint8_t* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                                 uint8_t* out, int64_t ldo);

}  // namespace hg
