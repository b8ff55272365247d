// Pose-normalised face crops (include/higsfa.h, "normalize_image"): the per-face geometry and the whole pixel rule on the host.
// Host-only unit (hg_normalize.cpp, built by g++ with contraction off): nothing here may need a HIP header.  The device path
// (hg_normalize.hip) reads the same geoms and shares the checks.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/higsfa.h"

namespace hg {

// At most this many staged pixels per face unless staging is forced: the taps of the final cut, 16 per output pixel
inline int64_t normalize_stage_limit(int out_w, int out_h) { return (int64_t)16 * out_w * out_h; }

// hg_normalize_geometry_host: nullptr, or why the call is refused
const char* normalize_geometry_host(const double* eyes, int64_t n, int frame_w, int frame_h, const hg_norm_consts* consts, hg_norm_geom* geoms_out);

// What both pixel entries refuse before they do anything: nullptr, or why
const char* normalize_check(const void* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                            const void* out, int64_t ldo);

// The same for the faces of a STACK of same-size frames (hg_patcher_normalize_frames_device, hg_estimator_estimate_frames_device): what
// normalize_check refuses, n_frames outside 1 .. HG_MAX_STACK_FRAMES, a frame_stride below (frame_h - 1) ld + frame_w, a null face_frame
// with n > 0.  Reads the geoms (host memory) and nothing behind frames / face_frame / out: an index outside the stack is no error.
// normalize_stack_check is the part about the stack and the faces alone (the estimator has no caller's images).
const char* normalize_stack_check(const void* frames, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms,
                                  const int32_t* face_frame, int64_t n);
const char* normalize_frames_check(const void* frames, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms,
                                   const int32_t* face_frame, int64_t n, int out_w, int out_h, const void* out, int64_t ldo);

// The same for the faces of a LIST of frames of different sizes (hg_patcher_normalize_frame_list_device,
// hg_estimator_estimate_frame_list_device): "" or why the call is refused, naming the frame where one frame is the reason.  n < 0, n_frames
// outside 1 .. HG_MAX_STACK_FRAMES, a null frames, any frame hg::list_frame_refusal (hg_frame_list.hpp, bpp = 1) refuses or that is larger
// than 2^24 per side, a bad output size or ldo, a null geoms / face_frame / out with n > 0, and a geom that was not built for the size of its
// face's OWN frame.  The geom of a face whose index lies outside the list belongs to no frame and is not looked at: such a face is no
// error.  Reads the descriptors and the geoms (host memory) and nothing behind a frame pointer or out.  normalize_list_check is the part
// about the list and the faces alone (the estimator has no caller's images).
std::string normalize_list_check(const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* face_frame, int64_t n);
std::string normalize_frame_list_check(const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* face_frame, int64_t n, int out_w,
                                       int out_h, const void* out, int64_t ldo);

// hg_normalize_faces_host
const char* normalize_faces_host(const uint8_t* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                                 uint8_t* out, int64_t ldo);

}  // namespace hg
