// Colour frame formats (include/higsfa.h, HG_FRAME_*) and PIL's "L" conversion, shared by the device kernels (hg_extract.hip) and the
// host entry (hg_hostpack.cpp, built by g++ without HIP: nothing here may need a HIP header).
#pragma once
#include <cstdint>

#include "../../include/higsfa.h"

#if defined(__HIPCC__)
#define HG_HOST_DEVICE __host__ __device__
#else
#define HG_HOST_DEVICE
#endif

namespace hg {

// bytes per pixel; 0: not a format
HG_HOST_DEVICE inline int frame_bpp(int format) {
    switch (format) {
        case HG_FRAME_L: return 1;
        case HG_FRAME_RGB:
        case HG_FRAME_BGR: return 3;
        case HG_FRAME_RGBA:
        case HG_FRAME_BGRA: return 4;
        default: return 0;
    }
}

// PIL's rgb2l (Convert.c, L24): integer, per pixel, the same for RGB, RGBA and RGBX
HG_HOST_DEVICE inline uint8_t rgb_to_gray(uint32_t r, uint32_t g, uint32_t b) {
    return (uint8_t)((r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16);
}

}  // namespace hg
