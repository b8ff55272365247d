// On-device sub-image extraction: the producer of the hot call's input,
//   subimages_arr = load_network_subimages(images, ..., curr_subimage_coordinates, curr_angles, w, h, NEAREST)
//                                                        (FaceDetectUpdated.py:686; face_analysis.py:775-800)
// which the reference does per patch with PIL: Image.transform((w, h), Image.EXTENT, (x0, y0, x1, y1),
// Image.NEAREST) inside cuicuilco.image_loader.extract_subimages_rotate.  This restates PIL's
// EXTENT/NEAREST index rule (ImagingScaleAffine) exactly, including its additive accumulation of the
// source coordinate in double precision:
//     a = (x1 - x0) / w;  xo = x0 + a/2;  for x in 0..w-1: xin = xo < 0 ? -1 : (int)xo;  xo += a
// (same for y); source pixels outside the frame leave the output pixel 0.
//
// Rotated windows (delta_ang != 0; the reference passes -1 * curr_angles, face_analysis.py:782, non-zero after the first
// PAng stage).  cuicuilco's own composition is not available ([K]); the rule implemented — and tested bit for bit
// against PIL — is
//     window = frame.rotate(delta_ang, NEAREST, center = ((x0 + x1) / 2, (y0 + y1) / 2)).transform((w, h), EXTENT, box, NEAREST)
// composed per output pixel: the EXTENT tables give the pixel (xr, yr) of the ROTATED frame, and PIL's affine_fixed()
// (Geometry.c) gives that pixel's source: 16.16 fixed-point coefficients A0..A5 from the matrix Image.rotate builds
// (cos / sin of -radians(angle % 360) rounded to 15 decimals), xs = (A2 + yr A1 + xr A0) >> 16, ys likewise.  The integer
// sums are PIL's running sums in closed form.  Multiples of 180 degrees take PIL's "scaling" branch (sin rounds to 0) with
// its floating running sums.  The coefficients are computed on the device in double precision without contraction (the pragma
// below: PIL computes m2 = m0 (-cx) + m1 (-cy) + cx in Python, where a fused multiply-add would move it by an ulp); the
// one place this can differ from the host's libm is the last bit of cos / sin before the 15-decimal rounding, which
// moves a fixed-point coefficient only if it sits within 7e-11 of a rounding boundary.  Rotated frames must stay inside
// PIL's fixed-point range (|source coordinate| < 32768), otherwise the window is left 0.
//
// The reference's other filters (interpolation_formats, FaceDetectUpdated.py:125: BILINEAR, BICUBIC) are the second half of this
// file ("BILINEAR / BICUBIC windows"): PIL's generic affine transform in doubles, the same composition for rotated windows with
// the stage's filter in both steps.
//
// Colour frames (include/higsfa.h, HG_FRAME_*): PIL's integer "L" rule (hg_frame_format.hpp) in k_frame_to_gray — a whole frame — and in
// k_extent_gather instantiated on a packed-pixel source type — NEAREST, unrotated windows cut straight from the colour frame, which is
// how the cascade prescales one.
#include <hip/hip_runtime.h>

#include "hg_common.hpp"
#include "hg_frame_format.hpp"
#include "hg_frame_list.hpp"

struct hg_patcher {
    int device = -1;
    hg::DevBuf tabs, boxes, frame, out, rot, angles;
    // hg_patcher_extract_keyed_device: index tables kept per key (boxes the CALLER declares unchanged: the prescale's whole-frame box, the
    // first-stage grid of a frame size) — the table kernel then runs once, not once per frame
    struct Keyed {
        uint64_t key = 0;
        int64_t n = 0;
        int out_w = 0, out_h = 0, frame_w = 0, frame_h = 0;
        int filtered = 0;       // 1: the tables are FiltEnt (BILINEAR / BICUBIC), 0: NEAREST indices
        hg::DevBuf tabs;
    };
    hg::DevBuf ftabs, frot;     // BILINEAR / BICUBIC: coordinate tables and rotation matrices of unkeyed calls
    Keyed keyed[4];
    int keyed_next = 0;
    // a frame list (hg::patcher_extract_frame_list): the descriptor table of a call that brings its descriptors in host memory, and the
    // shared first-stage tables of the whole list — one buffer that lives for the call, kept while the list's key and shape stay
    hg::DevBuf list_desc, list_tabs;
    uint64_t list_key = 0;
    int64_t list_rows = 0;
    int list_w = 0, list_h = 0, list_filtered = 0;
    void* resample = nullptr;   // hg_patcher_resize_device: the tables and the intermediate image (hg_resample.hip owns and frees it)
    void* normalize = nullptr;  // hg_patcher_normalize_device: face records and the staged rectangles (hg_normalize.hip owns and frees it)
    ~hg_patcher() {
        hg::resample_state_free(resample);
        hg::normalize_state_free(normalize);
    }
};

namespace hg { void set_last_error(const std::string& s); }

// No contraction anywhere below: under hipcc's -ffp-contract=fast-honor-pragmas the __dadd_rn / __dmul_rn of the HIP headers are plain
// operators, so a multiply feeding an add may become one fma.  The helpers (d_add ..., hg_filter_dev.hpp) are defined under the pragma:
// each operation rounds on its own, as PIL's C doubles and Python floats do (tests/test_fp_contract.py checks the fma count).
#pragma clang fp contract(off)
namespace {
#include "hg_filter_dev.hpp"      // d_add / d_sub / d_mul / d_div, FiltEnt, filter_coord, bicubic, filter_sample (shared with hg_normalize.hip)

// Source index tables, one entry per thread.  PIL steps the source coordinate by repeated addition
// (o += a per output pixel); to land on the same pixel in every case each thread repeats that sum from the start
// of its axis — O(m) dependent adds for the last entry instead of one thread walking all m entries with a
// conversion, two compares and a store per step.
__device__ __forceinline__ int32_t extent_entry(const double* __restrict__ box, int e, int w, int h, int fw, int fh) {
    const int axis = e >= w ? 1 : 0, i = axis ? e - w : e;
    const double lo = box[axis], hi = box[2 + axis];
    const int m = axis ? h : w, lim = axis ? fh : fw;
    const double a = (hi - lo) / m;
    double o = lo + a * 0.5;
    // PIL's running sum, one addition per output pixel before this one (rounded one by one: no contraction, no reassociation);
    // eight per trip, so that the loop's compare-and-branch is not what the chain waits for (the 1562-entry table of the prescale
    // took 26.8 us with one addition per trip)
    int k = 0;
    for (; k + 8 <= i; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) o = d_add(o, a);
    }
    for (; k < i; ++k) o = d_add(o, a);
    const int v = o < 0.0 ? -1 : (int)o;
    return (v >= 0 && v < lim) ? v : -1;
}

struct RotCoef;
__device__ __forceinline__ void rot_coef_store(const double* __restrict__ boxes, const double* __restrict__ angs, int64_t b, int fw, int fh, RotCoef* out);

// angs != nullptr: the thread of a box's first table entry also computes the box's rotation coefficients (a launch of its own —
// k_rot_coefs — cost the cascade 4.8 us nine times per frame; here it runs beside the other threads' addition chains)
__global__ void k_extent_tables(const double* __restrict__ boxes, int64_t n, int w, int h, int fw, int fh, int32_t* __restrict__ tabs,
                                const double* __restrict__ angs, RotCoef* __restrict__ rot) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wh = w + h;
    if (id >= n * wh) return;
    const int64_t b = id / wh;
    const int e = (int)(id - b * wh);
    tabs[b * wh + e] = extent_entry(boxes + b * 4, e, w, h, fw, fh);
    if (angs && e == 0) rot_coef_store(boxes, angs, b, fw, fh, rot);
}

// A packed colour pixel as a source pixel type of k_extent_gather (include/higsfa.h, HG_FRAME_*): BPP bytes, alignment 1, read as
// PIL's "L" value.  Only the BPP bytes of the pixel itself are read — a 4-byte read of a 3-byte pixel would leave the frame at the
// last pixel of its last row.
template <int BPP, bool BGR>
struct ColorPx {
    uint8_t c[BPP];
};
template <typename FT>
__device__ __forceinline__ FT px_load(const FT* __restrict__ row, int x) { return row[x]; }
template <int BPP, bool BGR>
__device__ __forceinline__ uint8_t px_load(const ColorPx<BPP, BGR>* __restrict__ row, int x) {
    const uint8_t* p = row[x].c;
    if constexpr (BPP == 4) {      // the pixel's own four bytes as one load
        uint32_t q;
        __builtin_memcpy(&q, p, 4);
        return hg::rgb_to_gray((q >> (BGR ? 16 : 0)) & 0xffu, (q >> 8) & 0xffu, (q >> (BGR ? 0 : 16)) & 0xffu);
    } else {
        return hg::rgb_to_gray(p[BGR ? 2 : 0], p[1], p[BGR ? 0 : 2]);
    }
}

// Windows from a STACK of same-size frames (hg_patcher_extract_frames_device): every gather kernel below takes, as an optional LAST
// argument, one FrameSel.  Without it (the instantiations every other entry launches) a kernel is the code it was before the stack
// existed: frame_of() is then `true` and touches nothing.  With it the box's frame is looked up once per box — the box index is uniform
// per workgroup — and `frame` moves to that frame's first pixel; a box whose frame index lies outside [0, n_frames) forms NO address
// from it: it reads frame 0 through the kernels' clamped addresses and every pixel is masked to 0.
struct FrameSel {
    const int32_t* row_frame;      // per box; the box's frame is row_frame[b] / div (the cascade passes its original-window indices and n0)
    int64_t stride;                // bytes from frame f to frame f + 1
    int32_t n_frames, div;
    int64_t tab_n;                 // unrotated boxes: box b reads the tables of box b % tab_n (a grid repeated per frame); n: a table per box
};
template <typename P>
__device__ __forceinline__ bool frame_of(int64_t, P&, int64_t&) { return true; }
template <typename P>
__device__ __forceinline__ bool frame_of(int64_t b, P& frame, int64_t& tb, const FrameSel& s) {
    const int32_t r = s.row_frame[b];
    const int32_t f = r / s.div;
    const bool in_stack = r >= 0 && f < s.n_frames;
    if (in_stack) frame = (P)((const char*)frame + (int64_t)f * s.stride);
    tb = b % s.tab_n;
    return in_stack;
}

// Windows from a LIST of grey uint8 frames of different sizes (hg_patcher_extract_frame_list_device, hg_common.hpp): the third form of
// the optional last argument.  The frame geometry is no longer the kernel's arguments but a device table of one descriptor per frame,
// and per box (uniform per workgroup) frame_of() replaces the frame pointer and the table row, geo() the kernels' locals ld, fw and fh (one descriptor load, returned by value),
// by the box's frame's.  Without a list geo() returns the kernel's own argument: the other instantiations stay the code they were.  The
// kernel's own arguments are frame 0's: a box whose frame lies outside [0, n_frames) forms no address from its index, keeps frame 0's
// geometry through the kernels' clamped addresses and is masked to 0, as in the stack form.
// The frame of box b: row_frame[b] itself (win_frame == nullptr), or win_frame[row_frame[b]] where row_frame holds the cascade's
// original-window indices (the array k_cascade_init_list writes, n_windows entries).  shared_tabs: the unrotated boxes are the
// concatenated grids of the list and original window r of frame f reads table row tab_row[f] + (r - first[f]) of one call-long buffer,
// which frames of equal grids share; otherwise a table per box.
struct FrameListSel {
    const hg::FrameDesc* desc;
    const int32_t* row_frame;
    const int32_t* win_frame;
    int32_t n_frames, n_windows, shared_tabs, pad;
};
__device__ __forceinline__ int32_t list_frame_of(int64_t b, const FrameListSel& s, int32_t& r) {
    r = s.row_frame[b];
    if (!s.win_frame) return r;
    return r >= 0 && r < s.n_windows ? s.win_frame[r] : -1;
}
template <typename P>
__device__ __forceinline__ bool frame_of(int64_t b, P& frame, int64_t& tb, const FrameListSel& s) {
    int32_t r;
    const int32_t f = list_frame_of(b, s, r);
    const bool in_list = f >= 0 && f < s.n_frames;
    if (s.shared_tabs) tb = 0;      // (a box outside the list: frame 0's first table row, inside frame 0 whatever it holds)
    if (in_list) {
        const hg::FrameDesc d = s.desc[f];
        frame = (P)d.px;
        if (s.shared_tabs) tb = (int64_t)d.tab_row + (r - d.first);
    }
    return in_list;
}
// ld / fw / fh of box b's frame, by value: the kernel's own arguments `g`, or, under a list, ONE load of the box's descriptor
struct BoxGeo {
    int64_t ld;
    int fw, fh;
};
__device__ __forceinline__ BoxGeo geo(int64_t, BoxGeo g) { return g; }
__device__ __forceinline__ BoxGeo geo(int64_t, BoxGeo g, const FrameSel&) { return g; }
__device__ __forceinline__ BoxGeo geo(int64_t b, BoxGeo g, const FrameListSel& s) {
    int32_t r;
    const int32_t f = list_frame_of(b, s, r);
    if (!(f >= 0 && f < s.n_frames)) return g;
    const hg::FrameDesc d = s.desc[f];
    return BoxGeo{d.ld, d.w, d.h};
}

// One workgroup per (group of output rows, box): no index divisions, the row's source line and the column table are
// read once; four output pixels per thread and one vector store when the output is uint8.  ld_bytes: the frame's row stride in
// bytes (a colour frame's rows need not be a whole number of pixels apart).
template <typename FT, typename OT, typename... SEL>
__global__ void __launch_bounds__(256) k_extent_gather(const FT* __restrict__ frame0, int64_t ld_bytes0, const int32_t* __restrict__ tabs, int64_t n,
                                                        int w, int h, OT* __restrict__ out, int64_t ldo, SEL... sel) {
    const int y = blockIdx.x * blockDim.y + threadIdx.y;     // blockDim.y output rows per workgroup
    if (y >= h) return;
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        const FT* frame = frame0;
        int64_t tb = b;
        const bool in_stack = frame_of(b, frame, tb, sel...);
        const int64_t ld_bytes = geo(b, BoxGeo{ld_bytes0, 0, 0}, sel...).ld;      // (the tables hold the frame's limits: this kernel reads its row stride only)
        const int32_t* t = tabs + tb * (w + h);
        const int ys = in_stack ? t[w + y] : -1;
        const FT* src = (const FT*)((const char*)frame + (int64_t)(ys >= 0 ? ys : 0) * ld_bytes);
        OT* dst = out + b * ldo + (int64_t)y * w;
        if constexpr (sizeof(OT) == 1) {
            if ((w & 3) == 0 && (ldo & 3) == 0 && ((uintptr_t)out & 3) == 0) {
                for (int x = threadIdx.x * 4; x < w; x += blockDim.x * 4) {
                    uint32_t pk = 0;
                    int xs4[4];
                    if (((w + h) & 3) == 0) {            // table rows 16-byte aligned: one vector read
                        const int4 v4 = *(const int4*)(t + x);
                        xs4[0] = v4.x; xs4[1] = v4.y; xs4[2] = v4.z; xs4[3] = v4.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) xs4[k] = t[x + k];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int xs = xs4[k];
                        const uint32_t v = (xs >= 0 && ys >= 0) ? (uint32_t)(uint8_t)(OT)px_load(src, xs) : 0u;
                        pk |= v << (8 * k);
                    }
                    *(uint32_t*)(dst + x) = pk;
                }
                continue;
            }
        }
        for (int x = threadIdx.x; x < w; x += blockDim.x) {
            const int xs = t[x];
            dst[x] = (xs >= 0 && ys >= 0) ? (OT)px_load(src, xs) : (OT)0;
        }
    }
}

// A whole colour frame -> grey (hg_frame_to_gray_device; BPP = 1: a pitched copy).  A thread takes four neighbouring pixels of one
// row: ONE unaligned load of their 4 * BPP bytes (rows start at any byte; gfx950 runs in unaligned-access mode, as for
// k_extent_gather_u8x16 below) and one 4-byte store where dst rows are 4-aligned (`packed`), four byte stores otherwise.  The last
// w % 4 pixels of a row are read pixel by pixel, so no load touches a byte outside [row start, row start + w * BPP).  Rows beyond the
// grid's reach (more than 65535 rows of workgroups) are taken in further trips.
template <int BPP, bool BGR>
__global__ void __launch_bounds__(256) k_frame_to_gray(const uint8_t* __restrict__ src, int64_t ld_bytes, int h, int w, uint8_t* __restrict__ dst,
                                                        int64_t dst_ld, int packed) {
    const int64_t x = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x >= w) return;
    auto gray = [](const uint8_t* p) -> uint32_t {
        if constexpr (BPP == 1) return p[0];
        else return hg::rgb_to_gray(p[BGR ? 2 : 0], p[1], p[BGR ? 0 : 2]);
    };
    for (int64_t y = (int64_t)blockIdx.y * blockDim.y + threadIdx.y; y < h; y += (int64_t)gridDim.y * blockDim.y) {
        const uint8_t* s = src + y * ld_bytes + x * BPP;
        uint8_t* d = dst + y * dst_ld + x;
        if (x + 4 <= w) {
            uint32_t q[BPP];      // the four pixels' 4 * BPP bytes as BPP words (kept as words: a byte array is split into a load per channel)
            __builtin_memcpy(q, s, 4 * BPP);
            auto byte = [&](int i) -> uint32_t { return (q[i >> 2] >> (8 * (i & 3))) & 0xffu; };
            uint32_t pk = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (BPP == 1) pk = q[0];
                else pk |= (uint32_t)hg::rgb_to_gray(byte(k * BPP + (BGR ? 2 : 0)), byte(k * BPP + 1), byte(k * BPP + (BGR ? 0 : 2))) << (8 * k);
            }
            if (packed) {
                *(uint32_t*)d = pk;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = (uint8_t)(pk >> (8 * k));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)      // the row's last w % 4 pixels
                if (x + k < w) d[k] = (uint8_t)gray(s + k * BPP);
        }
    }
}

// uint8 frame -> uint8 windows whose rows are a multiple of 16 pixels (the cascade's first stage: 1738 windows of 128 x 128 from a
// 1000 x 562 frame, 28 MB of output).  k_extent_gather above issues, per four pixels, one table load, four byte loads and one
// 4-byte store: 24 memory instructions per 16 pixels, and it is their issue that bounds it (35 us = 0.8 TB/s written).  Here a
// thread owns sixteen output columns of its window for all the rows of its workgroup: the column indices are read once and kept in
// registers; a window at most twice as wide as its output (most of a pyramid: the number of windows falls with the square of
// their size) has the four source pixels of four output pixels inside eight consecutive bytes, so ONE unaligned 8-byte load
// (gfx950 runs in unaligned-access mode: the compiler itself emits global_load_dwordx2 for a byte-aligned 8-byte copy) replaces
// four byte loads; one 16-byte store per row.  5 memory instructions per 16 pixels.  Same bytes: every pixel is still
// frame[ytab[y]][xtab[x]] or 0.
template <typename... SEL>
__global__ void __launch_bounds__(256) k_extent_gather_u8x16(const uint8_t* __restrict__ frame0, int64_t ld0, int fw0, const int32_t* __restrict__ tabs,
                                                             int64_t n, int w, int h, uint8_t* __restrict__ out, int64_t ldo, int rows_per_wg, SEL... sel) {
    const int tpr = w >> 4;                                   // threads per output row (a power of two, <= 256)
    const int tx = threadIdx.x & (tpr - 1), ty = threadIdx.x / tpr, rows_per_pass = 256 / tpr;
    const int y_begin = blockIdx.x * rows_per_wg, y_end = min(h, y_begin + rows_per_wg);
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        const uint8_t* frame = frame0;
        int64_t tb = b;
        const bool in_stack = frame_of(b, frame, tb, sel...);      // (a box outside the stack: every row below reads as "outside the frame")
        const BoxGeo g = geo(b, BoxGeo{ld0, fw0, 0}, sel...);
        const int64_t ld = g.ld;
        const int fw = g.fw;
        const int32_t* t = tabs + tb * (w + h);
        int xs[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int4 v = *(const int4*)(t + tx * 16 + q * 4);      // (table rows are 16-byte aligned: checked by the launcher)
            xs[q * 4] = v.x; xs[q * 4 + 1] = v.y; xs[q * 4 + 2] = v.z; xs[q * 4 + 3] = v.w;
        }
        // a group of four columns can come out of one 8-byte load if all four are inside the frame, ascending within 8 bytes of the
        // first, and the 8 bytes end inside the frame's row.  The choice is made per WAVE and the loads carry no per-lane branch
        // (a branch per load puts a wait behind each one: the loads of a row, and of the four rows of the unrolled loop, must overlap)
        bool all8 = true;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int x0 = xs[g * 4];
            bool asc = x0 >= 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) asc = asc && xs[g * 4 + k] >= x0;
            all8 = all8 && asc && xs[g * 4 + 3] < x0 + 8 && xs[g * 4 + 2] < x0 + 8 && xs[g * 4 + 1] < x0 + 8 && x0 + 8 <= fw;
        }
        const bool wave8 = __builtin_amdgcn_ballot_w64(!all8) == 0;
        uint8_t* dst = out + b * ldo + tx * 16;
        if (wave8) {
#pragma unroll 4
            for (int y = y_begin + ty; y < y_end; y += rows_per_pass) {      // (unrolled: the rows' loads overlap, one latency for four rows)
                const int ys = in_stack ? t[w + y] : -1;
                const uint8_t* src = frame + (int64_t)(ys >= 0 ? ys : 0) * ld;
                uint32_t pk[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint64_t c;
                    __builtin_memcpy(&c, src + xs[g * 4], 8);
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v |= (uint32_t)((c >> (8 * (xs[g * 4 + k] - xs[g * 4]))) & 0xffull) << (8 * k);
                    pk[g] = ys >= 0 ? v : 0u;
                }
                *(uint4*)(dst + (int64_t)y * w) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            }
        } else {
            // wide windows, windows that leave the frame: a byte load per pixel from a clamped address, the value masked afterwards
            // (a middle tier — one 16-byte load per four pixels for windows up to four times as wide as their output — was measured:
            // 23.7 us against 20.2 for the first stage's 1738 windows; the third code path costs registers every wave pays for)
#pragma unroll 2
            for (int y = y_begin + ty; y < y_end; y += rows_per_pass) {
                const int ys = in_stack ? t[w + y] : -1;
                const uint8_t* src = frame + (int64_t)(ys >= 0 ? ys : 0) * ld;
                uint32_t pk[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int x = xs[g * 4 + k];
                        const uint32_t px = src[x >= 0 ? x : 0];
                        v |= ((x >= 0 && ys >= 0) ? px : 0u) << (8 * k);
                    }
                    pk[g] = v;
                }
                *(uint4*)(dst + (int64_t)y * w) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            }
        }
    }
}

// Per-box rotation record (Image.rotate's matrix as affine_fixed / ImagingScaleAffine use it).
struct RotCoef {
    int32_t mode;            // 0: no rotation, 1: fixed point, 2: scaling branch (sin rounds to 0), 3: outside the fixed-point range
    int32_t A[6];
    int32_t pad;
    double m0, m2, m4, m5;   // scaling branch
};

__device__ __forceinline__ double round15(double v) {       // Python round(v, 15) for |v| <= 1
    return d_div(rint(d_mul(v, 1e15)), 1e15);
}
__device__ __forceinline__ int32_t fix16(double v) {        // Geometry.c FIX(): FLOOR(v * 65536 + 0.5)
    const double x = d_add(d_mul(v, 65536.0), 0.5);
    return x >= 0.0 ? (int32_t)x : (int32_t)floor(x);
}

// The matrix Image.rotate(angle, center = centre of box b) builds, m[0..5]; false: angle % 360 == 0 (or not finite), no rotation
__device__ __forceinline__ bool rot_matrix(const double* __restrict__ boxes, const double* __restrict__ angs, int64_t b, double* m) {
    double a = fmod(angs[b], 360.0);                 // Python's float %: result carries the divisor's sign
    if (a < 0.0) a += 360.0;
    if (a == 360.0) a = 0.0;
    if (!(a != 0.0 && isfinite(a))) return false;
    const double cx = d_mul(d_add(boxes[b * 4], boxes[b * 4 + 2]), 0.5), cy = d_mul(d_add(boxes[b * 4 + 1], boxes[b * 4 + 3]), 0.5);
    const double r = -d_mul(a, 3.14159265358979323846 / 180.0);       // -math.radians(angle)
    const double c = round15(cos(r)), sn = round15(sin(r));
    m[0] = c; m[1] = sn; m[3] = -sn; m[4] = c;
    // transform(-cx, -cy, matrix) = (a x + b y) + c, then += center: every operation rounded on its own
    m[2] = d_add(d_add(d_add(d_mul(m[0], -cx), d_mul(m[1], -cy)), 0.0), cx);
    m[5] = d_add(d_add(d_add(d_mul(m[3], -cx), d_mul(m[4], -cy)), 0.0), cy);
    return true;
}

__device__ __forceinline__ RotCoef rot_coef_of(const double* __restrict__ boxes, const double* __restrict__ angs, int64_t b, int fw, int fh) {
    RotCoef rc{};
    double m[6];
    if (rot_matrix(boxes, angs, b, m)) {
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        if (m1 == 0.0 && m3 == 0.0) {
            rc.mode = 2;
            rc.m0 = m0; rc.m2 = m2; rc.m4 = m4; rc.m5 = m5;
        } else {
            // check_fixed() on the four corners of the rotated frame (same size as the frame)
            bool ok = true;
            const double xs[2] = {0.0, (double)fw}, ys[2] = {0.0, (double)fh};
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const double u = d_add(d_add(d_mul(xs[i], m0), d_mul(ys[j], m1)), m2);
                    const double v = d_add(d_add(d_mul(xs[i], m3), d_mul(ys[j], m4)), m5);
                    ok = ok && fabs(u) < 32768.0 && fabs(v) < 32768.0;
                }
            rc.mode = ok ? 1 : 3;
            rc.A[0] = fix16(m0); rc.A[1] = fix16(m1); rc.A[3] = fix16(m3); rc.A[4] = fix16(m4);
            rc.A[2] = fix16(d_add(d_add(m2, d_mul(m0, 0.5)), d_mul(m1, 0.5)));
            rc.A[5] = fix16(d_add(d_add(m5, d_mul(m3, 0.5)), d_mul(m4, 0.5)));
        }
    }
    return rc;
}

__device__ __forceinline__ void rot_coef_store(const double* __restrict__ boxes, const double* __restrict__ angs, int64_t b, int fw, int fh, RotCoef* out) {
    out[b] = rot_coef_of(boxes, angs, b, fw, fh);
}

// Rotated windows: per pixel, EXTENT table -> pixel of the rotated frame -> source pixel.  The frame (<= a few MB)
// sits in L2; the access pattern is a rotated scan line.
// One output row y of one box: EXTENT table (t[0..w) columns, t[w..w+h) rows) -> pixel of the rotated frame -> source pixel.
// uint8 windows: four pixels per thread and one 32-bit store (round 4: byte stores made the first stage's 1738 windows 79 us).
template <typename FT, typename OT>
__device__ __forceinline__ void gather_rot_row(const FT* __restrict__ frame, int64_t ld, int fw, int fh, const int32_t* t, const RotCoef& rc, int y,
                                               int w, OT* __restrict__ dst, bool packed, int tx, int ntx) {
    const int yr = t[w + y];
    double yo = 0.0;
    int ys2 = -1;
    if (rc.mode == 2 && yr >= 0) {      // ImagingScaleAffine on the rotated frame: yo = a5 + a4 / 2, then += a4 per row
        yo = d_add(rc.m5, d_mul(rc.m4, 0.5));
        for (int k = 0; k < yr; ++k) yo = d_add(yo, rc.m4);
        ys2 = yo < 0.0 ? -1 : (int)yo;
        if (ys2 >= fh) ys2 = -1;
    }
    auto pixel = [&](int x) -> OT {
        const int xr = t[x];
        int xs = -1, ys = -1;
        if (xr >= 0 && yr >= 0) {
            if (rc.mode == 0) {
                xs = xr; ys = yr;
            } else if (rc.mode == 1) {
                const int64_t xx = (int64_t)rc.A[2] + (int64_t)yr * rc.A[1] + (int64_t)xr * rc.A[0];
                const int64_t yy = (int64_t)rc.A[5] + (int64_t)yr * rc.A[4] + (int64_t)xr * rc.A[3];
                xs = (int)(xx >> 16); ys = (int)(yy >> 16);
            } else if (rc.mode == 2) {
                double xo = d_add(rc.m2, d_mul(rc.m0, 0.5));
                for (int k = 0; k < xr; ++k) xo = d_add(xo, rc.m0);
                xs = xo < 0.0 ? -1 : (int)xo;
                ys = ys2;
            }
        }
        const bool in = xs >= 0 && xs < fw && ys >= 0 && ys < fh;
        return in ? (OT)frame[(int64_t)ys * ld + xs] : (OT)0;
    };
    if constexpr (sizeof(OT) == 1) {
        if (packed) {
            // sixteen pixels per thread where the row allows (the launcher then gives a row w / 16 threads): the sixteen source
            // addresses first, then sixteen independent loads in flight and ONE 16-byte store — a thread with four pixels spent
            // its time in three dependent round trips (table -> frame -> store): 51 us for the first stage's 1738 windows
            if ((w & 15) == 0 && (((uintptr_t)dst) & 15) == 0 && rc.mode != 2) {
                // (round 5: no branch between the loads — the sixteen table entries as four 16-byte loads where the table row allows it,
                // the rotation mode tested once per box, every pixel load unconditional from a clamped address and masked afterwards;
                // with a branch around each load the compiler put a wait behind each one)
                const bool tab16 = ((uintptr_t)t & 15) == 0;
                const int mode = rc.mode;
                for (int x = tx * 16; x < w; x += ntx * 16) {
                    int xr[16];
                    if (tab16) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int4 v = *(const int4*)(t + x + q * 4);
                            xr[q * 4] = v.x; xr[q * 4 + 1] = v.y; xr[q * 4 + 2] = v.z; xr[q * 4 + 3] = v.w;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 16; ++q) xr[q] = t[x + q];
                    }
                    int64_t off[16];
                    bool in[16];
                    if (mode == 1) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int64_t xx = (int64_t)rc.A[2] + (int64_t)yr * rc.A[1] + (int64_t)xr[q] * rc.A[0];
                            const int64_t yy = (int64_t)rc.A[5] + (int64_t)yr * rc.A[4] + (int64_t)xr[q] * rc.A[3];
                            const int xs = (int)(xx >> 16), ys = (int)(yy >> 16);
                            in[q] = (xr[q] >= 0) & (yr >= 0) & (xs >= 0) & (xs < fw) & (ys >= 0) & (ys < fh);      // (&: no short-circuit branches)
                            off[q] = in[q] ? (int64_t)ys * ld + xs : 0;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            in[q] = (mode == 0) & (xr[q] >= 0) & (yr >= 0) & (xr[q] < fw) & (yr < fh);      // (mode 3: outside the fixed-point range, the window stays 0)
                            off[q] = in[q] ? (int64_t)yr * ld + xr[q] : 0;
                        }
                    }
                    uint32_t px[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) px[q] = (uint32_t)(uint8_t)frame[off[q]];
                    uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int q = 0; q < 16; ++q) pk[q >> 2] |= (in[q] ? px[q] : 0u) << (8 * (q & 3));
                    *(uint4*)(dst + x) = uint4{pk[0], pk[1], pk[2], pk[3]};
                }
                return;
            }
            for (int x = tx * 4; x < w; x += ntx * 4) {
                uint32_t pk = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) pk |= (uint32_t)(uint8_t)pixel(x + q) << (8 * q);
                *(uint32_t*)(dst + x) = pk;
            }
            return;
        }
    }
    for (int x = tx; x < w; x += ntx) dst[x] = pixel(x);
}

// Rotated windows, tables from memory (k_extent_tables, k_rot_coefs): the frame (<= a few MB) sits in L2; the access pattern is a
// rotated scan line.
template <typename FT, typename OT, typename... SEL>
__global__ void __launch_bounds__(256) k_extent_gather_rot(const FT* __restrict__ frame0, int64_t ld0, int fw0, int fh0, const int32_t* __restrict__ tabs,
                                                            const RotCoef* __restrict__ rot, int64_t n, int w, int h, OT* __restrict__ out, int64_t ldo,
                                                            SEL... sel) {
    const int y = blockIdx.x * blockDim.y + threadIdx.y;
    if (y >= h) return;
    const bool packed = sizeof(OT) == 1 && (w & 3) == 0 && (ldo & 3) == 0 && ((uintptr_t)out & 3) == 0;
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        if constexpr (sizeof...(SEL) == 0) {
            const RotCoef rc = rot[b];
            gather_rot_row<FT, OT>(frame0, ld0, fw0, fh0, tabs + b * (w + h), rc, y, w, out + b * ldo + (int64_t)y * w, packed, threadIdx.x, blockDim.x);
        } else {
            const FT* frame = frame0;
            int64_t tb = b;      // (rotated boxes: a table per box)
            RotCoef rc = rot[b];
            if (!frame_of(b, frame, tb, sel...)) rc.mode = 3;      // a box outside the stack: as outside the fixed-point range, the window stays 0
            const BoxGeo g = geo(b, BoxGeo{ld0, fw0, fh0}, sel...);
            gather_rot_row<FT, OT>(frame, g.ld, g.fw, g.fh, tabs + b * (w + h), rc, y, w, out + b * ldo + (int64_t)y * w, packed, threadIdx.x, blockDim.x);
        }
    }
}

// ---- BILINEAR / BICUBIC windows (include/higsfa.h, hg_patcher_extract_filter_device) --------------------------------------------
// PIL's ImagingGenericTransform with affine_transform and bilinear_filter8 / bicubic_filter8 (Geometry.c), for uint8 frames: the
// coordinate entries (FiltEnt, filter_coord) and the filters (bicubic, filter_sample) are in hg_filter_dev.hpp.

// Image.rotate's matrix as doubles (the 16.16 fixed point is NEAREST's); rotated = 0: angle % 360 == 0, the window is cut from the frame itself
struct RotAff {
    double m[6];
    int32_t rotated, pad;
};

// a0 xin + a1 yin + a2 with a = ((x1 - x0) / w, 0, x0, 0, (y1 - y0) / h, y0): the zero product adds nothing to the sum
__device__ __forceinline__ FiltEnt filter_entry(const double* __restrict__ box, int e, int w, int h, int fw, int fh) {
    const int axis = e >= w ? 1 : 0, i = axis ? e - w : e;
    const double lo = box[axis], hi = box[2 + axis];
    const double a = d_div(d_sub(hi, lo), (double)(axis ? h : w));
    return filter_coord(d_add(d_mul(a, d_add((double)i, 0.5)), lo), axis ? fh : fw);
}

__global__ void k_filter_tables(const double* __restrict__ boxes, int64_t n, int w, int h, int fw, int fh, FiltEnt* __restrict__ tabs,
                                const double* __restrict__ angs, RotAff* __restrict__ rot) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wh = w + h;
    if (id >= n * wh) return;
    const int64_t b = id / wh;
    const int e = (int)(id - b * wh);
    tabs[b * wh + e] = filter_entry(boxes + b * 4, e, w, h, fw, fh);
    if (angs && e == 0) {
        RotAff ra{};
        ra.rotated = rot_matrix(boxes, angs, b, ra.m) ? 1 : 0;
        rot[b] = ra;
    }
}

// The table builders of a frame LIST: k_extent_tables / k_filter_tables with the frame's size taken per box from the box's descriptor
// (the entries and the rotation records are functions of that size).  A box outside the list gets the size 0 x 0: every entry "outside".
__device__ __forceinline__ void list_size_of(int64_t b, const FrameListSel& s, int& fw, int& fh) {
    int32_t r;
    const int32_t f = list_frame_of(b, s, r);
    fw = fh = 0;
    if (f >= 0 && f < s.n_frames) {
        fw = s.desc[f].w;
        fh = s.desc[f].h;
    }
}
__global__ void k_extent_tables_list(const double* __restrict__ boxes, int64_t n, int w, int h, int32_t* __restrict__ tabs, const double* __restrict__ angs,
                                     RotCoef* __restrict__ rot, FrameListSel s) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wh = w + h;
    if (id >= n * wh) return;
    const int64_t b = id / wh;
    const int e = (int)(id - b * wh);
    int fw, fh;
    list_size_of(b, s, fw, fh);
    tabs[b * wh + e] = extent_entry(boxes + b * 4, e, w, h, fw, fh);
    if (angs && e == 0) rot_coef_store(boxes, angs, b, fw, fh, rot);
}
__global__ void k_filter_tables_list(const double* __restrict__ boxes, int64_t n, int w, int h, FiltEnt* __restrict__ tabs, const double* __restrict__ angs,
                                     RotAff* __restrict__ rot, FrameListSel s) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wh = w + h;
    if (id >= n * wh) return;
    const int64_t b = id / wh;
    const int e = (int)(id - b * wh);
    int fw, fh;
    list_size_of(b, s, fw, fh);
    tabs[b * wh + e] = filter_entry(boxes + b * 4, e, w, h, fw, fh);
    if (angs && e == 0) {
        RotAff ra{};
        ra.rotated = rot_matrix(boxes, angs, b, ra.m) ? 1 : 0;
        rot[b] = ra;
    }
}

// The descriptors of a frame list, from the launch's own arguments into the device table (hg::put_frame_descs)
constexpr int kDescChunk = 64;
struct DescChunk {
    hg::FrameDesc d[kDescChunk];
};
__global__ void k_put_descs(DescChunk c, int n, hg::FrameDesc* __restrict__ dst) {
    const int i = threadIdx.x;
    if (i < n) dst[i] = c.d[i];
}

// Pixel (xr, yr) of frame.rotate(angle, F, center): affine_transform with the rotation's matrix, then the filter on the frame
template <int F>
__device__ __forceinline__ uint8_t rot_pixel(const uint8_t* __restrict__ frame, int64_t ld, int W, int H, const double* m, int xr, int yr) {
    const double xin = d_add((double)xr, 0.5), yin = d_add((double)yr, 0.5);
    const FiltEnt ex = filter_coord(d_add(d_add(d_mul(m[0], xin), d_mul(m[1], yin)), m[2]), W);
    const FiltEnt ey = filter_coord(d_add(d_add(d_mul(m[3], xin), d_mul(m[4], yin)), m[5]), H);
    if (ex.i == kFiltOutside || ey.i == kFiltOutside) return 0;
    return filter_sample<F>([&](int xc, int yc) { return (double)frame[(int64_t)yc * ld + xc]; }, ex.i, ex.d, ey.i, ey.d, W, H);
}

// Unrotated windows: a workgroup per (group of output rows, box), a thread per output pixel
template <int F, typename OT, typename... SEL>
__global__ void __launch_bounds__(256) k_filter_gather(const uint8_t* __restrict__ frame0, int64_t ld0, int fw0, int fh0, const FiltEnt* __restrict__ tabs,
                                                        int64_t n, int w, int h, OT* __restrict__ out, int64_t ldo, SEL... sel) {
    const int y = blockIdx.x * blockDim.y + threadIdx.y;
    if (y >= h) return;
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        const uint8_t* frame = frame0;
        int64_t tb = b;
        const bool in_stack = frame_of(b, frame, tb, sel...);
        const BoxGeo g = geo(b, BoxGeo{ld0, fw0, fh0}, sel...);
        const int64_t ld = g.ld;
        const int fw = g.fw, fh = g.fh;
        const FiltEnt* t = tabs + tb * (w + h);
        FiltEnt ey = t[w + y];
        if (!in_stack) ey.i = kFiltOutside;      // a box outside the stack: every row outside the frame
        OT* dst = out + b * ldo + (int64_t)y * w;
        for (int x = threadIdx.x; x < w; x += blockDim.x) {
            const FiltEnt ex = t[x];
            uint8_t v = 0;
            if (ex.i != kFiltOutside && ey.i != kFiltOutside)
                v = filter_sample<F>([&](int xc, int yc) { return (double)frame[(int64_t)yc * ld + xc]; }, ex.i, ex.d, ey.i, ey.d, fw, fh);
            dst[x] = (OT)v;
        }
    }
}

// Rotated windows: frame.rotate(angle, F, center).transform((w, h), EXTENT, box, F).  Each tap of the second step is a pixel of the
// rotated frame, itself 2 x 2 / 4 x 4 source reads and a quantisation: composed naively, 16 / 256 source reads per output pixel.  A
// workgroup takes a 16 x 16 tile of output pixels; the taps of the tile cover a rectangle of the rotated frame (from the tile's
// table entries), and when that rectangle is small enough it is computed ONCE into LDS as uint8 and the tile filters from there.  A
// tile of a window shrunk so much that its taps are sparse in the rectangle computes each tap where it is used instead.  Both paths
// give the same bytes (rot_pixel either way).  The limit is counted in the tile's own taps taken one by one (256 x 4 or 256 x 16
// rotated pixels) and was settled by measurement (profiles/r08_filter_times.txt, 300 windows of 128 x 128 at 17 degrees):
//   BILINEAR stages a rectangle of at most 1 x its taps (1024 pixels: windows shrunk up to 1.9 x).  Staging up to 2 x was slower:
//     windows cut from 320 pixels (41 x 41 per tile) 0.121 ms staged against 0.098 ms tap by tap.
//   BICUBIC stages up to 2 x its taps (8192 pixels, kFiltPatch bytes: windows shrunk up to 5.4 x).  A 128-pixel window cut from 576
//     pixels of a 1000-pixel frame (75 x 75 per tile, 5625 rotated pixels against the 4096 of the taps) took 1.100 ms staged against
//     1.237 ms tap by tap, although it computes more rotated pixels: tap by tap, sixteen threads compute the same rotated pixel
//     at the same time and every one of them reads the frame from L2, where the staged tile reads LDS.
constexpr int kFiltTile = 16, kFiltPatch = 256 * 16 * 2;
template <int F, typename OT, typename... SEL>
__global__ void __launch_bounds__(256) k_filter_gather_rot(const uint8_t* __restrict__ frame0, int64_t ld0, int fw0, int fh0, const FiltEnt* __restrict__ tabs,
                                                            const RotAff* __restrict__ rot, int64_t n, int w, int h, OT* __restrict__ out, int64_t ldo,
                                                            int tiles_x, SEL... sel) {
    constexpr int LO = F == HG_FILTER_BICUBIC ? 1 : 0, HI = F == HG_FILTER_BICUBIC ? 2 : 1, TAPS = (LO + HI + 1) * (LO + HI + 1);
    constexpr int kStageLimit = TAPS * kFiltTile * kFiltTile * (F == HG_FILTER_BICUBIC ? 2 : 1);      // rotated pixels; see above
    static_assert(kStageLimit <= kFiltPatch, "the staged rectangle must fit the LDS patch");
    __shared__ uint8_t patch[kFiltPatch];
    __shared__ int rng[4];
    const int tx = threadIdx.x & (kFiltTile - 1), ty = threadIdx.x / kFiltTile;
    const int ox = (int)(blockIdx.x % tiles_x) * kFiltTile + tx, oy = (int)(blockIdx.x / tiles_x) * kFiltTile + ty;
    const bool live = ox < w && oy < h;
    auto clip = [](int v, int lim) { return v < 0 ? 0 : v < lim ? v : lim - 1; };
    const uint8_t* frame = frame0;
    int64_t ld = ld0;
    int fw = fw0, fh = fh0;
    auto frame_tap = [&](int xc, int yc) { return (double)frame[(int64_t)yc * ld + xc]; };
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {      // (every thread of the workgroup takes every trip: barriers below)
        int64_t tb = b;      // (rotated boxes: a table per box)
        frame = frame0;
        const bool in_stack = frame_of(b, frame, tb, sel...);
        const BoxGeo g = geo(b, BoxGeo{ld0, fw0, fh0}, sel...);
        ld = g.ld;      // (frame_tap reads frame and ld by reference)
        fw = g.fw;
        fh = g.fh;      // uniform per workgroup; a box outside the stack: no entry inside the frame
        const FiltEnt* t = tabs + b * (w + h);
        FiltEnt ex, ey;
        ex.i = ey.i = kFiltOutside;
        ex.d = ey.d = 0.0;
        if (live && in_stack) {
            ex = t[ox];
            ey = t[w + oy];
        }
        const bool inside = ex.i != kFiltOutside && ey.i != kFiltOutside;
        const RotAff ra = rot[b];
        uint8_t v = 0;
        if (!ra.rotated) {
            if (inside) v = filter_sample<F>(frame_tap, ex.i, ex.d, ey.i, ey.d, fw, fh);
        } else {
            __syncthreads();      // the previous box's reads of patch / rng are done
            if (threadIdx.x == 0) {
                rng[0] = rng[2] = INT32_MAX;
                rng[1] = rng[3] = INT32_MIN;
            }
            __syncthreads();
            // the tile's first row holds all its columns and its first column all its rows (both exist: the tile does)
            if (ty == 0 && ex.i != kFiltOutside) {
                atomicMin(&rng[0], clip(ex.i - LO, fw));
                atomicMax(&rng[1], clip(ex.i + HI, fw));
            }
            if (tx == 0 && ey.i != kFiltOutside) {
                atomicMin(&rng[2], clip(ey.i - LO, fh));
                atomicMax(&rng[3], clip(ey.i + HI, fh));
            }
            __syncthreads();
            const int xlo = rng[0], xhi = rng[1], ylo = rng[2], yhi = rng[3];
            // (an axis none of whose entries is inside the frame leaves its range at INT32_MAX / INT32_MIN: tested before any difference is taken)
            const bool any = xhi >= xlo && yhi >= ylo;
            const int pw = any ? xhi - xlo + 1 : 0, ph = any ? yhi - ylo + 1 : 0;
            const bool staged = any && (int64_t)pw * ph <= kStageLimit;
            if (staged) {
                const int np = pw * ph;      // <= kFiltPatch
                for (int idx = threadIdx.x; idx < np; idx += blockDim.x) {
                    const int py = idx / pw, px = idx - py * pw;
                    patch[idx] = rot_pixel<F>(frame, ld, fw, fh, ra.m, xlo + px, ylo + py);
                }
                __syncthreads();
                if (inside) v = filter_sample<F>([&](int xc, int yc) { return (double)patch[(yc - ylo) * pw + (xc - xlo)]; }, ex.i, ex.d, ey.i, ey.d, fw, fh);
            } else if (inside) {
                v = filter_sample<F>([&](int xc, int yc) { return (double)rot_pixel<F>(frame, ld, fw, fh, ra.m, xc, yc); }, ex.i, ex.d, ey.i, ey.d, fw, fh);
            }
        }
        if (live) out[b * ldo + (int64_t)oy * w + ox] = (OT)v;
    }
}

// (Round 4 also measured tables + coefficients + gather as ONE launch, a workgroup per box building its tables and coefficients in
// LDS: 48.6 us against 38.5 for the first stage's 1738 windows and 25 against 21 for a few hundred — one thread's double-precision
// fmod / cos / sin and the dependent additions of the tables sit on every workgroup's critical path instead of being spread over
// a launch of their own.  Not kept.)

template <typename F>
int guarded(F&& fn) {
    try {
        fn();
        return HG_OK;
    } catch (const hg::Error& e) {
        hg::set_last_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        hg::set_last_error(e.what());
        return HG_ERR_STATE;
    }
}

// ld_bytes: the frame's row stride in bytes (ld * sizeof(FT) for the scalar pixel types)
// sel: nothing, or the FrameSel of a frame stack (the kernels' optional last argument)
template <typename FT, typename... SEL>
void launch_gather(const void* frame, int64_t ld_bytes, int fw, const int32_t* tabs, int64_t n, int w, int h, void* out, int out_dtype, int64_t ldo,
                   hipStream_t st, SEL... sel) {
    if constexpr (sizeof(FT) == 1) {
        const int tpr = w >> 4;
        if (out_dtype == HG_U8 && (w & 15) == 0 && tpr >= 1 && tpr <= 256 && (tpr & (tpr - 1)) == 0 && ((w + h) & 3) == 0 && (ldo & 15) == 0 &&
            ((uintptr_t)out & 15) == 0 && ((uintptr_t)tabs & 15) == 0) {
            // whole windows per workgroup while that leaves >= 1024 workgroups, else row chunks (the column indices are read once per chunk)
            const int rows_per_pass = 256 / tpr;
            int passes = (h + rows_per_pass - 1) / rows_per_pass;
            while (passes > 1 && n * ((h + rows_per_pass * passes - 1) / (rows_per_pass * passes)) < 1024) passes = (passes + 1) / 2;
            const int rows_per_wg = rows_per_pass * passes;
            const dim3 grid((unsigned)((h + rows_per_wg - 1) / rows_per_wg), (unsigned)std::min<int64_t>(n, 65535));
            hipLaunchKernelGGL((k_extent_gather_u8x16<SEL...>), grid, 256, 0, st, (const uint8_t*)frame, ld_bytes, fw, tabs, n, w, h, (uint8_t*)out, ldo, rows_per_wg, sel...);
            return;
        }
    }
    const unsigned tx = w >= 1024 ? 256 : w >= 256 ? 64 : 32;       // four pixels per thread on the uint8 path
    const dim3 thr(tx, 256 / tx);
    const dim3 grid((unsigned)((h + thr.y - 1) / thr.y), (unsigned)std::min<int64_t>(n, 65535));
    switch (out_dtype) {
        case HG_U8: hipLaunchKernelGGL((k_extent_gather<FT, uint8_t, SEL...>), grid, thr, 0, st, (const FT*)frame, ld_bytes, tabs, n, w, h, (uint8_t*)out, ldo, sel...); break;
        case HG_F32: hipLaunchKernelGGL((k_extent_gather<FT, float, SEL...>), grid, thr, 0, st, (const FT*)frame, ld_bytes, tabs, n, w, h, (float*)out, ldo, sel...); break;
        default: hipLaunchKernelGGL((k_extent_gather<FT, double, SEL...>), grid, thr, 0, st, (const FT*)frame, ld_bytes, tabs, n, w, h, (double*)out, ldo, sel...); break;
    }
}

// the gather by frame format: HG_FRAME_L is the grey frame's own launch (the 16-pixel kernel where it applies)
void launch_gather_format(int format, const void* frame, int64_t ld_bytes, int fw, const int32_t* tabs, int64_t n, int w, int h, void* out, int out_dtype,
                          int64_t ldo, hipStream_t st) {
    switch (format) {
        case HG_FRAME_L: launch_gather<uint8_t>(frame, ld_bytes, fw, tabs, n, w, h, out, out_dtype, ldo, st); break;
        case HG_FRAME_RGB: launch_gather<ColorPx<3, false>>(frame, ld_bytes, fw, tabs, n, w, h, out, out_dtype, ldo, st); break;
        case HG_FRAME_BGR: launch_gather<ColorPx<3, true>>(frame, ld_bytes, fw, tabs, n, w, h, out, out_dtype, ldo, st); break;
        case HG_FRAME_RGBA: launch_gather<ColorPx<4, false>>(frame, ld_bytes, fw, tabs, n, w, h, out, out_dtype, ldo, st); break;
        default: launch_gather<ColorPx<4, true>>(frame, ld_bytes, fw, tabs, n, w, h, out, out_dtype, ldo, st); break;
    }
}

template <typename FT, typename... SEL>
void launch_gather_rot(const void* frame, int64_t ld, int fw, int fh, const int32_t* tabs, const RotCoef* rot, int64_t n, int w, int h, void* out,
                       int out_dtype, int64_t ldo, hipStream_t st, SEL... sel) {
    // uint8 windows: a thread packs sixteen pixels where the row is a multiple of 16 (a 128-pixel row takes 8 threads and a
    // workgroup 32 rows), four otherwise
    const unsigned tx = out_dtype == HG_U8 ? ((w & 15) == 0 ? (w >= 2048 ? 128 : w >= 1024 ? 64 : w >= 512 ? 32 : w >= 256 ? 16 : w >= 128 ? 8 : 4)
                                                            : (w >= 512 ? 128 : w >= 256 ? 64 : 32))
                                           : (w >= 128 ? 128 : w >= 64 ? 64 : 32);
    const dim3 thr(tx, 256 / tx);
    const dim3 grid((unsigned)((h + thr.y - 1) / thr.y), (unsigned)std::min<int64_t>(n, 65535));
    switch (out_dtype) {
        case HG_U8: hipLaunchKernelGGL((k_extent_gather_rot<FT, uint8_t, SEL...>), grid, thr, 0, st, (const FT*)frame, ld, fw, fh, tabs, rot, n, w, h, (uint8_t*)out, ldo, sel...); break;
        case HG_F32: hipLaunchKernelGGL((k_extent_gather_rot<FT, float, SEL...>), grid, thr, 0, st, (const FT*)frame, ld, fw, fh, tabs, rot, n, w, h, (float*)out, ldo, sel...); break;
        default: hipLaunchKernelGGL((k_extent_gather_rot<FT, double, SEL...>), grid, thr, 0, st, (const FT*)frame, ld, fw, fh, tabs, rot, n, w, h, (double*)out, ldo, sel...); break;
    }
}

template <int F, typename... SEL>
void launch_filter(const uint8_t* frame, int64_t ld, int fw, int fh, const FiltEnt* tabs, const RotAff* rot, int64_t n, int w, int h, void* out, int out_dtype,
                   int64_t ldo, hipStream_t st, SEL... sel) {
    const unsigned ny = (unsigned)std::min<int64_t>(n, 65535);
    if (rot) {
        const int tiles_x = (w + kFiltTile - 1) / kFiltTile, tiles_y = (h + kFiltTile - 1) / kFiltTile;      // <= 256 each (check_args)
        const dim3 grid((unsigned)(tiles_x * tiles_y), ny);
        switch (out_dtype) {
            case HG_U8: hipLaunchKernelGGL((k_filter_gather_rot<F, uint8_t, SEL...>), grid, 256, 0, st, frame, ld, fw, fh, tabs, rot, n, w, h, (uint8_t*)out, ldo, tiles_x, sel...); break;
            case HG_F32: hipLaunchKernelGGL((k_filter_gather_rot<F, float, SEL...>), grid, 256, 0, st, frame, ld, fw, fh, tabs, rot, n, w, h, (float*)out, ldo, tiles_x, sel...); break;
            default: hipLaunchKernelGGL((k_filter_gather_rot<F, double, SEL...>), grid, 256, 0, st, frame, ld, fw, fh, tabs, rot, n, w, h, (double*)out, ldo, tiles_x, sel...); break;
        }
        return;
    }
    const unsigned tx = w >= 256 ? 256 : w >= 128 ? 128 : w >= 64 ? 64 : 32;
    const dim3 thr(tx, 256 / tx);
    const dim3 grid((unsigned)((h + thr.y - 1) / thr.y), ny);
    switch (out_dtype) {
        case HG_U8: hipLaunchKernelGGL((k_filter_gather<F, uint8_t, SEL...>), grid, thr, 0, st, frame, ld, fw, fh, tabs, n, w, h, (uint8_t*)out, ldo, sel...); break;
        case HG_F32: hipLaunchKernelGGL((k_filter_gather<F, float, SEL...>), grid, thr, 0, st, frame, ld, fw, fh, tabs, n, w, h, (float*)out, ldo, sel...); break;
        default: hipLaunchKernelGGL((k_filter_gather<F, double, SEL...>), grid, thr, 0, st, frame, ld, fw, fh, tabs, n, w, h, (double*)out, ldo, sel...); break;
    }
}

void check_args(const hg_patcher* p, const void* frame, int frame_dtype, int fh, int fw, int64_t ld, const double* boxes, int64_t n,
                int w, int h, const void* out, int out_dtype, int64_t ldo) {
    if (!p) hg::fail(HG_ERR_ARG, "null patcher handle");
    if (frame_dtype != HG_U8 && frame_dtype != HG_F32) hg::fail(HG_ERR_ARG, "frame dtype must be HG_U8 or HG_F32");
    if (out_dtype != HG_U8 && out_dtype != HG_F32 && out_dtype != HG_F64) hg::fail(HG_ERR_ARG, "bad output dtype");
    if (fh <= 0 || fw <= 0 || ld < fw) hg::fail(HG_ERR_ARG, "bad frame geometry");
    if (w <= 0 || h <= 0 || w > 4096 || h > 4096) hg::fail(HG_ERR_ARG, "bad sub-image size");
    if (n < 0 || ldo < (int64_t)w * h) hg::fail(HG_ERR_ARG, "bad batch geometry");
    if (n > 0 && (!frame || !boxes || !out)) hg::fail(HG_ERR_ARG, "null data pointer");
}

void check_filter(int filter, int frame_dtype) {
    if (filter != HG_FILTER_NEAREST && filter != HG_FILTER_BILINEAR && filter != HG_FILTER_BICUBIC)
        hg::fail(HG_ERR_ARG, "unknown interpolation filter %d (0 NEAREST, 2 BILINEAR, 3 BICUBIC)", filter);
    if (filter != HG_FILTER_NEAREST && frame_dtype != HG_U8) hg::fail(HG_ERR_ARG, "BILINEAR / BICUBIC windows need an HG_U8 frame");
}

// The NEAREST index tables of n unrotated boxes, built on `st`: key != 0 — kept in the patcher's ring under that key
// (hg_patcher_extract_keyed_device's contract) and built on the first use only; key == 0 — the patcher's own table buffer, rebuilt.
// The tables hold pixel indices: they do not depend on the frame's format.
const int32_t* nearest_tables(hg_patcher* p, uint64_t key, int frame_h, int frame_w, const double* boxes_dev, int64_t n, int out_w, int out_h, hipStream_t st) {
    const int64_t n_ent = n * (out_w + out_h);
    if ((n_ent + 255) / 256 > 0x7fffffffll) hg::fail(HG_ERR_ARG, "too many boxes");
    int32_t* tabs = nullptr;
    if (key) {
        hg_patcher::Keyed* K = nullptr;
        for (auto& k : p->keyed)
            if (k.key == key && !k.filtered && k.n == n && k.out_w == out_w && k.out_h == out_h && k.frame_w == frame_w && k.frame_h == frame_h) K = &k;
        if (K) return (const int32_t*)K->tabs.p;
        // first use of this key (or its shape changed): build the tables, in stream order, into a buffer of their own
        K = &p->keyed[p->keyed_next];
        p->keyed_next = (p->keyed_next + 1) % 4;
        if (K->tabs.p && (size_t)n_ent * 4 > K->tabs.bytes) HG_HIP(hipStreamSynchronize(st));      // a launch in flight may still read the old buffer
        K->tabs.alloc((size_t)n_ent * 4);
        K->key = key; K->n = n; K->out_w = out_w; K->out_h = out_h; K->frame_w = frame_w; K->frame_h = frame_h; K->filtered = 0;
        tabs = (int32_t*)K->tabs.p;
    } else {
        p->tabs.alloc((size_t)n_ent * 4);
        tabs = (int32_t*)p->tabs.p;
    }
    hipLaunchKernelGGL(k_extent_tables, (unsigned)((n_ent + 255) / 256), 256, 0, st, boxes_dev, n, out_w, out_h, frame_w, frame_h, tabs, (const double*)nullptr,
                       (RotCoef*)nullptr);
    return tabs;
}

// The BILINEAR / BICUBIC coordinate tables of n boxes (they hold coordinates, not taps: both filters share them), built on `st`, and,
// for rotated boxes, their matrices (*rot).  key != 0 and no angles: kept per key under hg_patcher_extract_keyed_device's contract.
const FiltEnt* filter_tables(hg_patcher* p, uint64_t key, int frame_h, int frame_w, const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w,
                             int out_h, hipStream_t st, const RotAff** rot) {
    const int64_t n_ent = n * (out_w + out_h);
    if ((n_ent + 255) / 256 > 0x7fffffffll) hg::fail(HG_ERR_ARG, "too many boxes");
    *rot = nullptr;
    if (key && !delta_angs_dev) {
        hg_patcher::Keyed* K = nullptr;
        for (auto& k : p->keyed)
            if (k.key == key && k.filtered && k.n == n && k.out_w == out_w && k.out_h == out_h && k.frame_w == frame_w && k.frame_h == frame_h) K = &k;
        if (!K) {
            K = &p->keyed[p->keyed_next];
            p->keyed_next = (p->keyed_next + 1) % 4;
            if (K->tabs.p && (size_t)n_ent * sizeof(FiltEnt) > K->tabs.bytes) HG_HIP(hipStreamSynchronize(st));      // a launch in flight may still read the old buffer
            K->tabs.alloc((size_t)n_ent * sizeof(FiltEnt));
            K->key = key; K->n = n; K->out_w = out_w; K->out_h = out_h; K->frame_w = frame_w; K->frame_h = frame_h; K->filtered = 1;
            hipLaunchKernelGGL(k_filter_tables, (unsigned)((n_ent + 255) / 256), 256, 0, st, boxes_dev, n, out_w, out_h, frame_w, frame_h, (FiltEnt*)K->tabs.p,
                               (const double*)nullptr, (RotAff*)nullptr);
        }
        return (const FiltEnt*)K->tabs.p;
    }
    p->ftabs.alloc((size_t)n_ent * sizeof(FiltEnt));
    if (delta_angs_dev) p->frot.alloc((size_t)n * sizeof(RotAff));
    hipLaunchKernelGGL(k_filter_tables, (unsigned)((n_ent + 255) / 256), 256, 0, st, boxes_dev, n, out_w, out_h, frame_w, frame_h, (FiltEnt*)p->ftabs.p,
                       delta_angs_dev, delta_angs_dev ? (RotAff*)p->frot.p : nullptr);
    if (delta_angs_dev) *rot = (const RotAff*)p->frot.p;
    return (const FiltEnt*)p->ftabs.p;
}

void check_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        hg::fail(HG_ERR_DEVICE, "no HIP device available (this library has no CPU execution path)");
    if (device < 0 || device >= count) hg::fail(HG_ERR_DEVICE, "device %d out of range", device);
}

// what every entry that reads a colour frame refuses before it launches anything
void check_color_frame(int format, int frame_h, int frame_w, int64_t ld_bytes) {
    const int bpp = hg::frame_bpp(format);
    if (!bpp) hg::fail(HG_ERR_ARG, "unknown frame format %d (0 L, 1 RGB, 2 BGR, 3 RGBA, 4 BGRA)", format);
    if (frame_h <= 0 || frame_w <= 0 || ld_bytes < (int64_t)frame_w * bpp)
        hg::fail(HG_ERR_ARG, "bad frame geometry: %d rows of %d pixels of %d bytes, %lld bytes apart", frame_h, frame_w, bpp, (long long)ld_bytes);
}

template <int BPP, bool BGR>
void launch_to_gray(const void* src, int64_t ld_bytes, int h, int w, uint8_t* dst, int64_t dst_ld, hipStream_t st) {
    const int w4 = (w + 3) / 4;                                          // threads a row needs
    const unsigned tx = w4 > 64 ? 256 : w4 > 32 ? 64 : 32;
    const dim3 thr(tx, 256 / tx);
    const dim3 grid((unsigned)((w4 + tx - 1) / tx), (unsigned)std::min<int64_t>(((int64_t)h + thr.y - 1) / thr.y, 65535));
    const int packed = ((uintptr_t)dst & 3) == 0 && (dst_ld & 3) == 0 ? 1 : 0;
    hipLaunchKernelGGL((k_frame_to_gray<BPP, BGR>), grid, thr, 0, st, (const uint8_t*)src, ld_bytes, h, w, dst, dst_ld, packed);
}

}  // namespace

extern "C" {

int hg_frame_to_gray_device(int device, const void* src_dev, int format, int frame_h, int frame_w, int64_t ld_bytes, uint8_t* dst_dev, int64_t dst_ld,
                            void* stream) {
    return guarded([&] {
        check_color_frame(format, frame_h, frame_w, ld_bytes);
        if (!src_dev || !dst_dev) hg::fail(HG_ERR_ARG, "null data pointer");
        if (dst_ld < frame_w) hg::fail(HG_ERR_ARG, "bad output row stride %lld for %d pixels", (long long)dst_ld, frame_w);
        check_device(device);
        HG_HIP(hipSetDevice(device));
        hipStream_t st = (hipStream_t)stream;
        switch (format) {
            case HG_FRAME_L: launch_to_gray<1, false>(src_dev, ld_bytes, frame_h, frame_w, dst_dev, dst_ld, st); break;
            case HG_FRAME_RGB: launch_to_gray<3, false>(src_dev, ld_bytes, frame_h, frame_w, dst_dev, dst_ld, st); break;
            case HG_FRAME_BGR: launch_to_gray<3, true>(src_dev, ld_bytes, frame_h, frame_w, dst_dev, dst_ld, st); break;
            case HG_FRAME_RGBA: launch_to_gray<4, false>(src_dev, ld_bytes, frame_h, frame_w, dst_dev, dst_ld, st); break;
            default: launch_to_gray<4, true>(src_dev, ld_bytes, frame_h, frame_w, dst_dev, dst_ld, st); break;
        }
        HG_HIP(hipGetLastError());
    });
}

int hg_patcher_extract_format_device(hg_patcher* p, int frame_format, const void* frame_dev, int frame_h, int frame_w, int64_t ld_bytes,
                                     const double* boxes_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    return hg::patcher_extract_format(p, 0, frame_format, frame_dev, frame_h, frame_w, ld_bytes, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
}

int hg_patcher_create(int device, hg_patcher** out) {
    return guarded([&] {
        if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
        *out = nullptr;
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            hg::fail(HG_ERR_DEVICE, "no HIP device available (this library has no CPU execution path)");
        if (device < 0 || device >= count) hg::fail(HG_ERR_DEVICE, "device %d out of range", device);
        auto p = std::make_unique<hg_patcher>();
        p->device = device;
        *out = p.release();
    });
}

void hg_patcher_free(hg_patcher* p) {
    if (p && p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
}

int hg_patcher_extract_rotate_device(hg_patcher* p, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                                     const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w, int out_h, void* out_dev,
                                     int out_dtype, int64_t ldo, void* stream) {
    return guarded([&] {
        check_args(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo);
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        p->tabs.alloc((size_t)n * (out_w + out_h) * 4);
        const int64_t n_ent = n * (out_w + out_h);
        if ((n_ent + 255) / 256 > 0x7fffffffll) hg::fail(HG_ERR_ARG, "too many boxes");
        if (delta_angs_dev) {
            if (frame_w >= 32768 || frame_h >= 32768) hg::fail(HG_ERR_ARG, "rotated windows need a frame smaller than 32768 pixels per side");
            p->rot.alloc((size_t)n * sizeof(RotCoef));
        }
        hipLaunchKernelGGL(k_extent_tables, (unsigned)((n_ent + 255) / 256), 256, 0, st, boxes_dev, n, out_w, out_h, frame_w, frame_h,
                           (int32_t*)p->tabs.p, delta_angs_dev, delta_angs_dev ? (RotCoef*)p->rot.p : nullptr);
        if (delta_angs_dev) {
            if (frame_dtype == HG_U8)
                launch_gather_rot<uint8_t>(frame_dev, ld, frame_w, frame_h, (const int32_t*)p->tabs.p, (const RotCoef*)p->rot.p, n, out_w, out_h, out_dev,
                                           out_dtype, ldo, st);
            else
                launch_gather_rot<float>(frame_dev, ld, frame_w, frame_h, (const int32_t*)p->tabs.p, (const RotCoef*)p->rot.p, n, out_w, out_h, out_dev,
                                         out_dtype, ldo, st);
        } else if (frame_dtype == HG_U8) {
            launch_gather<uint8_t>(frame_dev, ld, frame_w, (const int32_t*)p->tabs.p, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        } else {
            launch_gather<float>(frame_dev, ld * 4, frame_w, (const int32_t*)p->tabs.p, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        }
        HG_HIP(hipGetLastError());
    });
}

int hg_patcher_extract_keyed_device(hg_patcher* p, uint64_t key, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                                    const double* boxes_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    if (key == 0) return hg_patcher_extract_rotate_device(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, nullptr, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
    return guarded([&] {
        check_args(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo);
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        const int32_t* tabs = nearest_tables(p, key, frame_h, frame_w, boxes_dev, n, out_w, out_h, st);
        if (frame_dtype == HG_U8) launch_gather<uint8_t>(frame_dev, ld, frame_w, tabs, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        else launch_gather<float>(frame_dev, ld * 4, frame_w, tabs, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        HG_HIP(hipGetLastError());
    });
}

int hg_patcher_extract_device(hg_patcher* p, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                              const double* boxes_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo,
                              void* stream) {
    return hg_patcher_extract_rotate_device(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, nullptr, n, out_w, out_h, out_dev, out_dtype,
                                            ldo, stream);
}

int hg_patcher_extract_filter_device(hg_patcher* p, int filter, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                                     const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype,
                                     int64_t ldo, void* stream) {
    return hg::patcher_extract(p, 0, filter, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, delta_angs_dev, n, out_w, out_h, out_dev, out_dtype, ldo,
                               stream);
}

int hg_patcher_extract_filter(hg_patcher* p, int filter, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld, const double* boxes,
                              const double* delta_angs, int64_t n, int out_w, int out_h, void* out, int out_dtype, int64_t ldo) {
    return guarded([&] {
        check_filter(filter, frame_dtype);
        check_args(p, frame, frame_dtype, frame_h, frame_w, ld, boxes, n, out_w, out_h, out, out_dtype, ldo);
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        const size_t fs = hg::dtype_size(frame_dtype), os = hg::dtype_size(out_dtype);
        p->frame.alloc((size_t)frame_h * frame_w * fs);
        HG_HIP(hipMemcpy2D(p->frame.p, (size_t)frame_w * fs, frame, (size_t)ld * fs, (size_t)frame_w * fs, (size_t)frame_h, hipMemcpyHostToDevice));
        p->boxes.upload(boxes, (size_t)n * 4 * 8);
        if (delta_angs) p->angles.upload(delta_angs, (size_t)n * 8);
        const size_t row = (size_t)out_w * out_h;
        p->out.alloc((size_t)n * row * os);
        int rc = hg::patcher_extract(p, 0, filter, p->frame.p, frame_dtype, frame_h, frame_w, frame_w, (const double*)p->boxes.p,
                                     delta_angs ? (const double*)p->angles.p : nullptr, n, out_w, out_h, p->out.p, out_dtype, (int64_t)row, nullptr);
        if (rc != HG_OK) hg::fail(rc, "%s", hg_last_error());
        HG_HIP(hipMemcpy2D(out, (size_t)ldo * os, p->out.p, row * os, row * os, (size_t)n, hipMemcpyDeviceToHost));
    });
}

int hg_patcher_extract_rotate(hg_patcher* p, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld, const double* boxes,
                              const double* delta_angs, int64_t n, int out_w, int out_h, void* out, int out_dtype, int64_t ldo) {
    return hg_patcher_extract_filter(p, HG_FILTER_NEAREST, frame, frame_dtype, frame_h, frame_w, ld, boxes, delta_angs, n, out_w, out_h, out, out_dtype, ldo);
}

int hg_patcher_extract(hg_patcher* p, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld, const double* boxes,
                       int64_t n, int out_w, int out_h, void* out, int out_dtype, int64_t ldo) {
    return hg_patcher_extract_rotate(p, frame, frame_dtype, frame_h, frame_w, ld, boxes, nullptr, n, out_w, out_h, out, out_dtype, ldo);
}

}  // extern "C"

namespace hg {
void*& patcher_resample_state(hg_patcher* p) { return p->resample; }
void*& patcher_normalize_state(hg_patcher* p) { return p->normalize; }
int patcher_device(const hg_patcher* p) { return p->device; }

// NEAREST, unrotated windows from a frame of any format (hg_patcher_extract_format_device; key as for patcher_extract: the cascade's
// prescale passes the key of its whole-frame box, whose tables a grey and a colour frame of one size share)
int patcher_extract_format(hg_patcher* p, uint64_t key, int format, const void* frame_dev, int frame_h, int frame_w, int64_t ld_bytes, const double* boxes_dev,
                           int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    return guarded([&] {
        check_color_frame(format, frame_h, frame_w, ld_bytes);
        check_args(p, frame_dev, HG_U8, frame_h, frame_w, ld_bytes, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo);
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        const int32_t* tabs = nearest_tables(p, key, frame_h, frame_w, boxes_dev, n, out_w, out_h, st);
        launch_gather_format(format, frame_dev, ld_bytes, frame_w, tabs, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        HG_HIP(hipGetLastError());
    });
}

// The single dispatch (hg_common.hpp): every C entry of this file that takes a filter, and the cascade's stage loop, come through here.
// NEAREST goes to the entries it always went to; BILINEAR and BICUBIC share a coordinate table (it holds coordinates, not taps), kept
// per key under the contract of hg_patcher_extract_keyed_device (key != 0: unrotated boxes the caller declares unchanged).
int patcher_extract(hg_patcher* p, uint64_t key, int filter, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                    const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo,
                    void* stream) {
    if (filter == HG_FILTER_NEAREST)
        return key && !delta_angs_dev
                   ? hg_patcher_extract_keyed_device(p, key, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo, stream)
                   : hg_patcher_extract_rotate_device(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, delta_angs_dev, n, out_w, out_h, out_dev, out_dtype,
                                                      ldo, stream);
    return guarded([&] {
        check_filter(filter, frame_dtype);
        check_args(p, frame_dev, frame_dtype, frame_h, frame_w, ld, boxes_dev, n, out_w, out_h, out_dev, out_dtype, ldo);
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        const RotAff* rot = nullptr;
        const FiltEnt* tabs = filter_tables(p, key, frame_h, frame_w, boxes_dev, delta_angs_dev, n, out_w, out_h, st, &rot);
        if (filter == HG_FILTER_BILINEAR)
            launch_filter<HG_FILTER_BILINEAR>((const uint8_t*)frame_dev, ld, frame_w, frame_h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        else
            launch_filter<HG_FILTER_BICUBIC>((const uint8_t*)frame_dev, ld, frame_w, frame_h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st);
        HG_HIP(hipGetLastError());
    });
}

// The sibling of patcher_extract for a stack of same-size grey uint8 frames (hg_common.hpp; hg_patcher_extract_frames_device is this
// with key = 0, tab_n = 0, row_div = 1): the same tables, the same kernels instantiated with a FrameSel.  Every refusal comes before
// the handle or a data pointer is dereferenced and before anything is launched.
int patcher_extract_frames(hg_patcher* p, uint64_t key, int64_t tab_n, int filter, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                           int frame_w, int64_t ld, const double* boxes_dev, const double* delta_angs_dev, const int32_t* row_frame_dev, int row_div, int64_t n,
                           int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    return guarded([&] {
        check_filter(filter, HG_U8);
        if (!p || !frames_dev || !boxes_dev || !row_frame_dev || !out_dev) fail(HG_ERR_ARG, "null pointer");
        if (n_frames < 1) fail(HG_ERR_ARG, "bad frame count %d", n_frames);
        if (frame_h <= 0 || frame_w <= 0 || ld < frame_w) fail(HG_ERR_ARG, "bad frame geometry");
        if (frame_stride < (int64_t)(frame_h - 1) * ld + frame_w)
            fail(HG_ERR_ARG, "frames %lld bytes apart, a frame reaches over %lld", (long long)frame_stride, (long long)((int64_t)(frame_h - 1) * ld + frame_w));
        if (out_dtype != HG_U8 && out_dtype != HG_F32 && out_dtype != HG_F64) fail(HG_ERR_ARG, "bad output dtype");
        if (out_w <= 0 || out_h <= 0 || out_w > 4096 || out_h > 4096) fail(HG_ERR_ARG, "bad sub-image size");
        if (n < 0 || ldo < (int64_t)out_w * out_h || row_div < 1 || tab_n < 0) fail(HG_ERR_ARG, "bad batch geometry");
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        if ((n * (out_w + out_h) + 255) / 256 > 0x7fffffffll) fail(HG_ERR_ARG, "too many boxes");
        const bool repeat = key && tab_n > 0 && tab_n < n && !delta_angs_dev;      // the first tab_n boxes' tables serve every frame's copy of them
        const int64_t n_tab = repeat ? tab_n : n;
        const FrameSel sel{row_frame_dev, frame_stride, n_frames, row_div, n_tab};
        if (filter == HG_FILTER_NEAREST) {
            if (delta_angs_dev) {
                if (frame_w >= 32768 || frame_h >= 32768) fail(HG_ERR_ARG, "rotated windows need a frame smaller than 32768 pixels per side");
                p->tabs.alloc((size_t)n * (out_w + out_h) * 4);
                p->rot.alloc((size_t)n * sizeof(RotCoef));
                hipLaunchKernelGGL(k_extent_tables, (unsigned)((n * (out_w + out_h) + 255) / 256), 256, 0, st, boxes_dev, n, out_w, out_h, frame_w, frame_h,
                                   (int32_t*)p->tabs.p, delta_angs_dev, (RotCoef*)p->rot.p);
                launch_gather_rot<uint8_t>(frames_dev, ld, frame_w, frame_h, (const int32_t*)p->tabs.p, (const RotCoef*)p->rot.p, n, out_w, out_h, out_dev,
                                           out_dtype, ldo, st, sel);
            } else {
                const int32_t* tabs = nearest_tables(p, key, frame_h, frame_w, boxes_dev, n_tab, out_w, out_h, st);
                launch_gather<uint8_t>(frames_dev, ld, frame_w, tabs, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
            }
        } else {
            const RotAff* rot = nullptr;
            const FiltEnt* tabs = filter_tables(p, key, frame_h, frame_w, boxes_dev, delta_angs_dev, n_tab, out_w, out_h, st, &rot);
            if (filter == HG_FILTER_BILINEAR)
                launch_filter<HG_FILTER_BILINEAR>((const uint8_t*)frames_dev, ld, frame_w, frame_h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
            else
                launch_filter<HG_FILTER_BICUBIC>((const uint8_t*)frames_dev, ld, frame_w, frame_h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
        }
        HG_HIP(hipGetLastError());
    });
}
void put_frame_descs(const FrameDesc* host, int n_frames, FrameDesc* dev, hipStream_t st) {
    for (int at = 0; at < n_frames; at += kDescChunk) {
        DescChunk c{};
        const int m = std::min(kDescChunk, n_frames - at);
        memcpy(c.d, host + at, (size_t)m * sizeof(FrameDesc));
        hipLaunchKernelGGL(k_put_descs, 1, kDescChunk, 0, st, c, m, dev + at);
    }
    HG_HIP(hipGetLastError());
}

// The sibling of patcher_extract_frames for a LIST of grey uint8 frames of different sizes (hg_common.hpp, FrameList): the same kernels
// instantiated with a FrameListSel, the tables of k_extent_tables_list / k_filter_tables_list (a table per box, its frame's size per
// box), or, for the concatenated grids of a cascade's first stage (fl.key), the existing table kernels once per DISTINCT grid into the
// list's own call-long buffer.  Every refusal comes before the handle or a data pointer is dereferenced and before anything is launched.
int patcher_extract_frame_list(hg_patcher* p, const FrameList& fl, int filter, const double* boxes_dev, const double* delta_angs_dev,
                               const int32_t* row_frame_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    return guarded([&] {
        check_filter(filter, HG_U8);
        if (!p || !fl.host || !boxes_dev || !row_frame_dev || !out_dev) fail(HG_ERR_ARG, "null pointer");
        if (fl.n_frames < 1 || fl.n_frames > HG_MAX_STACK_FRAMES) fail(HG_ERR_ARG, "%d frames in a list (1..%d)", fl.n_frames, HG_MAX_STACK_FRAMES);
        for (int f = 0; f < fl.n_frames; ++f) {
            const FrameDesc& d = fl.host[f];
            std::string bad = list_frame_refusal(f, d.px, d.h, d.w, d.ld, 1);      // (hg_frame_list.hpp: one text for the patcher and the cascade)
            if (bad.empty() && filter == HG_FILTER_NEAREST && delta_angs_dev) bad = list_rotated_refusal(f, d.w, d.h);
            if (!bad.empty()) fail(HG_ERR_ARG, "%s", bad.c_str());
        }
        if (out_dtype != HG_U8 && out_dtype != HG_F32 && out_dtype != HG_F64) fail(HG_ERR_ARG, "bad output dtype");
        if (out_w <= 0 || out_h <= 0 || out_w > 4096 || out_h > 4096) fail(HG_ERR_ARG, "bad sub-image size");
        if (n < 0 || ldo < (int64_t)out_w * out_h) fail(HG_ERR_ARG, "bad batch geometry");
        if (fl.win_frame_dev && (fl.n_windows < 1 || fl.n_windows > 0x7fffffffll)) fail(HG_ERR_ARG, "bad window count of the list");
        const bool shared = fl.key != 0 && !delta_angs_dev;
        if (shared && (!fl.win_frame_dev || n != fl.n_windows || fl.tab_rows < 1 || fl.tab_rows > n)) fail(HG_ERR_ARG, "bad shared tables of the list");
        if (n == 0) return;
        HG_HIP(hipSetDevice(p->device));
        hipStream_t st = (hipStream_t)stream;
        const int wh = out_w + out_h;
        if ((n * wh + 255) / 256 > 0x7fffffffll) fail(HG_ERR_ARG, "too many boxes");
        const FrameDesc* desc = fl.dev;
        if (!desc) {
            p->list_desc.alloc((size_t)fl.n_frames * sizeof(FrameDesc));
            put_frame_descs(fl.host, fl.n_frames, (FrameDesc*)p->list_desc.p, st);
            desc = (const FrameDesc*)p->list_desc.p;
        }
        const FrameListSel sel{desc, row_frame_dev, fl.win_frame_dev, fl.n_frames, (int32_t)fl.n_windows, shared ? 1 : 0, 0};
        const FrameDesc& d0 = fl.host[0];      // the kernels' own frame arguments: frame 0's (what a box outside the list keeps)
        const bool filtered = filter != HG_FILTER_NEAREST;
        const void* shared_tabs = nullptr;
        if (shared) {
            const size_t ent = filtered ? sizeof(FiltEnt) : 4;
            if (!(p->list_key == fl.key && p->list_rows == fl.tab_rows && p->list_w == out_w && p->list_h == out_h && p->list_filtered == (int)filtered)) {
                const size_t need = (size_t)fl.tab_rows * wh * ent;
                if (p->list_tabs.p && need > p->list_tabs.bytes) HG_HIP(hipStreamSynchronize(st));      // a launch in flight may still read the old buffer
                p->list_tabs.alloc(need);
                p->list_key = 0;      // (until every launch below is enqueued)
                std::vector<char> built((size_t)fl.tab_rows, 0);
                for (int f = 0; f < fl.n_frames; ++f) {
                    const FrameDesc& d = fl.host[f];
                    const int64_t n0 = (f + 1 < fl.n_frames ? fl.host[f + 1].first : fl.n_windows) - d.first;
                    if (d.first < 0 || n0 < 0 || d.tab_row < 0 || d.tab_row + n0 > fl.tab_rows) fail(HG_ERR_ARG, "frame %d of the list: bad table rows", f);
                    if (n0 == 0 || built[(size_t)d.tab_row]) continue;      // (an equal grid earlier in the list: its rows serve this frame too)
                    built[(size_t)d.tab_row] = 1;
                    const unsigned blocks = (unsigned)((n0 * wh + 255) / 256);
                    if (filtered)
                        hipLaunchKernelGGL(k_filter_tables, blocks, 256, 0, st, boxes_dev + (int64_t)d.first * 4, n0, out_w, out_h, d.w, d.h,
                                           (FiltEnt*)p->list_tabs.p + (int64_t)d.tab_row * wh, (const double*)nullptr, (RotAff*)nullptr);
                    else
                        hipLaunchKernelGGL(k_extent_tables, blocks, 256, 0, st, boxes_dev + (int64_t)d.first * 4, n0, out_w, out_h, d.w, d.h,
                                           (int32_t*)p->list_tabs.p + (int64_t)d.tab_row * wh, (const double*)nullptr, (RotCoef*)nullptr);
                }
                HG_HIP(hipGetLastError());
                p->list_key = fl.key; p->list_rows = fl.tab_rows; p->list_w = out_w; p->list_h = out_h; p->list_filtered = (int)filtered;
            }
            shared_tabs = p->list_tabs.p;
        }
        const unsigned tab_blocks = (unsigned)((n * wh + 255) / 256);
        if (!filtered) {
            if (delta_angs_dev) {
                p->tabs.alloc((size_t)n * wh * 4);
                p->rot.alloc((size_t)n * sizeof(RotCoef));
                hipLaunchKernelGGL(k_extent_tables_list, tab_blocks, 256, 0, st, boxes_dev, n, out_w, out_h, (int32_t*)p->tabs.p, delta_angs_dev, (RotCoef*)p->rot.p, sel);
                launch_gather_rot<uint8_t>(d0.px, d0.ld, d0.w, d0.h, (const int32_t*)p->tabs.p, (const RotCoef*)p->rot.p, n, out_w, out_h, out_dev, out_dtype, ldo,
                                           st, sel);
            } else {
                const int32_t* tabs = (const int32_t*)shared_tabs;
                if (!tabs) {
                    p->tabs.alloc((size_t)n * wh * 4);
                    hipLaunchKernelGGL(k_extent_tables_list, tab_blocks, 256, 0, st, boxes_dev, n, out_w, out_h, (int32_t*)p->tabs.p, (const double*)nullptr,
                                       (RotCoef*)nullptr, sel);
                    tabs = (const int32_t*)p->tabs.p;
                }
                launch_gather<uint8_t>(d0.px, d0.ld, d0.w, tabs, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
            }
        } else {
            const FiltEnt* tabs = (const FiltEnt*)shared_tabs;
            const RotAff* rot = nullptr;
            if (!tabs) {
                p->ftabs.alloc((size_t)n * wh * sizeof(FiltEnt));
                if (delta_angs_dev) p->frot.alloc((size_t)n * sizeof(RotAff));
                hipLaunchKernelGGL(k_filter_tables_list, tab_blocks, 256, 0, st, boxes_dev, n, out_w, out_h, (FiltEnt*)p->ftabs.p, delta_angs_dev,
                                   delta_angs_dev ? (RotAff*)p->frot.p : nullptr, sel);
                tabs = (const FiltEnt*)p->ftabs.p;
                if (delta_angs_dev) rot = (const RotAff*)p->frot.p;
            }
            if (filter == HG_FILTER_BILINEAR)
                launch_filter<HG_FILTER_BILINEAR>(d0.px, d0.ld, d0.w, d0.h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
            else
                launch_filter<HG_FILTER_BICUBIC>(d0.px, d0.ld, d0.w, d0.h, tabs, rot, n, out_w, out_h, out_dev, out_dtype, ldo, st, sel);
        }
        HG_HIP(hipGetLastError());
    });
}

// One of the three dispatches above, by the kind of the source (hg_common.hpp)
int patcher_extract_source(hg_patcher* p, const FrameSource& src, uint64_t key, RowFrames rows, int filter, const double* boxes_dev, const double* delta_angs_dev,
                           int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    if (src.kind == FrameSource::ONE)
        return patcher_extract(p, key, filter, src.px, HG_U8, src.h, src.w, src.ld, boxes_dev, delta_angs_dev, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
    if (src.kind == FrameSource::STACK)
        return patcher_extract_frames(p, key, rows.windows ? rows.period : 0, filter, src.px, src.n_frames, src.stride, src.h, src.w, src.ld, boxes_dev,
                                      delta_angs_dev, rows.index_dev, rows.windows ? (int)rows.period : 1, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
    if (!src.list) return guarded([] { fail(HG_ERR_ARG, "null pointer"); });
    FrameList fl = *src.list;
    fl.key = key;      // (the concatenated grids are the first stage's boxes only: no key behind it)
    if (!rows.windows) {      // a frame index per row, a table per box
        fl.win_frame_dev = nullptr;
        fl.n_windows = 0;
        fl.tab_rows = 0;
    }
    return patcher_extract_frame_list(p, fl, filter, boxes_dev, delta_angs_dev, rows.index_dev, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
}
}  // namespace hg

extern "C" int hg_patcher_extract_frame_list_device(hg_patcher* p, int filter, const hg_frame_ref* frames, int n_frames, const double* boxes_dev,
                                                    const double* delta_angs_dev, const int32_t* row_frame_dev, int64_t n, int out_w, int out_h, void* out_dev,
                                                    int out_dtype, int64_t ldo, void* stream) {
    return guarded([&] {
        if (!frames) hg::fail(HG_ERR_ARG, "null pointer");
        if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) hg::fail(HG_ERR_ARG, "%d frames in a list (1..%d)", n_frames, HG_MAX_STACK_FRAMES);
        std::vector<hg::FrameDesc> desc((size_t)n_frames);
        for (int f = 0; f < n_frames; ++f) desc[(size_t)f] = hg::FrameDesc{(const uint8_t*)frames[f].frame_dev, frames[f].ld, frames[f].frame_w, frames[f].frame_h, 0, 0};
        const hg::FrameList fl{desc.data(), nullptr, n_frames, nullptr, 0, 0, 0};
        const int rc = hg::patcher_extract_frame_list(p, fl, filter, boxes_dev, delta_angs_dev, row_frame_dev, n, out_w, out_h, out_dev, out_dtype, ldo, stream);
        if (rc != HG_OK) hg::fail(rc, "%s", hg_last_error());
    });
}

extern "C" int hg_patcher_extract_frames_device(hg_patcher* p, int filter, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w,
                                                int64_t ld, const double* boxes_dev, const double* delta_angs_dev, const int32_t* row_frame_dev, int64_t n,
                                                int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream) {
    return hg::patcher_extract_frames(p, 0, 0, filter, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, boxes_dev, delta_angs_dev, row_frame_dev, 1, n,
                                      out_w, out_h, out_dev, out_dtype, ldo, stream);
}
