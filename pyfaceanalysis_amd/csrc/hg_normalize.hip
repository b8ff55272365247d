// Pose-normalised face crops on the device (include/higsfa.h, "normalize_image"; hg_patcher_normalize_device): what the reference does
// with the purged rows of a frame next (face_analysis.py:983-1013, :1170-1222), per face
//     crop = im.transform((W, H), EXTENT, integer box)            a shift of the frame, 0 outside it; W x H up to about 2 x the frame per axis
//     rot  = crop.rotate(angle, BICUBIC)                          about the crop's centre
//     out  = rot.transform((out_w, out_h), EXTENT, box, BICUBIC)
// The geometry (crop origin and size, Image.rotate's matrix, the box, and the rectangle of rot the cut can read) is computed on the host
// (hg_normalize.cpp: the host's libm, no device trigonometry); here are the pixels.  Neither the crop nor rot is materialised: a tap of
// the rotation reads the VIRTUAL crop — frame[(j + crop_y0) * ld + i + crop_x0] inside the frame, 0 outside — and only the rectangle of
// rot the cut reads is computed.
//   staged       k_norm_rect computes every pixel of a face's rectangle once into per-face scratch (uint8), k_norm_cut<1> cuts from it
//   tap by tap   k_norm_cut<2>: each of the cut's 16 taps computes its rotated pixel where it is used (16 x 16 frame reads per output
//                pixel), no scratch
// Both give the same bytes (the same rot_px either way).  A face is staged while its rectangle holds at most as many pixels as the cut has
// taps, 16 out_w out_h (hg::normalize_stage_limit): beyond that — a face shrunk more than about 4 x per axis — staging computes rotated
// pixels no tap reads.  That bound is work equality, not a measurement; it also caps the scratch at 16 out_w out_h bytes per face.
// Measured on an MI355X (profiles/r15_normalize_times.txt; 16 faces of one shrink factor on a 1000 x 562 frame, 64 x 48 output, device time,
// medians of 30 alternated calls, staged / tap by tap): 2 x 0.030 / 0.062 ms, 3 x 0.032 / 0.060, 4 x — the bound, 49152 rotated pixels
// either way — 0.037 / 0.059, 4.5 x 0.038 / 0.059, 6 x 0.049 / 0.060, 8 x (a rectangle of 3.9 x the taps) 0.065 / 0.063.  So at this size
// the crossover sits near 8 x, not at the bound: tap by tap costs the same at every factor (3072 threads with 16 rotated pixels in a row
// each, sixteen threads computing the same one), staged grows with the rectangle and has a thread per rotated pixel.  The bound stays
// where it is: beyond it the scratch per face would no longer be bounded by the output's size, and a batch of such faces is 0.02 ms apart.
// Every grid and scratch size comes from the host's geoms; no launch is sized by anything read on the device.
// The faces of a STACK of same-size frames (hg_patcher_normalize_frames_device) run the same bodies: k_norm_rect_frames and
// k_norm_cut<…, StackRef, StackFace>, each face reading its own frame; the single frame keeps k_norm_rect and k_norm_cut<…, FrameRef, NormFace>.
// The faces of a LIST of frames of different sizes (hg_patcher_normalize_frame_list_device) run them a third time: k_norm_rect_list and
// k_norm_cut<…, ListRef, ListFace>, each record carrying the frame the host resolved for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "hg_common.hpp"
#include "hg_normalize.hpp"

namespace hg { void set_last_error(const std::string& s); }

#pragma clang fp contract(off)
namespace {
#include "hg_filter_dev.hpp"

enum : int32_t { kModeZero = 0, kModeStaged = 1, kModeTaps = 2 };

// One face as the kernels read it
struct NormFace {
    double m[6];
    double box[4];
    int32_t crop_x0, crop_y0, W, H;
    int32_t rotated, mode;
    int32_t rx0, ry0, rw, rh;      // the rectangle of rot the cut reads
    int64_t scratch_off;           // kModeStaged: where the rectangle lives in the scratch
};

struct FrameRef {
    static constexpr bool kStack = false;
    const uint8_t* p;
    int64_t ld;
    int w, h;
};

// A STACK of same-size frames (hg_patcher_normalize_frames_device): the face record carries the index of its frame, the reference the
// stack's frame_stride in bytes — any value >= (h - 1) ld + w, not necessarily a multiple of ld.  The kernels below are instantiated
// once for (FrameRef, NormFace), the single frame with the records and the code it has always had, and once for (StackRef, StackFace).
struct StackFace {
    NormFace f;
    int32_t frame, pad;
};

struct StackRef {
    static constexpr bool kStack = true;
    const uint8_t* p;              // frame 0
    int64_t ld, frame_stride;
    int w, h, n_frames;
};

// A LIST of frames of different sizes (hg_patcher_normalize_frame_list_device): the face record carries its RESOLVED frame — base
// pointer, row stride, size — which the host fills from frames[face_frame[i]]; p == nullptr for a refused face and for one whose index
// lies outside the list.  No table of frames on the device and no index to check there: the one upload of the records is all a call
// sends.  The third instantiation, (ListRef, ListFace); the reference itself carries nothing the kernels read.
struct ListFace {
    NormFace f;
    const uint8_t* p;
    int64_t ld;
    int32_t w, h;
};

struct ListRef {
    static constexpr bool kStack = true;      // as for the stack: a face without a frame (p == nullptr) is the all-zero image
    int32_t n_frames;                         // (not read on the device)
};

__device__ __forceinline__ const NormFace& rec(const NormFace& f) { return f; }
__device__ __forceinline__ const NormFace& rec(const StackFace& s) { return s.f; }
__device__ __forceinline__ const NormFace& rec(const ListFace& s) { return s.f; }
__device__ __forceinline__ FrameRef frame_of(const ListRef&, const ListFace& s) { return FrameRef{s.p, s.ld, s.w, s.h}; }
__device__ __forceinline__ FrameRef frame_of(const FrameRef& fr, const NormFace&) { return fr; }
// the face's own frame; p == nullptr for an index outside [0, n_frames): no address is formed from such an index (the host has made
// such a face kModeZero already; the kernels do not rely on it)
__device__ __forceinline__ FrameRef frame_of(const StackRef& sr, const StackFace& s) {
    const bool in = s.frame >= 0 && s.frame < sr.n_frames;
    return FrameRef{in ? sr.p + (int64_t)s.frame * sr.frame_stride : nullptr, sr.ld, sr.w, sr.h};
}

// pixel (xc, yc) of the virtual crop
__device__ __forceinline__ double crop_px(const FrameRef& fr, const NormFace& f, int xc, int yc) {
    const int fx = xc + f.crop_x0, fy = yc + f.crop_y0;      // (|crop origin| and the crop size are below 2^26: no overflow)
    const bool in = fx >= 0 && fx < fr.w && fy >= 0 && fy < fr.h;
    return in ? (double)fr.p[(int64_t)fy * fr.ld + fx] : 0.0;
}

// pixel (xr, yr) of crop.rotate(angle, BICUBIC): affine_transform with the matrix of the geom, then the filter on the virtual crop
__device__ __forceinline__ uint8_t rot_px(const FrameRef& fr, const NormFace& f, int xr, int yr) {
    if (!f.rotated) return (uint8_t)crop_px(fr, f, xr, yr);      // Image.rotate's copy at angle % 360 == 0
    const double xin = d_add((double)xr, 0.5), yin = d_add((double)yr, 0.5);
    const FiltEnt ex = filter_coord(d_add(d_add(d_mul(f.m[0], xin), d_mul(f.m[1], yin)), f.m[2]), f.W);
    const FiltEnt ey = filter_coord(d_add(d_add(d_mul(f.m[3], xin), d_mul(f.m[4], yin)), f.m[5]), f.H);
    if (ex.i == kFiltOutside || ey.i == kFiltOutside) return 0;
    return filter_sample<HG_FILTER_BICUBIC>([&](int xc, int yc) { return crop_px(fr, f, xc, yc); }, ex.i, ex.d, ey.i, ey.d, f.W, f.H);
}

// a (i + 0.5) + lo with a = (hi - lo) / n: the EXTENT cut's source coordinate of output index i (the zero product of the other axis adds nothing)
__device__ __forceinline__ FiltEnt cut_entry(double lo, double hi, int n, int i, int lim) {
    const double a = d_div(d_sub(hi, lo), (double)n);
    return filter_coord(d_add(d_mul(a, d_add((double)i, 0.5)), lo), lim);
}

// Pass A: a thread per pixel of a staged face's rectangle; blockIdx.y walks the faces, blockIdx.x the rectangle in chunks of 256 pixels
// (the grid covers the largest rectangle of the call: the workgroups beyond a smaller face's rectangle leave at once).
template <typename Ref, typename Face>
__device__ __forceinline__ void norm_rect(const Ref& ref, const Face* __restrict__ faces, int64_t n, uint8_t* __restrict__ scratch) {
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        const Face F = faces[b];
        const NormFace& f = rec(F);
        if (f.mode != kModeStaged) continue;
        const FrameRef fr = frame_of(ref, F);
        if constexpr (Ref::kStack)
            if (!fr.p) continue;
        const int64_t np = (int64_t)f.rw * f.rh;
        for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < np; idx += (int64_t)gridDim.x * 256) {
            const int py = (int)(idx / f.rw), px = (int)(idx - (int64_t)py * f.rw);
            scratch[f.scratch_off + idx] = rot_px(fr, f, f.rx0 + px, f.ry0 + py);
        }
    }
}
__global__ void __launch_bounds__(256) k_norm_rect(FrameRef fr, const NormFace* __restrict__ faces, int64_t n, uint8_t* __restrict__ scratch) {
    norm_rect(fr, faces, n, scratch);
}
__global__ void __launch_bounds__(256) k_norm_rect_frames(StackRef sr, const StackFace* __restrict__ faces, int64_t n, uint8_t* __restrict__ scratch) {
    norm_rect(sr, faces, n, scratch);
}
__global__ void __launch_bounds__(256) k_norm_rect_list(ListRef lr, const ListFace* __restrict__ faces, int64_t n, uint8_t* __restrict__ scratch) {
    norm_rect(lr, faces, n, scratch);
}

// Pass B: the EXTENT / BICUBIC cut, a 16 x 16 tile of output pixels per workgroup.  MODE kModeStaged also writes the all-zero image of
// a refused face (kModeZero); MODE kModeTaps takes the faces left to it.  A face of the other mode costs a workgroup one record read.
constexpr int kTile = 16;
template <int MODE, typename Ref, typename Face>
__global__ void __launch_bounds__(256) k_norm_cut(Ref ref, const Face* __restrict__ faces, int64_t n, const uint8_t* __restrict__ scratch, int out_w,
                                                  int out_h, uint8_t* __restrict__ out, int64_t ldo, int tiles_x) {
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int ox = (int)(blockIdx.x % tiles_x) * kTile + tx, oy = (int)(blockIdx.x / tiles_x) * kTile + ty;
    if (ox >= out_w || oy >= out_h) return;
    for (int64_t b = blockIdx.y; b < n; b += gridDim.y) {
        const Face F = faces[b];
        const NormFace& f = rec(F);
        if (MODE == kModeStaged ? f.mode == kModeTaps : f.mode != kModeTaps) continue;
        const FrameRef fr = frame_of(ref, F);
        bool zero = f.mode == kModeZero;
        if constexpr (Ref::kStack) zero = zero || !fr.p;      // a face whose frame lies outside the stack: the all-zero image
        uint8_t v = 0;
        if (!zero) {
            const FiltEnt ex = cut_entry(f.box[0], f.box[2], out_w, ox, f.W), ey = cut_entry(f.box[1], f.box[3], out_h, oy, f.H);
            if (ex.i != kFiltOutside && ey.i != kFiltOutside) {
                if constexpr (MODE == kModeStaged) {
                    // (the clamps change nothing for a geom of the host unit: its rectangle holds every tap; no hand-made one can make a read leave the scratch)
                    const uint8_t* r = scratch + f.scratch_off;
                    auto tap = [&](int xc, int yc) {
                        const int px = min(max(xc - f.rx0, 0), f.rw - 1), py = min(max(yc - f.ry0, 0), f.rh - 1);
                        return (double)r[(int64_t)py * f.rw + px];
                    };
                    v = filter_sample<HG_FILTER_BICUBIC>(tap, ex.i, ex.d, ey.i, ey.d, f.W, f.H);
                } else {
                    v = filter_sample<HG_FILTER_BICUBIC>([&](int xc, int yc) { return (double)rot_px(fr, f, xc, yc); }, ex.i, ex.d, ey.i, ey.d, f.W, f.H);
                }
            }
        }
        out[b * ldo + (int64_t)oy * out_w + ox] = v;
    }
}

// ---- the patcher's normalisation state ------------------------------------------------------------------------------------------
// The face records travel through pinned host memory: a ring of slots, each with the event of its last upload, so that a call never
// overwrites records a copy still reads and — four slots deep — does not wait for the stream in steady state either.
constexpr int kSlots = 4;
struct NormState {
    struct Slot {
        void* host = nullptr;      // NormFace or StackFace records
        size_t cap = 0;            // bytes
        hipEvent_t copied = nullptr;
        bool pending = false;
    } slot[kSlots];
    int next = 0;
    hg::DevBuf faces, scratch;
    ~NormState() {
        for (auto& s : slot) {
            if (s.pending) (void)hipEventSynchronize(s.copied);
            if (s.copied) (void)hipEventDestroy(s.copied);
            if (s.host) (void)hipHostFree(s.host);
        }
    }
};

NormState* state_of(hg_patcher* p) {
    void*& s = hg::patcher_normalize_state(p);
    if (!s) s = new NormState();
    return (NormState*)s;
}

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

constexpr int64_t kForcedStageLimit = (int64_t)1 << 26;      // pixels of one rectangle when bit 0 of flags forces staging

}  // namespace

namespace hg {
void normalize_state_free(void* state) { delete (NormState*)state; }
}  // namespace hg


namespace {

// frame: the face's index, checked, or -1 for a face without a frame; list: the list's descriptors (nullptr elsewhere)
inline void set_frame(NormFace&, int32_t, const hg_frame_ref*) {}
inline void set_frame(StackFace& s, int32_t frame, const hg_frame_ref*) { s.frame = frame; }
inline void set_frame(ListFace& s, int32_t frame, const hg_frame_ref* list) {
    if (frame < 0) return;      // (the zeroed record: a null frame)
    const hg_frame_ref& F = list[frame];
    s.p = (const uint8_t*)F.frame_dev;
    s.ld = F.ld;
    s.w = F.frame_w;
    s.h = F.frame_h;
}
inline NormFace& rec_host(NormFace& f) { return f; }
inline NormFace& rec_host(StackFace& s) { return s.f; }
inline NormFace& rec_host(ListFace& s) { return s.f; }

// All three entries behind their argument checks, n > 0.  face_frame / n_frames: the stack's or the list's (nullptr / 0 for the single
// frame); list: the list's descriptors (host; nullptr elsewhere).  A face whose frame index lies outside [0, n_frames) is a refused face
// here already — kModeZero, no scratch, no part in any grid size.
template <typename Ref, typename Face>
void normalize_run(hg_patcher* p, int flags, const Ref& ref, const hg_norm_geom* geoms_host, const int32_t* face_frame, int n_frames, int64_t n, int out_w, int out_h,
                   uint8_t* out_dev, int64_t ldo, void* stream, const hg_frame_ref* list = nullptr) {
    if (n > (1 << 24)) hg::fail(HG_ERR_ARG, "normalize: more than 2^24 faces in one call");
    auto live = [&](int64_t i) {
        const hg_norm_geom& g = geoms_host[i];
        return g.status == 0 && g.rect[2] > 0 && (!face_frame || (face_frame[i] >= 0 && face_frame[i] < n_frames));
    };
    // the path of every face and the scratch it needs, from the geoms alone
    const int64_t limit = hg::normalize_stage_limit(out_w, out_h);
    int64_t scratch_bytes = 0, max_rect = 0, n_taps = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!live(i)) continue;
        const hg_norm_geom& g = geoms_host[i];
        const int64_t np = (int64_t)g.rect[2] * g.rect[3];
        const bool staged = (flags & 1) ? true : (flags & 2) ? false : np <= limit;
        if (!staged) {
            ++n_taps;
            continue;
        }
        if ((flags & 1) && np > kForcedStageLimit) hg::fail(HG_ERR_ARG, "normalize: forced staging of a rectangle of %lld pixels (at most 2^26)", (long long)np);
        scratch_bytes += (np + 15) & ~(int64_t)15;
        max_rect = std::max(max_rect, np);
    }
    HG_HIP(hipSetDevice(hg::patcher_device(p)));
    hipStream_t st = (hipStream_t)stream;
    NormState* S = state_of(p);
    NormState::Slot& slot = S->slot[S->next];
    S->next = (S->next + 1) % kSlots;
    if (slot.pending) {
        HG_HIP(hipEventSynchronize(slot.copied));      // the upload of four calls ago
        slot.pending = false;
    }
    if (!slot.copied) HG_HIP(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
    const size_t bytes = (size_t)n * sizeof(Face);
    if (bytes > slot.cap) {
        if (slot.host) HG_HIP(hipHostFree(slot.host));
        slot.host = nullptr;
        slot.cap = 0;
        const size_t cap = std::max<size_t>((size_t)n, 64) * sizeof(Face);
        HG_HIP(hipHostMalloc(&slot.host, cap, hipHostMallocDefault));
        slot.cap = cap;
    }
    Face* host = (Face*)slot.host;
    int64_t off = 0;
    for (int64_t i = 0; i < n; ++i) {
        const hg_norm_geom& g = geoms_host[i];
        Face F{};
        NormFace& f = rec_host(F);
        if (live(i)) {
            for (int k = 0; k < 6; ++k) f.m[k] = g.m[k];
            for (int k = 0; k < 4; ++k) f.box[k] = g.box[k];
            f.crop_x0 = g.crop_x0; f.crop_y0 = g.crop_y0; f.W = g.W; f.H = g.H;
            f.rotated = g.rotated ? 1 : 0;
            f.rx0 = g.rect[0]; f.ry0 = g.rect[1]; f.rw = g.rect[2]; f.rh = g.rect[3];
            const int64_t np = (int64_t)f.rw * f.rh;
            const bool staged = (flags & 1) ? true : (flags & 2) ? false : np <= limit;
            f.mode = staged ? kModeStaged : kModeTaps;
            if (staged) {
                f.scratch_off = off;
                off += (np + 15) & ~(int64_t)15;
            }
            if (face_frame) set_frame(F, face_frame[i], list);
        } else if (face_frame) {
            set_frame(F, -1, list);
        }      // kModeZero — a refused face, one none of whose output pixels is inside rot, or one whose frame is outside the stack / list
        host[i] = F;
    }
    if (S->faces.p && bytes > S->faces.bytes) HG_HIP(hipStreamSynchronize(st));      // a launch in flight may still read the old buffer
    S->faces.alloc(std::max<size_t>((size_t)n, 64) * sizeof(Face));
    if (S->scratch.p && (size_t)scratch_bytes > S->scratch.bytes) HG_HIP(hipStreamSynchronize(st));
    S->scratch.alloc((size_t)scratch_bytes);
    HG_HIP(hipMemcpyAsync(S->faces.p, host, bytes, hipMemcpyHostToDevice, st));
    HG_HIP(hipEventRecord(slot.copied, st));
    slot.pending = true;
    const Face* faces = (const Face*)S->faces.p;
    const unsigned ny = (unsigned)std::min<int64_t>(n, 65535);
    if (max_rect > 0) {
        const dim3 grid((unsigned)((max_rect + 255) / 256), ny);      // <= 2^20 chunks (16 * 4096 * 4096 pixels; forced: kForcedStageLimit)
        if constexpr (std::is_same_v<Ref, ListRef>) hipLaunchKernelGGL(k_norm_rect_list, grid, 256, 0, st, ref, faces, n, (uint8_t*)S->scratch.p);
        else if constexpr (Ref::kStack) hipLaunchKernelGGL(k_norm_rect_frames, grid, 256, 0, st, ref, faces, n, (uint8_t*)S->scratch.p);
        else hipLaunchKernelGGL(k_norm_rect, grid, 256, 0, st, ref, faces, n, (uint8_t*)S->scratch.p);
    }
    const int tiles_x = (out_w + kTile - 1) / kTile, tiles_y = (out_h + kTile - 1) / kTile;      // <= 256 each
    const dim3 grid((unsigned)(tiles_x * tiles_y), ny);
    if (n_taps < n)
        hipLaunchKernelGGL((k_norm_cut<kModeStaged, Ref, Face>), grid, 256, 0, st, ref, faces, n, (const uint8_t*)S->scratch.p, out_w, out_h, out_dev, ldo, tiles_x);
    if (n_taps > 0)
        hipLaunchKernelGGL((k_norm_cut<kModeTaps, Ref, Face>), grid, 256, 0, st, ref, faces, n, (const uint8_t*)nullptr, out_w, out_h, out_dev, ldo, tiles_x);
    HG_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int hg_patcher_normalize_device(hg_patcher* p, int flags, const uint8_t* frame_dev, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms_host,
                                int64_t n, int out_w, int out_h, uint8_t* out_dev, int64_t ldo, void* stream) {
    return guarded([&] {
        if (!p) hg::fail(HG_ERR_ARG, "null patcher handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "normalize: bad flags %d (1: staged, 2: tap by tap)", flags);
        if (const char* why = hg::normalize_check(frame_dev, frame_h, frame_w, ld, geoms_host, n, out_w, out_h, out_dev, ldo)) hg::fail(HG_ERR_ARG, "%s", why);
        if (n == 0) return;
        normalize_run<FrameRef, NormFace>(p, flags, FrameRef{frame_dev, ld, frame_w, frame_h}, geoms_host, nullptr, 0, n, out_w, out_h, out_dev, ldo, stream);
    });
}

int hg_patcher_normalize_frames_device(hg_patcher* p, int flags, const uint8_t* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld,
                                       const hg_norm_geom* geoms_host, const int32_t* face_frame_host, int64_t n, int out_w, int out_h, uint8_t* out_dev, int64_t ldo,
                                       void* stream) {
    return guarded([&] {
        if (!p) hg::fail(HG_ERR_ARG, "null patcher handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "normalize: bad flags %d (1: staged, 2: tap by tap)", flags);
        if (const char* why = hg::normalize_frames_check(frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, geoms_host, face_frame_host, n, out_w, out_h, out_dev, ldo))
            hg::fail(HG_ERR_ARG, "%s", why);
        if (n == 0) return;
        normalize_run<StackRef, StackFace>(p, flags, StackRef{frames_dev, ld, frame_stride, frame_w, frame_h, n_frames}, geoms_host, face_frame_host, n_frames, n, out_w,
                                           out_h, out_dev, ldo, stream);
    });
}

int hg_patcher_normalize_frame_list_device(hg_patcher* p, int flags, const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms_host,
                                           const int32_t* face_frame_host, int64_t n, int out_w, int out_h, uint8_t* out_dev, int64_t ldo, void* stream) {
    return guarded([&] {
        if (!p) hg::fail(HG_ERR_ARG, "null patcher handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "normalize: bad flags %d (1: staged, 2: tap by tap)", flags);
        const std::string why = hg::normalize_frame_list_check(frames, n_frames, geoms_host, face_frame_host, n, out_w, out_h, out_dev, ldo);
        if (!why.empty()) hg::fail(HG_ERR_ARG, "%s", why.c_str());
        if (n == 0) return;
        normalize_run<ListRef, ListFace>(p, flags, ListRef{n_frames}, geoms_host, face_frame_host, n_frames, n, out_w, out_h, out_dev, ldo, stream, frames);
    });
}

}  // extern "C"
