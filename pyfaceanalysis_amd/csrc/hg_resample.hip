// PIL's Image.resize((w, h), filter) on the device (include/higsfa.h, hg_patcher_resize_device): the antialiased prescale.
//
// The coefficient tables of an axis come from the host unit (hg_resample.cpp: Pillow's doubles, the host's libm) and are uploaded once
// per (in, out, filter); everything here is Pillow's integer arithmetic: out = clip8((2^21 + sum in[xmin + x] k[x]) >> 22) in int32,
// horizontal pass first, a uint8 image between the passes.  An "element" below is a byte of the images the passes see: a pixel for grey
// output (a colour source is converted per pixel READ — convert("L") first, then the passes), a band of a pixel for colour output (band
// by band with the same tables, so the vertical pass does not need to know about bands at all).
//
// Two shapes of the same arithmetic:
//   general   k_resample_h over the source rows the vertical pass reads (bounds_v[0].xmin .. last row's xmin + xmax) into the patcher's
//             intermediate image, then k_resample_v.  An axis that keeps its size gets no pass: one launch, straight into dst.
//   fused     one launch; a workgroup owns a 64 x 16 tile of output pixels, runs the horizontal pass for the source rows its tile needs
//             into LDS (uint8, 64 bytes a row), then filters vertically from LDS.  Neighbouring tiles repeat the horizontal pass of the
//             rows they share (the filter's support: about 4 of 35 rows for BILINEAR at 1920 x 1080 -> 1000 x 562, 12 of 43 for LANCZOS)
//             and save the intermediate's round trip and a launch.  Eligible when both axes change and every tile needs at most
//             kFusedRows rows (16 KB).  Which sources and filters take it by default is kFusedDefault below, set from the A/B in
//             profiles/r12_prescale_filters.txt; flags bit 0 forces the two launches, bit 1 the fused kernel where it is eligible.
// Four output elements per thread, one 32-bit store where dst rows are 4-aligned, byte stores otherwise; sources are read pixel by pixel
// (or four grey bytes that lie inside the row as one unaligned load): no load touches a byte outside [row start, row start + w * bpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_common.hpp"
#include "hg_frame_format.hpp"
#include "hg_resample.hpp"

namespace hg { void set_last_error(const std::string& s); }

namespace {

constexpr int kBits = 22;                 // Pillow's PRECISION_BITS for 8-bit images
constexpr int kTileW = 64, kTileH = 16;   // the fused kernel's output tile: 256 threads x 4 elements
constexpr int kFusedRows = 256;           // intermediate rows a tile may need: kFusedRows * kTileW bytes = 16 KB of LDS
// The default path of an eligible call: [source kind][filter code], source kinds {grey source, colour source with grey output, colour
// output}, filter codes PIL's (0 NEAREST: no tables, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING).  True where one launch
// measured faster than two at 1920 x 1080 -> 1000 x 562 with warm tables, in both runs of profiles/r12_prescale_filters.txt: the wider
// filters everywhere (BICUBIC 0.024 against 0.028 ms and LANCZOS 0.029 against 0.036 on a grey frame), the narrow ones only where
// the source is colour (their horizontal pass then converts every pixel it reads, and the intermediate's round trip weighs more).
constexpr bool kFusedDefault[3][6] = {{false, true, false, true, false, false},
                                      {false, true, true, true, false, true},
                                      {false, true, true, true, true, true}};
constexpr int kSlots = 8;                 // axes whose tables a patcher keeps

// how a kernel reads its source: BPP bytes per pixel; GRAY: an element is a pixel's "L" value, else an element is one byte of the row
template <int BPP_, bool BGR_, bool GRAY_>
struct Mode {
    static constexpr int BPP = BPP_;
    static constexpr bool BGR = BGR_, GRAY = GRAY_;
    static constexpr int C = GRAY_ ? 1 : BPP_;      // elements per pixel
};

// element (pixel px, band) of a source row
template <typename M>
__device__ __forceinline__ uint32_t src_at(const uint8_t* __restrict__ row, int px, int band) {
    if constexpr (!M::GRAY) {
        return row[(int64_t)px * M::BPP + band];
    } else if constexpr (M::BPP == 1) {
        return row[px];
    } else if constexpr (M::BPP == 4) {      // the pixel's own four bytes as one load
        uint32_t q;
        __builtin_memcpy(&q, row + (int64_t)px * 4, 4);
        return hg::rgb_to_gray((q >> (M::BGR ? 16 : 0)) & 0xffu, (q >> 8) & 0xffu, (q >> (M::BGR ? 0 : 16)) & 0xffu);
    } else {
        const uint8_t* p = row + (int64_t)px * 3;
        return hg::rgb_to_gray(p[M::BGR ? 2 : 0], p[1], p[M::BGR ? 0 : 2]);
    }
}

// elements e0 .. e0 + 3 of a source row of n elements (0 for those past the row's end)
template <typename M>
__device__ __forceinline__ void load4(const uint8_t* __restrict__ row, int e0, int n, uint32_t v[4]) {
    if constexpr (M::BPP == 1 || !M::GRAY) {
        if (e0 + 4 <= n) {
            uint32_t q;
            __builtin_memcpy(&q, row + e0, 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (q >> (8 * j)) & 0xffu;
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = e0 + j < n ? (uint32_t)row[e0 + j] : 0u;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = e0 + j < n ? src_at<M>(row, e0 + j, 0) : 0u;
    }
}

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {      // unsigned sums: Pillow's int arithmetic with wrap-around defined
    const int32_t v = (int32_t)acc >> kBits;
    return (uint32_t)min(max(v, 0), 255);
}

// output element e of the horizontal pass over one source row
template <typename M>
__device__ __forceinline__ uint32_t h_element(const uint8_t* __restrict__ row, int e, const int32_t* __restrict__ bounds, const int32_t* __restrict__ k, int ksize) {
    const int xx = e / M::C, band = e - xx * M::C;
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const int32_t* kk = k + (int64_t)xx * ksize;
    uint32_t acc = 1u << (kBits - 1);
    for (int x = 0; x < xmax; ++x) acc += src_at<M>(row, xmin + x, band) * (uint32_t)kk[x];
    return clip8(acc);
}

__device__ __forceinline__ void store4(uint8_t* __restrict__ d, int e0, int n, const uint32_t v[4], int packed) {
    if (packed && e0 + 4 <= n) {
        *(uint32_t*)d = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) d[j] = (uint8_t)v[j];
    }
}

// The horizontal pass: source rows y_first .. y_first + n_rows - 1 -> dst rows 0 .. n_rows - 1 of n = out_w * C elements.
template <typename M>
__global__ void __launch_bounds__(256) k_resample_h(const uint8_t* __restrict__ src, int64_t ld_bytes, int y_first, int n_rows, const int32_t* __restrict__ bounds,
                                                     const int32_t* __restrict__ k, int ksize, int n, uint8_t* __restrict__ dst, int64_t dst_ld, int packed) {
    const int64_t e64 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e64 >= n) return;
    const int e0 = (int)e64;
    for (int64_t r = (int64_t)blockIdx.y * blockDim.y + threadIdx.y; r < n_rows; r += (int64_t)gridDim.y * blockDim.y) {
        const uint8_t* row = src + (y_first + r) * ld_bytes;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) v[j] = h_element<M>(row, e0 + j, bounds, k, ksize);
        store4(dst + r * dst_ld + e0, e0, n, v, packed);
    }
}

// The vertical pass over rows of n elements: src row 0 is row `first` of the image the bounds index.
template <typename M>
__global__ void __launch_bounds__(256) k_resample_v(const uint8_t* __restrict__ src, int64_t ld_bytes, int first, const int32_t* __restrict__ bounds,
                                                     const int32_t* __restrict__ k, int ksize, int n, int out_h, uint8_t* __restrict__ dst, int64_t dst_ld, int packed) {
    const int64_t e64 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e64 >= n) return;
    const int e0 = (int)e64;
    for (int64_t yy = (int64_t)blockIdx.y * blockDim.y + threadIdx.y; yy < out_h; yy += (int64_t)gridDim.y * blockDim.y) {
        const int ymin = bounds[2 * yy] - first, ymax = bounds[2 * yy + 1];
        const int32_t* kk = k + yy * ksize;
        uint32_t acc[4] = {1u << (kBits - 1), 1u << (kBits - 1), 1u << (kBits - 1), 1u << (kBits - 1)};
        for (int y = 0; y < ymax; ++y) {
            uint32_t v[4];
            load4<M>(src + (int64_t)(ymin + y) * ld_bytes, e0, n, v);
            const uint32_t c = (uint32_t)kk[y];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[j] * c;
        }
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = clip8(acc[j]);
        store4(dst + yy * dst_ld + e0, e0, n, v, packed);
    }
}

// Both passes in one launch: tile (blockIdx.x, blockIdx.y) of kTileW x kTileH output elements.  The launcher guarantees that every tile
// needs at most kFusedRows intermediate rows.
template <typename M>
__global__ void __launch_bounds__(256) k_resample_fused(const uint8_t* __restrict__ src, int64_t ld_bytes, const int32_t* __restrict__ bounds_h,
                                                         const int32_t* __restrict__ k_h, int ksize_h, const int32_t* __restrict__ bounds_v,
                                                         const int32_t* __restrict__ k_v, int ksize_v, int n, int out_h, uint8_t* __restrict__ dst,
                                                         int64_t dst_ld, int packed) {
    __shared__ __attribute__((aligned(16))) uint8_t mid[kFusedRows * kTileW];
    const int e_base = blockIdx.x * kTileW, yy_base = blockIdx.y * kTileH;
    const int yy_last = min(yy_base + kTileH, out_h) - 1;
    const int y0 = bounds_v[2 * yy_base];
    const int rows = min(bounds_v[2 * yy_last] + bounds_v[2 * yy_last + 1] - y0, kFusedRows);
    const int tw = min(kTileW, n - e_base);
    for (int idx = threadIdx.x; idx < rows * kTileW; idx += 256) {
        const int r = idx / kTileW, c = idx - r * kTileW;
        if (c < tw) mid[idx] = (uint8_t)h_element<M>(src + (int64_t)(y0 + r) * ld_bytes, e_base + c, bounds_h, k_h, ksize_h);
    }
    __syncthreads();
    const int ty = threadIdx.x / (kTileW / 4), c0 = (threadIdx.x - ty * (kTileW / 4)) * 4;
    const int yy = yy_base + ty;
    if (yy >= out_h || c0 >= tw) return;
    const int ymin = bounds_v[2 * yy] - y0, ymax = min(bounds_v[2 * yy + 1], rows - ymin);
    const int32_t* kk = k_v + (int64_t)yy * ksize_v;
    uint32_t acc[4] = {1u << (kBits - 1), 1u << (kBits - 1), 1u << (kBits - 1), 1u << (kBits - 1)};
    for (int y = 0; y < ymax; ++y) {
        const uint32_t q = *(const uint32_t*)&mid[(ymin + y) * kTileW + c0];      // (columns past the tile's width: never stored)
        const uint32_t c = (uint32_t)kk[y];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += ((q >> (8 * j)) & 0xffu) * c;
    }
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = clip8(acc[j]);
    const int e0 = e_base + c0;
    store4(dst + (int64_t)yy * dst_ld + e0, e0, n, v, packed);
}

// ---- the patcher's resize state ---------------------------------------------------------------------------------------------
struct AxisEntry {
    hg::ResampleAxis host;      // kept: the async upload reads these vectors, and the fused choice reads the bounds
    hg::DevBuf dev;             // bounds (2 * out int32), then k (out * ksize int32)
    int max_tile_rows = 0;      // most intermediate rows a kTileH-row tile of this axis (as the vertical one) needs
    bool live = false;
    uint64_t used = 0;          // the state's clock at the entry's last use: the least recently used entry is the one replaced
    const int32_t* bounds() const { return (const int32_t*)dev.p; }
    const int32_t* k() const { return (const int32_t*)dev.p + (size_t)host.out * 2; }
};

struct ResampleState {
    AxisEntry ent[kSlots];
    uint64_t clock = 0;
    hg::DevBuf mid;             // the intermediate image of the two-launch path
    hg::DevBuf box;             // NEAREST: the whole-frame box of (box_w, box_h)
    int box_w = 0, box_h = 0;
};

ResampleState* state_of(hg_patcher* p) {
    void*& s = hg::patcher_resample_state(p);
    if (!s) s = new ResampleState();
    return (ResampleState*)s;
}

// The tables of (in, out, filter) on the device: found, or built on the host and uploaded in stream order into the least recently used
// entry.  `pinned`: an entry this call already holds.  A replaced entry first waits for the stream: a launch may still read its tables,
// an upload its host vectors.
AxisEntry* axis_of(ResampleState* S, int in, int out, int filter, const AxisEntry* pinned, hipStream_t st) {
    for (auto& e : S->ent)
        if (e.live && e.host.in == in && e.host.out == out && e.host.filter == filter) {
            e.used = ++S->clock;
            return &e;
        }
    hg::ResampleAxis ax;
    if (const char* why = hg::resample_axis(in, out, filter, ax)) hg::fail(HG_ERR_ARG, "%s", why);
    AxisEntry* e = nullptr;
    for (auto& c : S->ent)
        if (&c != pinned && (!e || (!c.live && e->live) || (c.live == e->live && c.used < e->used))) e = &c;
    if (e->live) HG_HIP(hipStreamSynchronize(st));
    e->live = false;
    e->host = std::move(ax);
    e->dev.alloc(e->host.bytes());
    const size_t nb = e->host.bounds.size() * 4, nk = e->host.k.size() * 4;
    HG_HIP(hipMemcpyAsync(e->dev.p, e->host.bounds.data(), nb, hipMemcpyHostToDevice, st));
    HG_HIP(hipMemcpyAsync((char*)e->dev.p + nb, e->host.k.data(), nk, hipMemcpyHostToDevice, st));
    int most = 0;
    for (int y = 0; y < out; y += kTileH) {
        const int last = std::min(y + kTileH, out) - 1;
        most = std::max(most, e->host.bounds[(size_t)last * 2] + e->host.bounds[(size_t)last * 2 + 1] - e->host.bounds[(size_t)y * 2]);
    }
    e->max_tile_rows = most;
    e->used = ++S->clock;
    e->live = true;
    return e;
}

template <typename F>
void by_mode(int format, bool gray, F&& f) {
    if (!gray) {
        if (hg::frame_bpp(format) == 3) f(Mode<3, false, false>{});
        else f(Mode<4, false, false>{});
        return;
    }
    switch (format) {
        case HG_FRAME_L: f(Mode<1, false, true>{}); break;
        case HG_FRAME_RGB: f(Mode<3, false, true>{}); break;
        case HG_FRAME_BGR: f(Mode<3, true, true>{}); break;
        case HG_FRAME_RGBA: f(Mode<4, false, true>{}); break;
        default: f(Mode<4, true, true>{}); break;
    }
}

// a row of n elements, four per thread: threads per row and rows per workgroup, and the grid over (row chunks, rows)
void shape_of(int n, int64_t rows, dim3& thr, dim3& grid) {
    const int n4 = (n + 3) / 4;
    const unsigned tx = n4 > 64 ? 256 : n4 > 32 ? 64 : 32;
    thr = dim3(tx, 256 / tx);
    grid = dim3((unsigned)((n4 + tx - 1) / tx), (unsigned)std::min<int64_t>((rows + thr.y - 1) / thr.y, 65535));
}

int is_packed(const void* dst, int64_t ld) { return ((uintptr_t)dst & 3) == 0 && (ld & 3) == 0 ? 1 : 0; }

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

// NEAREST: the whole-frame gather the prescale has always used, under a key of its own (the keyed table is found by the key AND the two
// sizes, and the whole-frame box depends on the sizes alone).  A pitched destination is filled through the intermediate image.
void resize_nearest(hg_patcher* p, ResampleState* S, const void* src, int format, int h, int w, int64_t ld_bytes, void* dst, int out_h, int out_w,
                    int64_t dst_ld, hipStream_t st) {
    if (out_w > 4096 || out_h > 4096) hg::fail(HG_ERR_ARG, "resize: NEAREST writes at most 4096 x 4096 pixels (the window gather's limit)");
    if (S->box_w != w || S->box_h != h) {
        const double box[4] = {0.0, 0.0, (double)w, (double)h};
        if (S->box.p) HG_HIP(hipStreamSynchronize(st));
        S->box.upload(box, sizeof box);
        S->box_w = w;
        S->box_h = h;
    }
    const bool dense = dst_ld == out_w;
    void* out = dst;
    if (!dense) {
        const size_t need = (size_t)out_w * out_h;
        if (S->mid.p && need > S->mid.bytes) HG_HIP(hipStreamSynchronize(st));
        S->mid.alloc(need);
        out = S->mid.p;
    }
    if (hg::patcher_extract_format(p, 0x52657a4e52535431ull, format, src, h, w, ld_bytes, (const double*)S->box.p, 1, out_w, out_h, out, HG_U8,
                                   (int64_t)out_w * out_h, st) != HG_OK)
        hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    if (!dense) HG_HIP(hipMemcpy2DAsync(dst, (size_t)dst_ld, out, (size_t)out_w, (size_t)out_w, (size_t)out_h, hipMemcpyDeviceToDevice, st));
}

}  // namespace

namespace hg {
void resample_state_free(void* state) { delete (ResampleState*)state; }
}  // namespace hg

extern "C" {

int hg_patcher_resize_device(hg_patcher* p, int filter, int flags, const void* src_dev, int format, int h, int w, int64_t ld_bytes, int out_format,
                             void* dst_dev, int out_h, int out_w, int64_t dst_ld_bytes, void* stream) {
    return guarded([&] {
        if (!p) hg::fail(HG_ERR_ARG, "null patcher handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "resize: bad flags %d (1: two launches, 2: one launch where eligible)", flags);
        if (const char* why = hg::resize_check(filter, src_dev, format, h, w, ld_bytes, out_format, dst_dev, out_h, out_w, dst_ld_bytes)) hg::fail(HG_ERR_ARG, "%s", why);
        if (std::max(w, out_w) > (1 << 28)) hg::fail(HG_ERR_ARG, "resize: rows of more than 2^28 pixels");
        HG_HIP(hipSetDevice(hg::patcher_device(p)));
        hipStream_t st = (hipStream_t)stream;
        ResampleState* S = state_of(p);
        const uint8_t* src = (const uint8_t*)src_dev;
        uint8_t* dst = (uint8_t*)dst_dev;
        if (filter == HG_RESAMPLE_NEAREST) {
            resize_nearest(p, S, src, format, h, w, ld_bytes, dst, out_h, out_w, dst_ld_bytes, st);
            return;
        }
        const bool gray = out_format == HG_FRAME_L;
        const int C = gray ? 1 : hg::frame_bpp(format);
        const int n = out_w * C;      // elements of an output row
        const bool need_h = out_w != w, need_v = out_h != h;
        const int packed = is_packed(dst, dst_ld_bytes);
        if (!need_h && !need_v) {
            if (gray) {      // convert("L") alone (HG_FRAME_L: a pitched copy)
                if (hg_frame_to_gray_device(hg::patcher_device(p), src, format, h, w, ld_bytes, dst, dst_ld_bytes, stream) != HG_OK)
                    hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
            } else {
                HG_HIP(hipMemcpy2DAsync(dst, (size_t)dst_ld_bytes, src, (size_t)ld_bytes, (size_t)n, (size_t)h, hipMemcpyDeviceToDevice, st));
            }
            return;
        }
        AxisEntry* ah = need_h ? axis_of(S, w, out_w, filter, nullptr, st) : nullptr;
        AxisEntry* av = need_v ? axis_of(S, h, out_h, filter, ah, st) : nullptr;
        dim3 thr, grid;
        if (need_h && need_v && hg::resize_vertical_first(h, w, out_h)) {
            // Image.resize's exception for very tall images: the height first, at full width, into the intermediate; then the width
            const int nw = w * C;
            const int64_t mid_ld = ((int64_t)nw + 3) & ~(int64_t)3;
            const size_t need = (size_t)mid_ld * (size_t)out_h;
            if (S->mid.p && need > S->mid.bytes) HG_HIP(hipStreamSynchronize(st));
            S->mid.alloc(need);
            shape_of(nw, out_h, thr, grid);
            by_mode(format, gray, [&](auto m) {
                using M = decltype(m);
                hipLaunchKernelGGL((k_resample_v<M>), grid, thr, 0, st, src, ld_bytes, 0, av->bounds(), av->k(), av->host.ksize, nw, out_h, (uint8_t*)S->mid.p, mid_ld, 1);
            });
            shape_of(n, out_h, thr, grid);
            by_mode(out_format, gray, [&](auto m) {      // the intermediate is an image of the output's format
                using M = Mode<decltype(m)::BPP, false, decltype(m)::BPP == 1>;
                hipLaunchKernelGGL((k_resample_h<M>), grid, thr, 0, st, (const uint8_t*)S->mid.p, mid_ld, 0, out_h, ah->bounds(), ah->k(), ah->host.ksize, n, dst,
                                   dst_ld_bytes, packed);
            });
        } else if (!need_v) {
            shape_of(n, h, thr, grid);
            by_mode(format, gray, [&](auto m) {
                using M = decltype(m);
                hipLaunchKernelGGL((k_resample_h<M>), grid, thr, 0, st, src, ld_bytes, 0, h, ah->bounds(), ah->k(), ah->host.ksize, n, dst, dst_ld_bytes, packed);
            });
        } else if (!need_h) {
            shape_of(n, out_h, thr, grid);
            by_mode(format, gray, [&](auto m) {
                using M = decltype(m);
                hipLaunchKernelGGL((k_resample_v<M>), grid, thr, 0, st, src, ld_bytes, 0, av->bounds(), av->k(), av->host.ksize, n, out_h, dst, dst_ld_bytes, packed);
            });
        } else if (!(flags & 1) && ((flags & 2) || kFusedDefault[!gray ? 2 : format != HG_FRAME_L ? 1 : 0][filter]) && av->max_tile_rows <= kFusedRows &&
                   (out_h + kTileH - 1) / kTileH <= 65535) {
            const dim3 tiles((unsigned)((n + kTileW - 1) / kTileW), (unsigned)((out_h + kTileH - 1) / kTileH));
            by_mode(format, gray, [&](auto m) {
                using M = decltype(m);
                hipLaunchKernelGGL((k_resample_fused<M>), tiles, 256, 0, st, src, ld_bytes, ah->bounds(), ah->k(), ah->host.ksize, av->bounds(), av->k(),
                                   av->host.ksize, n, out_h, dst, dst_ld_bytes, packed);
            });
        } else {
            const int y_first = av->host.bounds[0];
            const int y_last = av->host.bounds[(size_t)out_h * 2 - 2] + av->host.bounds[(size_t)out_h * 2 - 1];
            const int64_t mid_ld = ((int64_t)n + 3) & ~(int64_t)3;
            const size_t need = (size_t)mid_ld * (size_t)(y_last - y_first);
            if (S->mid.p && need > S->mid.bytes) HG_HIP(hipStreamSynchronize(st));      // a launch in flight may still read the old buffer
            S->mid.alloc(need);
            shape_of(n, y_last - y_first, thr, grid);
            by_mode(format, gray, [&](auto m) {
                using M = decltype(m);
                hipLaunchKernelGGL((k_resample_h<M>), grid, thr, 0, st, src, ld_bytes, y_first, y_last - y_first, ah->bounds(), ah->k(), ah->host.ksize, n,
                                   (uint8_t*)S->mid.p, mid_ld, 1);
            });
            shape_of(n, out_h, thr, grid);
            // the intermediate is an image of n one-byte elements a row, whatever the source was
            hipLaunchKernelGGL((k_resample_v<Mode<1, false, true>>), grid, thr, 0, st, (const uint8_t*)S->mid.p, mid_ld, y_first, av->bounds(), av->k(),
                               av->host.ksize, n, out_h, dst, dst_ld_bytes, packed);
        }
        HG_HIP(hipGetLastError());
    });
}

}  // extern "C"
