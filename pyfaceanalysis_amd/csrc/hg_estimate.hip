// Age, race and gender estimation for the faces of one frame: the reference's last step per image,
//     estimate_age_race_gender                             FaceDetectUpdated.py:1186-1187  (face_analysis.py:1170-1306)
//     1. normalize_image, out_size (256, 260), areaZ       :1214-1222   hg_patcher_normalize_device
//     2. one 96 x 96 sub-image of that crop + contrast     :1231-1247   k_age_patch (this file)
//     3. sl = networks[num_networks - 3].execute(...)      :1257        hg_flow_execute_device
//     4. age (with std), race and gender regressions on sl :1260-1292   hg_gauss_regression_device / _multi_device
// all enqueued on one stream, nothing read back.  Step 2 goes through cuicuilco's load_image_data_monoprocessor, which is not available:
// the rules are the build's (include/higsfa.h "Age, race and gender estimation") —
//     box       a plain parameter (pyfaceanalysis_amd.analysis.age_patch_box evaluates the reference's visible expressions)
//     cut       crop.transform((pw, ph), EXTENT, box, F), F NEAREST / BILINEAR / BICUBIC: the arithmetic of hg_extract.hip without rotation
//     contrast  the eye step's (k_eye_contrast, hg_eyes.hip): exact int64 sums, p' = (p - mean) / (std / target_std + 1e-8) + target_mean,
//               float32; `clip` 1 clips to [0, 255] as face_analysis.py:327 does, 0 does not
// k_age_patch fuses cut and contrast, one workgroup per face, the uint8 patch in LDS; patches above kFusedPixels pixels (and flag bit 0)
// take the composed path — hg_patcher_extract_filter_device per face into uint8 scratch, then k_patch_contrast — with the same bits.
//
// Workgroup size of k_age_patch: HG_EST_THREADS, 1024 unless the build defines another multiple of 64.  Both 256 and 1024 were measured
// (profiles/r16_analysis_times.txt; 96 x 96 patches of 256 x 260 crops, median device time of 30 alternated calls): one workgroup works
// on a face alone, so its time is the length of one thread's chain — 1 / 64 faces NEAREST 0.025 / 0.026 ms with 256 threads, 0.019 /
// 0.020 ms with 1024; BILINEAR 0.031 / 0.032 against 0.022 / 0.024 ms; BICUBIC 0.047 / 0.049 against 0.031 / 0.033 ms.  1024 is what
// is built.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "hg_common.hpp"
#include "hg_gauss_dev.hpp"
#include "hg_normalize.hpp"

#ifndef HG_EST_THREADS
#define HG_EST_THREADS 1024
#endif
static_assert(HG_EST_THREADS % 64 == 0 && HG_EST_THREADS >= 64 && HG_EST_THREADS <= 1024, "whole waves, at most 16");

namespace hg { void set_last_error(const std::string& s); }

// No contraction anywhere below (see hg_filter_dev.hpp): each double operation rounds on its own, as PIL's C doubles and numpy's do
// (tests/test_analysis_fp_contract.py checks the fma count).
#pragma clang fp contract(off)
namespace {
#include "hg_filter_dev.hpp"      // d_add / d_sub / d_mul / d_div, FiltEnt, filter_coord, bicubic, filter_sample

constexpr int kFusedPixels = 16384;               // patch pixels the fused kernel keeps in LDS
constexpr int kFusedEntries = 4096 + 4;           // w + h of such a patch with w, h <= 4096
constexpr int64_t kMaxPixels = 65536;             // N S2 - S1^2 stays exact in a double (as for the eye patches)

struct Box4 {
    double v[4];
};

// The NEAREST source index of output column / row i (hg_extract.hip extent_entry: PIL's running sum, one addition per output pixel
// before this one); -1: outside the crop, the output pixel stays 0.
__device__ __forceinline__ int32_t nearest_entry(double lo, double hi, int m, int i, int lim) {
    const double a = d_div(d_sub(hi, lo), (double)m);
    double o = d_add(lo, d_mul(a, 0.5));
    int k = 0;
    for (; k + 8 <= i; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) o = d_add(o, a);
    }
    for (; k < i; ++k) o = d_add(o, a);
    const int v = o < 0.0 ? -1 : (int)o;
    return (v >= 0 && v < lim) ? v : -1;
}

// The filtered coordinate of output column / row i (hg_extract.hip filter_entry): a closed form, PIL evaluates the affine map per pixel
__device__ __forceinline__ FiltEnt filtered_entry(double lo, double hi, int m, int i, int lim) {
    const double a = d_div(d_sub(hi, lo), (double)m);
    return filter_coord(d_add(d_mul(a, d_add((double)i, 0.5)), lo), lim);
}

// S1 = sum p, S2 = sum p^2 of the workgroup's pixels: wave shuffles, then across waves (integers: any order gives the same sums)
__device__ __forceinline__ void block_sums(long long s1, long long s2, long long* s1w, long long* s2w, long long& S1, long long& S2) {
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s1w[wave] = s1; s2w[wave] = s2; }
    __syncthreads();
    S1 = 0;
    S2 = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { S1 += s1w[w]; S2 += s2w[w]; }
}

// The divisor and the mean of the contrast step, k_eye_contrast's operations in its order
__device__ __forceinline__ void contrast_consts(long long S1, long long S2, long long N, double tstd, double& mean, double& div) {
    mean = d_div((double)S1, (double)N);
    const double sd = __dsqrt_rn(d_div((double)(N * S2 - S1 * S1), (double)(N * N)));
    div = d_add(d_div(sd, tstd), 1e-8);
}

__device__ __forceinline__ float contrast_pixel(uint8_t p, double mean, double div, double tmean, int clip) {
    double v = d_add(d_div(d_sub((double)p, mean), div), tmean);
    if (clip) v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    return (float)v;
}

// Cut and contrast of one face per workgroup.  crops: n images of ch rows of cw bytes, crop_stride bytes apart; out: n rows of
// pw * ph floats, ldp floats apart.  pw * ph <= kFusedPixels, pw, ph <= 4096 (the host checks).  Every index into the crop comes from
// nearest_entry / filter_coord / filter_sample, which keep it in [0, cw) x [0, ch).
template <int F>
__global__ void __launch_bounds__(HG_EST_THREADS) k_age_patch(const uint8_t* __restrict__ crops, int64_t crop_stride, int cw, int ch, Box4 box,
                                                                  int pw, int ph, int clip, double tmean, double tstd, float* __restrict__ out,
                                                                  int64_t ldp) {
    __shared__ uint8_t patch[kFusedPixels];
    __shared__ int32_t tab[F == HG_FILTER_NEAREST ? kFusedEntries : 1];
    __shared__ long long s1w[16], s2w[16];
    const uint8_t* __restrict__ crop = crops + (int64_t)blockIdx.x * crop_stride;
    const int npix = pw * ph;
    if constexpr (F == HG_FILTER_NEAREST) {
        for (int e = threadIdx.x; e < pw + ph; e += blockDim.x)
            tab[e] = e < pw ? nearest_entry(box.v[0], box.v[2], pw, e, cw) : nearest_entry(box.v[1], box.v[3], ph, e - pw, ch);
        __syncthreads();
    }
    long long s1 = 0, s2 = 0;
    for (int j = threadIdx.x; j < npix; j += blockDim.x) {
        const int y = j / pw, x = j - y * pw;
        uint8_t v = 0;
        if constexpr (F == HG_FILTER_NEAREST) {
            const int xs = tab[x], ys = tab[pw + y];
            if (xs >= 0 && ys >= 0) v = crop[(int64_t)ys * cw + xs];
        } else {
            const FiltEnt ex = filtered_entry(box.v[0], box.v[2], pw, x, cw), ey = filtered_entry(box.v[1], box.v[3], ph, y, ch);
            if (ex.i != kFiltOutside && ey.i != kFiltOutside)
                v = filter_sample<F>([&](int xc, int yc) { return (double)crop[(int64_t)yc * cw + xc]; }, ex.i, ex.d, ey.i, ey.d, cw, ch);
        }
        patch[j] = v;
        const long long q = v;
        s1 += q;
        s2 += q * q;
    }
    long long S1, S2;
    block_sums(s1, s2, s1w, s2w, S1, S2);      // (its barrier also publishes `patch`)
    double mean, div;
    contrast_consts(S1, S2, (long long)npix, tstd, mean, div);
    float* __restrict__ q = out + (int64_t)blockIdx.x * ldp;
    for (int j = threadIdx.x; j < npix; j += blockDim.x) q[j] = contrast_pixel(patch[j], mean, div, tmean, clip);
}

// The contrast step of the composed path: k_eye_contrast with the clip switch and an output row stride.  src: n patches npix bytes apart.
__global__ void __launch_bounds__(256) k_patch_contrast(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t ldp, int64_t npix, int clip,
                                                        double tmean, double tstd) {
    __shared__ long long s1w[16], s2w[16];
    const uint8_t* p = src + (int64_t)blockIdx.x * npix;
    float* q = dst + (int64_t)blockIdx.x * ldp;
    long long s1 = 0, s2 = 0;
    for (int64_t j = threadIdx.x; j < npix; j += blockDim.x) {
        const long long v = p[j];
        s1 += v;
        s2 += v * v;
    }
    long long S1, S2;
    block_sums(s1, s2, s1w, s2w, S1, S2);
    double mean, div;
    contrast_consts(S1, S2, (long long)npix, tstd, mean, div);
    for (int64_t j = threadIdx.x; j < npix; j += blockDim.x) q[j] = contrast_pixel(p[j], mean, div, tmean, clip);
}

// The finishing kernel: the rows of an absent classifier get the reference's initial values (face_analysis.py:1201-1204), a refused
// face (refused[i] != 0) NaN in all four rows.  out: (4, n) doubles, rows `stride` apart: age, age_std, race, gender.
__global__ void k_estimate_finish(int64_t n, const uint8_t* __restrict__ refused, double* __restrict__ out, int64_t stride, int has_age, int has_race,
                                  int has_gender) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (refused[i]) {
        for (int r = 0; r < 4; ++r) out[r * stride + i] = NAN;
        return;
    }
    if (!has_age) { out[i] = 0.0; out[stride + i] = 0.0; }
    if (!has_race) out[2 * stride + i] = 10.0;
    if (!has_gender) out[3 * stride + i] = 10.0;
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

void set_dev(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        hg::fail(HG_ERR_DEVICE, "no HIP device available (this library has no CPU execution path)");
    if (device < 0 || device >= count) hg::fail(HG_ERR_DEVICE, "device %d out of range (0..%d)", device, count - 1);
    HG_HIP(hipSetDevice(device));
}

constexpr int kSlots = 4;

}  // namespace

struct hg_estimator {
    int device = 0;
    hg_flow* flow = nullptr;
    hg_gauss *age = nullptr, *race = nullptr, *gender = nullptr;
    hg_estimator_consts c{};
    hg_patcher* patcher = nullptr;
    int64_t cap = 0, cap_u8 = 0;       // faces the buffers hold (cap_u8: the uint8 patches of the composed path)
    hg::DevBuf crops, pu8, pf32, sl, refused, box;
    // the refused flags travel through pinned memory, a ring of slots as for the normalise records (hg_normalize.hip)
    struct Slot {
        uint8_t* host = nullptr;
        size_t cap = 0;
        hipEvent_t copied = nullptr;
        bool pending = false;
    } slot[kSlots];
    int next = 0;

    int64_t npix() const { return (int64_t)c.patch_w * c.patch_h; }

    // Growing waits for `st`: a launch in flight may still read the old buffers
    void reserve(int64_t n, hipStream_t st) {
        if (n <= cap) return;
        if (cap) HG_HIP(hipStreamSynchronize(st));
        const int64_t m = std::max<int64_t>(n, 4);
        crops.alloc((size_t)m * c.crop_w * c.crop_h);
        pf32.alloc((size_t)m * npix() * 4);
        sl.alloc((size_t)m * c.n_features * 4);
        refused.alloc((size_t)m);
        if (hg_flow_reserve(flow, m) != HG_OK) hg::fail(HG_ERR_NOMEM, "%s", hg_last_error());
        cap = m;
    }
    void reserve_u8(int64_t n, hipStream_t st) {
        if (n <= cap_u8) return;
        if (cap_u8) HG_HIP(hipStreamSynchronize(st));
        const int64_t m = std::max<int64_t>(n, 4);
        pu8.alloc((size_t)m * npix());
        cap_u8 = m;
    }
};

namespace {

// bit 0: composed, bit 1: fused; neither: the default of the filter
bool use_fused(const hg_estimator* e, int flags, int64_t n) {
    if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "estimator: bad flags %d (1: composed patch path, 2: fused patch kernel)", flags);
    const bool fits = e->npix() <= kFusedPixels && e->c.patch_w + e->c.patch_h <= kFusedEntries;
    if ((flags & 2) && !fits) hg::fail(HG_ERR_ARG, "estimator: the fused patch kernel takes at most %d pixels, the patch has %lld", kFusedPixels, (long long)e->npix());
    if (flags & 1) return false;
    if (flags & 2) return true;
    // The default: the fused kernel only where it measured faster than the composed path by more than the spread between the two runs
    // (profiles/r16_analysis_times.txt; fused / composed, median device time, 1 / 4 / 16 / 64 faces): NEAREST 0.60 / 0.39 / 0.17 / 0.05,
    // BILINEAR 0.71 / 0.45 / 0.19 / 0.06 — fused; BICUBIC 0.97-0.99 at one face, inside the 4 % the composed path moved between the
    // runs — composed; 0.59 / 0.26 / 0.08 from four faces on — fused (two and three faces were not measured and stay composed).
    if (e->c.filter == HG_FILTER_BICUBIC && n < 4) return false;
    return fits;
}

// crops (device, n images crop_stride apart) -> out (n rows of patch_w * patch_h floats, ldp apart)
void run_patches(hg_estimator* e, bool fused, const uint8_t* crops, int64_t crop_stride, int64_t n, float* out, int64_t ldp, hipStream_t st) {
    const hg_estimator_consts& c = e->c;
    if (fused) {
        Box4 b;
        for (int k = 0; k < 4; ++k) b.v[k] = c.box[k];
#define HG_AGE_PATCH(FF) hipLaunchKernelGGL((k_age_patch<FF>), (unsigned)n, HG_EST_THREADS, 0, st, crops, crop_stride, c.crop_w, c.crop_h, b, c.patch_w, \
                                            c.patch_h, c.clip, c.target_mean, c.target_std, out, ldp)
        if (c.filter == HG_FILTER_NEAREST) HG_AGE_PATCH(HG_FILTER_NEAREST);
        else if (c.filter == HG_FILTER_BILINEAR) HG_AGE_PATCH(HG_FILTER_BILINEAR);
        else HG_AGE_PATCH(HG_FILTER_BICUBIC);
#undef HG_AGE_PATCH
        HG_HIP(hipGetLastError());
        return;
    }
    // composed: every crop is a frame of its own with the one box
    e->reserve_u8(n, st);
    const int64_t wh = e->npix();
    for (int64_t i = 0; i < n; ++i)
        if (hg_patcher_extract_filter_device(e->patcher, c.filter, crops + i * crop_stride, HG_U8, c.crop_h, c.crop_w, c.crop_w, (const double*)e->box.p, nullptr, 1,
                                             c.patch_w, c.patch_h, (uint8_t*)e->pu8.p + i * wh, HG_U8, wh, st) != HG_OK)
            hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    hipLaunchKernelGGL(k_patch_contrast, (unsigned)n, 256, 0, st, (const uint8_t*)e->pu8.p, out, ldp, wh, c.clip, c.target_mean, c.target_std);
    HG_HIP(hipGetLastError());
}

constexpr int64_t kMaxFaces = 1 << 20;

}  // namespace

extern "C" {

int hg_estimator_create(hg_flow* flow, hg_gauss* age, hg_gauss* race, hg_gauss* gender, const hg_estimator_consts* consts, hg_patcher* patcher, int device,
                        hg_estimator** out) {
    return guarded([&] {
        if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
        *out = nullptr;
        // in argument order where a host can tell: constants, the flow's shape, the classifiers; then what needs the device
        if (!consts) hg::fail(HG_ERR_ARG, "null constants");
        const hg_estimator_consts& c = *consts;
        if (c.crop_w < 1 || c.crop_w > 4096 || c.crop_h < 1 || c.crop_h > 4096) hg::fail(HG_ERR_ARG, "bad crop size %d x %d (1 .. 4096 each)", c.crop_w, c.crop_h);
        if (c.method != HG_NORM_AREA && c.method != HG_NORM_AREAZ) hg::fail(HG_ERR_ARG, "unknown normalisation method %d", c.method);
        if (c.rotate != 0 && c.rotate != 1) hg::fail(HG_ERR_ARG, "rotate must be 0 or 1");
        if (c.patch_w < 1 || c.patch_w > 4096 || c.patch_h < 1 || c.patch_h > 4096 || (int64_t)c.patch_w * c.patch_h > kMaxPixels)
            hg::fail(HG_ERR_ARG, "bad patch size %d x %d (at most 4096 per side and 65536 pixels: N S2 stays exact in a double)", c.patch_w, c.patch_h);
        if (c.filter != HG_FILTER_NEAREST && c.filter != HG_FILTER_BILINEAR && c.filter != HG_FILTER_BICUBIC)
            hg::fail(HG_ERR_ARG, "unknown interpolation filter %d (0 NEAREST, 2 BILINEAR, 3 BICUBIC)", c.filter);
        if (c.clip != 0 && c.clip != 1) hg::fail(HG_ERR_ARG, "clip must be 0 or 1");
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(c.box[k])) hg::fail(HG_ERR_ARG, "the patch box must be finite");
        if (!(c.target_std > 0.0) || !std::isfinite(c.target_std) || !std::isfinite(c.target_mean))
            hg::fail(HG_ERR_ARG, "bad contrast targets (target_std > 0, both finite; required)");
        if (c.n_features <= 0 || c.n_features > 256) hg::fail(HG_ERR_ARG, "bad feature count %d", c.n_features);
        if (c.reserved != 0) hg::fail(HG_ERR_ARG, "reserved must be 0");
        if (!flow) hg::fail(HG_ERR_ARG, "null flow");
        hg_info info{};
        if (hg_flow_info(flow, &info) != HG_OK) hg::fail(HG_ERR_ARG, "%s", hg_last_error());
        if (info.input_dim != (int64_t)c.patch_w * c.patch_h)
            hg::fail(HG_ERR_DIM, "the flow reads %lld columns, patches have %d x %d", (long long)info.input_dim, c.patch_w, c.patch_h);
        if (info.output_dim < c.n_features) hg::fail(HG_ERR_DIM, "the flow gives %lld features, %d kept", (long long)info.output_dim, c.n_features);
        if (!age && !race && !gender) hg::fail(HG_ERR_ARG, "at least one classifier (age, race, gender) must be given");
        for (hg_gauss* g : {age, race, gender}) {
            if (!g) continue;
            const hg::GaussParams P = hg::gauss_params(g);
            if (P.d > c.n_features) hg::fail(HG_ERR_DIM, "a classifier reads %d features, %d kept", P.d, c.n_features);
        }
        if (info.device != device) hg::fail(HG_ERR_ARG, "the flow lives on device %d, not %d", info.device, device);
        if (!patcher) hg::fail(HG_ERR_ARG, "null patcher handle");
        if (hg::patcher_device(patcher) != device) hg::fail(HG_ERR_ARG, "the patcher lives on device %d, not %d", hg::patcher_device(patcher), device);
        set_dev(device);
        auto e = std::make_unique<hg_estimator>();
        e->device = device;
        e->flow = flow; e->age = age; e->race = race; e->gender = gender;
        e->c = c;
        e->patcher = patcher;
        e->box.upload(c.box, 32);
        *out = e.release();
    });
}

void hg_estimator_free(hg_estimator* e) {
    if (!e) return;
    if (hipSetDevice(e->device) == hipSuccess) {
        for (auto& s : e->slot) {
            if (s.pending) (void)hipEventSynchronize(s.copied);
            if (s.copied) (void)hipEventDestroy(s.copied);
            if (s.host) (void)hipHostFree(s.host);
        }
    }
    delete e;
}

int hg_estimator_patches_device(hg_estimator* e, int flags, const uint8_t* crops_dev, int64_t crop_stride, int64_t n, float* patches_dev, int64_t ldp,
                                void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null estimator handle");
        const bool fused = use_fused(e, flags, n);
        if (n < 0 || n > kMaxFaces) hg::fail(HG_ERR_ARG, "bad face count");
        if (crop_stride < (int64_t)e->c.crop_w * e->c.crop_h) hg::fail(HG_ERR_ARG, "crops %lld bytes apart hold %d x %d", (long long)crop_stride, e->c.crop_w, e->c.crop_h);
        if (ldp < e->npix()) hg::fail(HG_ERR_ARG, "patch rows %lld floats apart hold %d x %d", (long long)ldp, e->c.patch_w, e->c.patch_h);
        if (n > 0 && (!crops_dev || !patches_dev)) hg::fail(HG_ERR_ARG, "null data pointer");
        if (n == 0) return;
        set_dev(e->device);
        run_patches(e, fused, crops_dev, crop_stride, n, patches_dev, ldp, (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {

// The chain of all three estimate entries behind their argument checks, n > 0.  frames_dev / n_frames / frame_stride / face_frame_host: the
// stack's (face_frame_host == nullptr: the single frame at frames_dev); list != nullptr: the n_frames descriptors of a LIST of frames of
// different sizes in place of frames_dev and the one frame shape.  A face whose frame index lies outside the stack / list counts as refused.
void run_estimate(hg_estimator* e, bool fused, const uint8_t* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld,
                  const hg_norm_geom* geoms_host, const int32_t* face_frame_host, int64_t n, double* out_dev, int64_t out_stride, float* patches_dev,
                  float* features_dev, void* stream, const hg_frame_ref* list = nullptr) {
        set_dev(e->device);
        hipStream_t st = (hipStream_t)stream;
        const hg_estimator_consts& c = e->c;
        e->reserve(n, st);
        // 1. the crops (a refused face: all zero)
        const int64_t crop_bytes = (int64_t)c.crop_w * c.crop_h;
        const int rc = list
            ? hg_patcher_normalize_frame_list_device(e->patcher, 0, list, n_frames, geoms_host, face_frame_host, n, c.crop_w, c.crop_h, (uint8_t*)e->crops.p, crop_bytes, st)
            : face_frame_host
            ? hg_patcher_normalize_frames_device(e->patcher, 0, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, geoms_host, face_frame_host, n, c.crop_w,
                                                 c.crop_h, (uint8_t*)e->crops.p, crop_bytes, st)
            : hg_patcher_normalize_device(e->patcher, 0, frames_dev, frame_h, frame_w, ld, geoms_host, n, c.crop_w, c.crop_h, (uint8_t*)e->crops.p, crop_bytes, st);
        if (rc != HG_OK) hg::fail(HG_ERR_ARG, "%s", hg_last_error());      // (its refusals are all argument errors; the message is its own)
        // the refused flags, through the ring
        hg_estimator::Slot& slot = e->slot[e->next];
        e->next = (e->next + 1) % kSlots;
        if (slot.pending) {
            HG_HIP(hipEventSynchronize(slot.copied));      // the upload of four calls ago
            slot.pending = false;
        }
        if (!slot.copied) HG_HIP(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
        if ((size_t)n > slot.cap) {
            if (slot.host) HG_HIP(hipHostFree(slot.host));
            slot.host = nullptr;
            slot.cap = 0;
            const size_t cap = std::max<size_t>((size_t)n, 64);
            HG_HIP(hipHostMalloc((void**)&slot.host, cap, hipHostMallocDefault));
            slot.cap = cap;
        }
        for (int64_t i = 0; i < n; ++i)
            slot.host[i] = (geoms_host[i].status != 0 || (face_frame_host && (face_frame_host[i] < 0 || face_frame_host[i] >= n_frames))) ? 1 : 0;
        HG_HIP(hipMemcpyAsync(e->refused.p, slot.host, (size_t)n, hipMemcpyHostToDevice, st));
        HG_HIP(hipEventRecord(slot.copied, st));
        slot.pending = true;
        // 2. the patches
        float* pf = patches_dev ? patches_dev : (float*)e->pf32.p;
        const int64_t wh = e->npix();
        run_patches(e, fused, (const uint8_t*)e->crops.p, crop_bytes, n, pf, wh, st);
        // 3. the network
        const int k = c.n_features;
        float* sl = features_dev ? features_dev : (float*)e->sl.p;
        if (hg_flow_execute_device(e->flow, pf, HG_F32, n, wh, sl, HG_F32, k, k, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        // 4. the regressions, straight into the rows of out
        if (e->age && hg_gauss_regression_device(e->age, sl, HG_F32, n, k, out_dev, out_dev + out_stride, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        if (e->race && e->gender) {
            hg_gauss* g[2] = {e->race, e->gender};
            if (hg_gauss_regression_multi_device(g, 2, sl, HG_F32, n, k, out_dev + 2 * out_stride, out_stride, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        } else if (e->race || e->gender) {
            hg_gauss* g = e->race ? e->race : e->gender;
            if (hg_gauss_regression_multi_device(&g, 1, sl, HG_F32, n, k, out_dev + (e->race ? 2 : 3) * out_stride, out_stride, st) != HG_OK)
                hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        }
        // 5. absent classifiers and refused faces
        hipLaunchKernelGGL(k_estimate_finish, (unsigned)((n + 255) / 256), 256, 0, st, n, (const uint8_t*)e->refused.p, out_dev, out_stride, e->age ? 1 : 0, e->race ? 1 : 0,
                           e->gender ? 1 : 0);
        HG_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int hg_estimator_estimate_device(hg_estimator* e, int flags, const uint8_t* frame_dev, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms_host,
                                 int64_t n, double* out_dev, int64_t out_stride, float* patches_dev, float* features_dev, void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null estimator handle");
        const bool fused = use_fused(e, flags, n);
        if (n < 0 || n > kMaxFaces) hg::fail(HG_ERR_ARG, "bad face count");
        if (frame_h <= 0 || frame_w <= 0 || ld < frame_w) hg::fail(HG_ERR_ARG, "bad frame shape");
        if (out_stride < n) hg::fail(HG_ERR_ARG, "output rows %lld apart hold %lld faces", (long long)out_stride, (long long)n);
        if (n > 0 && (!frame_dev || !geoms_host || !out_dev)) hg::fail(HG_ERR_ARG, "null data pointer");
        if (n == 0) return;
        run_estimate(e, fused, frame_dev, 1, 0, frame_h, frame_w, ld, geoms_host, nullptr, n, out_dev, out_stride, patches_dev, features_dev, stream);
    });
}

int hg_estimator_estimate_frames_device(hg_estimator* e, int flags, const uint8_t* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w,
                                        int64_t ld, const hg_norm_geom* geoms_host, const int32_t* face_frame_host, int64_t n, double* out_dev,
                                        int64_t out_stride, float* patches_dev, float* features_dev, void* stream) {
    return guarded([&] {
        // what a host can tell comes first and reads nothing behind the handle: a zeroed block in its place is refused, or told HG_OK at n == 0, like a live one
        if (!e) hg::fail(HG_ERR_ARG, "null estimator handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "estimator: bad flags %d (1: composed patch path, 2: fused patch kernel)", flags);
        if (n > kMaxFaces) hg::fail(HG_ERR_ARG, "bad face count");
        if (const char* why = hg::normalize_stack_check(frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, geoms_host, face_frame_host, n))
            hg::fail(HG_ERR_ARG, "%s", why);
        if (out_stride < n) hg::fail(HG_ERR_ARG, "output rows %lld apart hold %lld faces", (long long)out_stride, (long long)n);
        if (n > 0 && !out_dev) hg::fail(HG_ERR_ARG, "null data pointer");
        const bool fused = use_fused(e, flags, n);
        if (n == 0) return;
        run_estimate(e, fused, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, geoms_host, face_frame_host, n, out_dev, out_stride, patches_dev, features_dev,
                     stream);
    });
}

int hg_estimator_estimate_frame_list_device(hg_estimator* e, int flags, const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms_host,
                                            const int32_t* face_frame_host, int64_t n, double* out_dev, int64_t out_stride, float* patches_dev,
                                            float* features_dev, void* stream) {
    return guarded([&] {
        // as for the stack: what a host can tell comes first and reads nothing behind the handle
        if (!e) hg::fail(HG_ERR_ARG, "null estimator handle");
        if ((flags & ~3) || flags == 3) hg::fail(HG_ERR_ARG, "estimator: bad flags %d (1: composed patch path, 2: fused patch kernel)", flags);
        if (n > kMaxFaces) hg::fail(HG_ERR_ARG, "bad face count");
        const std::string why = hg::normalize_list_check(frames, n_frames, geoms_host, face_frame_host, n);
        if (!why.empty()) hg::fail(HG_ERR_ARG, "%s", why.c_str());
        if (out_stride < n) hg::fail(HG_ERR_ARG, "output rows %lld apart hold %lld faces", (long long)out_stride, (long long)n);
        if (n > 0 && !out_dev) hg::fail(HG_ERR_ARG, "null data pointer");
        const bool fused = use_fused(e, flags, n);
        if (n == 0) return;
        run_estimate(e, fused, nullptr, n_frames, 0, 0, 0, 0, geoms_host, face_frame_host, n, out_dev, out_stride, patches_dev, features_dev, stream, frames);
    });
}

}  // extern "C"
