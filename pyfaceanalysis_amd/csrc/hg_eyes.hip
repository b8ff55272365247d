// Eye localisation and duplicate purge after the face cascade: what the reference does per image once the 17 face stages are done,
//     eye boxes from the face boxes                        FaceDetectUpdated.py:947-950   (face_analysis.py:61-135)
//     find_Left_eyes / find_Right_eyes                     FaceDetectUpdated.py:992-1004  (face_analysis.py:1018-1109)
//     discard of the too-far faces, eye centres            FaceDetectUpdated.py:1006-1017
//     one row per face                                     FaceDetectUpdated.py:1036-1041
//     purgue_detected_faces_angles_eyes_confidence         FaceDetectUpdated.py:1180      (face_analysis.py:186-221)
// so that the frame path ends where the reference's per-image output does.  Float64 glue in the reference's operation order,
// no contraction (see the pragma below); the eye patches go through the patcher's rotated gather and the networks through
// hg_flow_execute_device / hg_gauss_regression_multi_device, all on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "hg_common.hpp"
#include "hg_frame_list.hpp"
#include "hg_gauss_dev.hpp"

namespace hg { void set_last_error(const std::string& s); }

// No contraction anywhere below: hipcc's default is -ffp-contract=fast-honor-pragmas, and the __dadd_rn / __dsub_rn / __dmul_rn of
// the HIP headers are plain operators compiled under that default, so a multiply feeding an add may become one fma.  These are
// defined under the pragma: their operations carry no contract flag, so each rounds on its own as numpy's do.
#pragma clang fp contract(off)
namespace {
__device__ __forceinline__ double d_add(double a, double b) { return a + b; }
__device__ __forceinline__ double d_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double d_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double d_div(double a, double b) { return a / b; }
}  // namespace

struct hg_eyes {
    int device = 0;
    hg_flow *fx = nullptr, *fy = nullptr;
    hg_gauss *gx = nullptr, *gy = nullptr;
    hg_eye_consts c{};
    hg_patcher* patcher = nullptr;
    int filter = HG_FILTER_NEAREST;      // of the eye patches (hg_eyes_set_interpolation)
    int64_t cap = 0;       // faces the buffers hold
    hg::DevBuf eboxes, dang, pu8, pf32, sl, sl2, reg, ecoords, toofar, rows, purged, scratch, count;
    hg::DevBuf row_src, kept_idx;        // a tracker's slots: the face of every assembled row, the assembled row of every kept row
    int32_t* host_words = nullptr;       // pinned: {faces after the discard, faces after the purge}
    hg::DevBuf row_frame, seg;           // a per-frame purge (eyes_tail_enqueue): the frame of every eye row; first row of every frame (n_frames + 1), rows kept per frame

    void reserve(int64_t n) {
        if (n <= cap) return;
        const size_t wh = (size_t)c.eye_w * c.eye_h;
        eboxes.alloc((size_t)n * 2 * 32);
        dang.alloc((size_t)n * 2 * 8);
        pu8.alloc((size_t)n * 2 * wh);
        pf32.alloc((size_t)n * 2 * wh * 4);
        sl.alloc((size_t)n * 2 * c.n_features * 4);
        if (fy != fx) sl2.alloc((size_t)n * 2 * c.n_features * 4);
        reg.alloc((size_t)n * 4 * 8);
        ecoords.alloc((size_t)n * 32);
        toofar.alloc((size_t)n);
        rows.alloc((size_t)n * 80);
        purged.alloc((size_t)(n + 1) * 80);
        scratch.alloc((size_t)(n + 1) * 16);
        row_src.alloc((size_t)n * 4);
        kept_idx.alloc((size_t)(n + 1) * 4);
        count.alloc(16);
        if (hg_flow_reserve(fx, 2 * n) != HG_OK || (fy != fx && hg_flow_reserve(fy, 2 * n) != HG_OK)) hg::fail(HG_ERR_NOMEM, "%s", hg_last_error());
        cap = n;
    }
};

namespace {

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

// compute_approximate_eye_boxes_coordinates(box, face_sampling=0.825, eye_sampling=2.3719, rot_angle=angle), face_analysis.py:61-135
// (its body spells the two samplings as literals; here they are the constants, equal to them).  Left box -> row i, right box ->
// row n + i; both patches are cut from the frame rotated by delta_ang = -1 * angle (face_analysis.py:1042, :782).
// n_dev (nullable): the number of faces lives on the device and n is the host's bound of it (a tracked frame, hg_cascade.hip) — the
// layout stays that of n faces, and the rows of the faces between the live count and n, whose boxes are whatever an earlier frame
// left there, get one defined window (the frame's first pixel, no rotation): the extraction and the networks behind this kernel are
// sized by n and must read finite boxes.
__global__ void k_eye_boxes(int64_t n, const int32_t* __restrict__ n_dev, const double* __restrict__ boxes, const double* __restrict__ angles,
                            hg_eye_consts c, double* __restrict__ eboxes, double* __restrict__ dang) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (n_dev && i >= *n_dev) {
        const double filler[4] = {0.0, 0.0, 1.0, 1.0};
        for (int q = 0; q < 4; ++q) eboxes[i * 4 + q] = eboxes[(n + i) * 4 + q] = filler[q];
        if (dang) dang[i] = dang[n + i] = 0.0;
        return;
    }
    const double x0 = boxes[i * 4], y0 = boxes[i * 4 + 1], x1 = boxes[i * 4 + 2], y1 = boxes[i * 4 + 3], ang = angles[i];
    const double fc_x = d_div(d_add(x0, x1), 2.0), fc_y = d_div(d_add(y0, y1), 2.0);                          // :89-90
    const double two_fs = d_mul(2.0, c.face_sampling);
    const double eye_dx = d_div(d_mul(18.5, d_div(fabs(d_sub(x1, x0)), 64.0)), two_fs);                        // :104
    const double eye_dy = d_div(d_mul(21.0, d_div(fabs(d_sub(y1, y0)), 64.0)), two_fs);                        // :105
    const double box_w = d_mul(d_div(fabs(d_sub(x1, x0)), d_mul(128.0, c.face_sampling)),
                                   d_div(d_mul(64.0, c.eye_sampling), 2.0));                                           // :109
    const double box_h = d_add(box_w, 0.0);                                                                                // :111
    const double rad = d_div(d_mul(ang, M_PI), 180.0);                                                                 // :115
    const double cs = cos(rad), sn = sin(rad);
    const double r_dx = d_sub(d_mul(eye_dx, cs), d_mul(eye_dy, sn));                                              // :117-120
    const double r_dy = d_add(d_mul(eye_dy, cs), d_mul(eye_dx, sn));
    const double l_dx = d_sub(d_mul(-eye_dx, cs), d_mul(eye_dy, sn));
    const double l_dy = d_add(d_mul(eye_dy, cs), d_mul(-eye_dx, sn));
    const double lx = d_add(fc_x, l_dx), rx = d_add(fc_x, r_dx);                                                      // :122-125
    const double ly = d_sub(fc_y, l_dy), ry = d_sub(fc_y, r_dy);
    const double hw = d_div(box_w, 2.0), hh = d_div(box_h, 2.0);                                                      // :126-133
    double* L = eboxes + i * 4;
    double* R = eboxes + (n + i) * 4;
    L[0] = d_sub(lx, hw); L[1] = d_sub(ly, hh); L[2] = d_add(lx, hw); L[3] = d_add(ly, hh);
    R[0] = d_sub(rx, hw); R[1] = d_sub(ry, hh); R[2] = d_add(rx, hw); R[3] = d_add(ry, hh);
    if (dang) {
        dang[i] = -ang;
        dang[n + i] = -ang;
    }
}

// The contrast step, one workgroup per gathered uint8 patch: image_array_contrast_normalize_avg_std (face_analysis.py:318-327) with
// exactly reproducible statistics — S1 = sum p, S2 = sum p^2 as int64 (zeros outside the frame included), mean = S1 / N,
// std = sqrt((N S2 - S1^2) / (N N)), one rounding per operation; p' = (p - mean) / (std / target_std + 1e-8) + target_mean, clipped
// to [0, 255], stored as float32 without quantising back to 8 bits.
__global__ void __launch_bounds__(256) k_eye_contrast(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t npix, double tmean,
                                                      double tstd) {
    __shared__ long long s1w[4], s2w[4];
    const uint8_t* p = src + (int64_t)blockIdx.x * npix;
    float* q = dst + (int64_t)blockIdx.x * npix;
    long long s1 = 0, s2 = 0;
    for (int64_t j = threadIdx.x; j < npix; j += blockDim.x) {
        const long long v = p[j];
        s1 += v;
        s2 += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s1w[wave] = s1; s2w[wave] = s2; }
    __syncthreads();
    long long S1 = 0, S2 = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { S1 += s1w[w]; S2 += s2w[w]; }
    const long long N = npix;
    const double mean = d_div((double)S1, (double)N);
    const double sd = __dsqrt_rn(d_div((double)(N * S2 - S1 * S1), (double)(N * N)));
    const double div = d_add(d_div(sd, tstd), 1e-8);
    for (int64_t j = threadIdx.x; j < npix; j += blockDim.x) {
        double v = d_add(d_div(d_sub((double)p[j], mean), div), tmean);
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
        q[j] = (float)v;
    }
}

// The shift of one eye box by its two regressions (face_analysis.py:1078-1104, left_eye = 1 for both eyes) and its centre
// (FaceDetectUpdated.py:1008-1009).
__device__ __forceinline__ void shift_eye(const double* b, double rx, double ry, double cs, double sn, const hg_eye_consts& c, double& ex, double& ey) {
    const double ox = d_div(d_mul(d_div(rx, c.eye_sampling), fabs(d_sub(b[2], b[0]))), c.eye_regression_width);
    const double oy = d_div(d_mul(d_div(ry, c.eye_sampling), fabs(d_sub(b[3], b[1]))), c.eye_regression_height);
    const double dx = d_sub(d_mul(ox, cs), d_mul(oy, sn));
    const double dy = d_add(d_mul(oy, cs), d_mul(ox, sn));
    ex = d_div(d_add(d_sub(b[0], dx), d_sub(b[2], dx)), 2.0);
    ey = d_div(d_add(d_sub(b[1], dy), d_sub(b[3], dy)), 2.0);
}

// Too-far test, rotated shift and eye centres per face; then the order-preserving compaction of the faces kept
// (FaceDetectUpdated.py:1010-1017; k_cascade_compact's ballot scan, one workgroup over chunks of its size) and the 10-column rows
// (:1036-1041).  reg: [0, 2n) EyeLX, [reg_stride, reg_stride + 2n) EyeLY; row i left eye, n + i right eye.  Every output may be null.
// n_dev (nullable): only the first min(*n_dev, n) faces exist (k_eye_boxes); the layout stays that of n faces.
// row_src (nullable): row_src[j] = the face i that assembled row j was made from (what a tracker's slots are composed of).
__global__ void __launch_bounds__(1024) k_eyes_glue(int64_t n, const int32_t* __restrict__ n_dev, hg_eye_consts c, const double* __restrict__ boxes, const double* __restrict__ angles,
                                                    const double* __restrict__ conf, const double* __restrict__ eboxes, const double* __restrict__ reg,
                                                    int64_t reg_stride, double* __restrict__ ecoords, uint8_t* __restrict__ toofar,
                                                    double* __restrict__ rows, int32_t* __restrict__ count, int32_t* __restrict__ row_src) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    const int64_t live = (n_dev && *n_dev < n) ? (int64_t)*n_dev : n;
    for (int64_t i0 = 0; i0 < live; i0 += blockDim.x) {
        const int64_t i = i0 + tid;
        int keep = 0;
        double e[4] = {0.0, 0.0, 0.0, 0.0};
        if (i < live) {
            const double rxl = reg[i], rxr = reg[n + i], ryl = reg[reg_stride + i], ryr = reg[reg_stride + n + i];
            const bool far = fabs(rxl) >= c.tolerance || fabs(ryl) >= c.tolerance || fabs(rxr) >= c.tolerance || fabs(ryr) >= c.tolerance;
            const double rad = d_div(d_mul(-angles[i], M_PI), 180.0);                           // face_analysis.py:1096
            const double cs = cos(rad), sn = sin(rad);
            shift_eye(eboxes + i * 4, rxl, ryl, cs, sn, c, e[0], e[1]);
            shift_eye(eboxes + (n + i) * 4, rxr, ryr, cs, sn, c, e[2], e[3]);
            if (ecoords) for (int q = 0; q < 4; ++q) ecoords[i * 4 + q] = e[q];
            if (toofar) toofar[i] = far ? 1 : 0;
            keep = far ? 0 : 1;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep && rows) {
            double* r = rows + (int64_t)(off + before) * 10;
            for (int q = 0; q < 4; ++q) r[q] = boxes[i * 4 + q];
            r[4] = angles[i];
            for (int q = 0; q < 4; ++q) r[5 + q] = e[q];
            r[9] = conf[i];
        }
        if (keep && row_src) row_src[off + before] = (int32_t)i;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    if (tid == 0 && count) *count = base;
}

// ---- the purge (face_analysis.py:186-221), one workgroup ------------------------------------------------------------------------
// numpy.argsort(w, kind="stable")[::-1]: descending, NaN first (numpy sorts NaN last), equal keys (-0 == +0, NaN == NaN) by
// DESCENDING index.  j precedes i in that order:
__device__ __forceinline__ bool precedes(double wj, int64_t j, double wi, int64_t i) {
    const bool nj = isnan(wj), ni = isnan(wi);
    if (nj != ni) return nj;
    if (!nj && wj != wi) return wj > wi;
    return j > i;
}

// relative_error_detection(app = cand[5:9], eye = kept[5:9]), face_analysis.py:158-165: Python's max() keeps its first argument
// unless the second is larger; x / 0 is inf or NaN as numpy's is.
__device__ __forceinline__ double rel_error(const double* a, const double* e) {
    const double l0 = d_sub(e[0], a[0]), l1 = d_sub(e[1], a[1]);
    const double r0 = d_sub(e[2], a[2]), r1 = d_sub(e[3], a[3]);
    const double d0 = d_sub(e[0], e[2]), d1 = d_sub(e[1], e[3]);
    const double dl = __dsqrt_rn(d_add(d_mul(l0, l0), d_mul(l1, l1)));
    const double dr = __dsqrt_rn(d_add(d_mul(r0, r0), d_mul(r1, r1)));
    const double de = __dsqrt_rn(d_add(d_mul(d0, d0), d_mul(d1, d1)));
    return d_div(dr > dl ? dr : dl, de);
}

// The purge of the n rows at `rows` by the workgroup that calls it (k_purge: all rows; k_purge_frames: one frame's rows).
// scratch: w (n_max doubles), then perm (n_max int32) and kept (n_max + 1 int32).
// out: room for n + 1 rows; *count = rows written.  kept_out (nullable, n_max + 1 entries): the index in `rows` of every row written.
__device__ __forceinline__ void purge_rows(const double* __restrict__ rows, int64_t n, int64_t n_max, double* __restrict__ out, int32_t* __restrict__ count,
                                           char* __restrict__ scratch, int32_t* __restrict__ kept_out) {
    __shared__ double tile[1024];
    __shared__ double redv[16];
    __shared__ int redf[16];
    __shared__ int nk_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (n <= 1) {                       // :219-220: a copy
        for (int64_t q = tid; q < n * 10; q += blockDim.x) out[q] = rows[q];
        if (tid == 0 && n == 1 && kept_out) kept_out[0] = 0;
        if (tid == 0) *count = (int32_t)n;
        return;
    }
    double* w = (double*)scratch;
    int32_t* perm = (int32_t*)(scratch + n_max * 8);
    int32_t* kept = perm + n_max;
    // weights (:193-197): (1 - conf) * ((eR_x - eL_x)^2 + (eR_y - eL_y)^2) ** 0.5, then w / w.max() (NaN propagates; of two equal
    // zeros the positive one)
    double mx = -INFINITY;
    int nan = 0;
    for (int64_t i = tid; i < n; i += blockDim.x) {
        const double* r = rows + i * 10;
        const double dx = d_sub(r[7], r[5]), dy = d_sub(r[8], r[6]);
        const double v = d_mul(d_sub(1.0, r[9]), __dsqrt_rn(d_add(d_mul(dx, dx), d_mul(dy, dy))));
        w[i] = v;
        if (isnan(v)) nan = 1;
        else if (v > mx || (v == mx && !signbit(v))) mx = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_down(mx, o, 64);
        nan |= __shfl_down(nan, o, 64);
        if (v > mx || (v == mx && !signbit(v))) mx = v;
    }
    if (lane == 0) { redv[wave] = mx; redf[wave] = nan; }
    __syncthreads();
    mx = redv[0];
    nan = redf[0];
    for (int q = 1; q < nw; ++q) {
        const double v = redv[q];
        nan |= redf[q];
        if (v > mx || (v == mx && !signbit(v))) mx = v;
    }
    if (nan) mx = NAN;
    for (int64_t i = tid; i < n; i += blockDim.x) w[i] = d_div(w[i], mx);
    __syncthreads();
    // the order (:198-200): rank of i = number of rows that precede it; the order is total, so the ranks are a permutation
    for (int64_t i0 = 0; i0 < n; i0 += blockDim.x) {
        const int64_t i = i0 + tid;
        const double wi = i < n ? w[i] : 0.0;
        int64_t rank = 0;
        for (int64_t j0 = 0; j0 < n; j0 += 1024) {
            __syncthreads();
            for (int q = tid; q < 1024 && j0 + q < n; q += blockDim.x) tile[q] = w[j0 + q];
            __syncthreads();
            const int64_t m = n - j0 < 1024 ? n - j0 : 1024;
            if (i < n)
                for (int64_t q = 0; q < m; ++q) rank += precedes(tile[q], j0 + q, wi, i) ? 1 : 0;
        }
        if (i < n) perm[rank] = (int32_t)i;
    }
    __syncthreads();
    // the greedy pass (:208-218): the first row, then every row in order (the first one again included) whose smallest error
    // against the rows kept so far — min_d starts at 10000 and moves on error < min_d only — is > 0.25
    if (tid == 0) { kept[0] = perm[0]; nk_s = 1; }
    __syncthreads();
    for (int64_t p = 0; p < n; ++p) {
        const int nk = nk_s;
        const double* a = rows + (int64_t)perm[p] * 10 + 5;
        double md = 10000.0;
        for (int k = tid; k < nk; k += blockDim.x) {
            const double err = rel_error(a, rows + (int64_t)kept[k] * 10 + 5);
            if (err < md) md = err;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_down(md, o, 64);
            if (v < md) md = v;
        }
        if (lane == 0) redv[wave] = md;
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < nw; ++q) md = redv[q] < md ? redv[q] : md;
            if (md > 0.25) kept[nk_s++] = perm[p];
        }
        __syncthreads();
    }
    const int nk = nk_s;
    for (int64_t q = tid; q < (int64_t)nk * 10; q += blockDim.x) out[q] = rows[(int64_t)kept[q / 10] * 10 + q % 10];
    if (kept_out)
        for (int q = tid; q < nk; q += blockDim.x) kept_out[q] = kept[q];
    if (tid == 0) *count = nk;
}

// rows (n_max, 10); n = min(*n_dev, n_max) when n_dev is given.
__global__ void __launch_bounds__(1024) k_purge(const double* __restrict__ rows, int64_t n_max, const int32_t* __restrict__ n_dev,
                                                double* __restrict__ out, int32_t* __restrict__ count, char* __restrict__ scratch,
                                                int32_t* __restrict__ kept_out) {
    const int64_t n = (n_dev && *n_dev < n_max) ? (int64_t)*n_dev : n_max;
    purge_rows(rows, n, n_max, out, count, scratch, kept_out);
}

// ---- a stack of frames: the purge is a per-image rule, so it runs per frame -----------------------------------------------------------
// The frame of every eye row of n faces (left eyes [0, n), right eyes [n, 2n)): the face's original window / n0 (hg_cascade.hip, StagePass::period)
__global__ void k_eye_row_frames(int64_t n, const int32_t* __restrict__ orig_index, int n0, int32_t* __restrict__ row_frame) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t f = orig_index[i] / n0;
    row_frame[i] = f;
    row_frame[n + i] = f;
}

// The assembled rows (k_eyes_glue keeps the survivors' order: by frame) cut into frames: seg_first[f] = first row of frame f,
// seg_first[n_frames] = *count.  Row j's frame: the original window of the survivor it was made from (row_src) / n0.  One workgroup;
// thread j writes the entries of the frames that begin at row j (those without a row included).
__global__ void __launch_bounds__(1024) k_frame_segments(const int32_t* __restrict__ row_src, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ orig_index, int n0, int n_frames, int32_t* __restrict__ seg_first) {
    const int cnt = *count;
    for (int j = threadIdx.x; j <= cnt; j += blockDim.x) {
        const int f_prev = j == 0 ? -1 : orig_index[row_src[j - 1]] / n0;
        const int f_here = j == cnt ? n_frames : orig_index[row_src[j]] / n0;
        for (int f = (f_prev < -1 ? -1 : f_prev) + 1; f <= f_here && f <= n_frames; ++f) seg_first[f] = j;
    }
}

// The two kernels above for a LIST of frames of different sizes (hg_cascade.hip, GRID_LIST): the frame of original window o is
// win_frame[o], the array k_cascade_init_list wrote (n_windows entries) — no division by a common n0.  An index outside the windows is
// frame -1 (k_eye_row_frames_list: an all-zero eye row) or ends the segments (k_frame_segments_list), as an index beyond the stack does.
__global__ void k_eye_row_frames_list(int64_t n, const int32_t* __restrict__ orig_index, const int32_t* __restrict__ win_frame, int n_windows,
                                      int32_t* __restrict__ row_frame) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t o = orig_index[i];
    const int32_t f = o >= 0 && o < n_windows ? win_frame[o] : -1;
    row_frame[i] = f;
    row_frame[n + i] = f;
}
__global__ void __launch_bounds__(1024) k_frame_segments_list(const int32_t* __restrict__ row_src, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ orig_index, const int32_t* __restrict__ win_frame, int n_windows,
                                                              int n_frames, int32_t* __restrict__ seg_first) {
    const int cnt = *count;
    auto frame = [&](int j) -> int {
        const int32_t o = orig_index[row_src[j]];
        return o >= 0 && o < n_windows ? win_frame[o] : n_frames;
    };
    for (int j = threadIdx.x; j <= cnt; j += blockDim.x) {
        const int f_prev = j == 0 ? -1 : frame(j - 1);
        const int f_here = j == cnt ? n_frames : frame(j);
        for (int f = (f_prev < -1 ? -1 : f_prev) + 1; f <= f_here && f <= n_frames; ++f) seg_first[f] = j;
    }
}

// k_purge per frame: workgroup f purges rows [seg_first[f], seg_first[f + 1]).  Frame f's kept rows start at row seg_first[f] + f of
// `out` and its scratch at 16 (seg_first[f] + f) bytes: every frame has room for its count + 1 rows (the first row appended twice).
__global__ void __launch_bounds__(1024) k_purge_frames(const double* __restrict__ rows, const int32_t* __restrict__ seg_first, double* __restrict__ out,
                                                       int32_t* __restrict__ seg_kept, char* __restrict__ scratch) {
    const int f = blockIdx.x;
    const int64_t lo = seg_first[f], n = seg_first[f + 1] - lo;
    purge_rows(rows + lo * 10, n, n, out + (lo + f) * 10, seg_kept + f, scratch + (lo + f) * 16, nullptr);
}

// The same, and for every row frame f keeps its index within the frame's rows (purge_rows' kept_out), at entry seg_first[f] + f onwards
// of kept_idx: what the slots of a stream set's tracked pass are composed of (hg_cascade.hip, k_stream_handover).  A kernel of its own,
// so that k_purge_frames stays the code it was.
__global__ void __launch_bounds__(1024) k_purge_frames_kept(const double* __restrict__ rows, const int32_t* __restrict__ seg_first, double* __restrict__ out,
                                                            int32_t* __restrict__ seg_kept, char* __restrict__ scratch, int32_t* __restrict__ kept_idx) {
    const int f = blockIdx.x;
    const int64_t lo = seg_first[f], n = seg_first[f + 1] - lo;
    purge_rows(rows + lo * 10, n, n, out + (lo + f) * 10, seg_kept + f, scratch + (lo + f) * 16, kept_idx + lo + f);
}

void launch_purge(const double* rows, int64_t n_max, const int32_t* n_dev, double* out, int32_t* count, void* scratch, hipStream_t st,
                  int32_t* kept_out = nullptr) {
    hipLaunchKernelGGL(k_purge, 1, 1024, 0, st, rows, n_max, n_dev, out, count, (char*)scratch, kept_out);
    HG_HIP(hipGetLastError());
}

// The eye step for n faces on the device (n known on the host).  Outputs as in hg_eyes_locate_device; rows / count (nullable): the
// discard and the row assembly as well (conf needed then).  n_dev (nullable): the face count stays on the device and n bounds it —
// every launch is sized by n; k_eye_boxes gives the faces past the live count a defined window, so the extraction, the contrast
// step and the networks read defined data in all 2n rows, and k_eyes_glue assembles the live faces only.
// row_frame (2n entries on the device; a source of several frames): eye row i is cut from frame row_frame[i]
void eyes_run(hg_eyes* e, const hg::FrameSource& src, const double* boxes, const double* angles, const double* conf, int64_t n, double* ecoords, uint8_t* toofar,
              float* patches, double* reg, double* rows, int32_t* count, hipStream_t st, const int32_t* n_dev = nullptr, int32_t* row_src = nullptr,
              const int32_t* row_frame = nullptr) {
    if (n == 0) {
        if (count) HG_HIP(hipMemsetAsync(count, 0, 4, st));
        return;
    }
    e->reserve(n);
    const hg_eye_consts& c = e->c;
    const int64_t wh = (int64_t)c.eye_w * c.eye_h, n2 = 2 * n;
    hipLaunchKernelGGL(k_eye_boxes, (unsigned)((n + 255) / 256), 256, 0, st, n, n_dev, boxes, angles, c, (double*)e->eboxes.p, (double*)e->dang.p);
    HG_HIP(hipGetLastError());
    if (hg::patcher_extract_source(e->patcher, src, 0, hg::RowFrames{row_frame, false, 0}, e->filter, (const double*)e->eboxes.p, (const double*)e->dang.p, n2,
                                   c.eye_w, c.eye_h, e->pu8.p, HG_U8, wh, st) != HG_OK)
        hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    float* pf = patches ? patches : (float*)e->pf32.p;
    hipLaunchKernelGGL(k_eye_contrast, (unsigned)n2, 256, 0, st, (const uint8_t*)e->pu8.p, pf, wh, c.target_mean, c.target_std);
    HG_HIP(hipGetLastError());
    // EyeLX and EyeLY (face_analysis.py:1064-1070): both eyes in one batch, L rows then R rows (rows are independent)
    double* rg = reg ? reg : (double*)e->reg.p;
    const int k = c.n_features;
    if (hg_flow_execute_device(e->fx, pf, HG_F32, n2, wh, e->sl.p, HG_F32, k, k, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    if (e->fy == e->fx) {
        hg_gauss* g[2] = {e->gx, e->gy};
        if (hg_gauss_regression_multi_device(g, 2, e->sl.p, HG_F32, n2, k, rg, n2, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    } else {
        if (hg_flow_execute_device(e->fy, pf, HG_F32, n2, wh, e->sl2.p, HG_F32, k, k, st) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        if (hg_gauss_regression_multi_device(&e->gx, 1, e->sl.p, HG_F32, n2, k, rg, n2, st) != HG_OK ||
            hg_gauss_regression_multi_device(&e->gy, 1, e->sl2.p, HG_F32, n2, k, rg + n2, n2, st) != HG_OK)
            hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    }
    hipLaunchKernelGGL(k_eyes_glue, 1, 1024, 0, st, n, n_dev, c, boxes, angles, conf, (const double*)e->eboxes.p, (const double*)rg, n2, ecoords, toofar,
                       rows, count, row_src);
    HG_HIP(hipGetLastError());
}

}  // namespace

namespace hg {
// The one eye tail (hg_common.hpp).  The reserve comes before any workspace pointer is taken: eyes_run reserves too, but its arguments
// are evaluated first — on a handle's first faces they were null (no rows written, the purge read an uninitialised count) and on growth
// they were the freed buffers.  A per-frame purge reserves n + n_frames: the purged rows and the scratch hold count + 1 per frame.
EyeTail eyes_tail_enqueue(hg_eyes* e, const FrameSource& src, const EyeSurvivors& s, hipStream_t st) {
    const bool per_frame = src.kind != FrameSource::ONE, is_list = src.kind == FrameSource::LIST;
    if (!e) fail(HG_ERR_ARG, "null eye handle");
    if (s.n_dev && s.n < 1) fail(HG_ERR_ARG, "bad bounded eye step");
    if (is_list && (!src.list || !src.list->host || !src.list->dev || !src.list->win_frame_dev)) fail(HG_ERR_ARG, "null argument");
    if (per_frame && (src.n_frames < 1 || (!is_list && s.period < 1))) fail(HG_ERR_ARG, "bad frame stack");
    const int64_t n = s.n;
    const int n_frames = per_frame ? src.n_frames : 0;
    if (n == 0) return EyeTail{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_frames, 0};
    e->reserve(n + n_frames);
    int32_t *seg_first = nullptr, *seg_kept = nullptr, *row_frame = nullptr;
    int32_t* row_src = per_frame || s.n_dev ? (int32_t*)e->row_src.p : nullptr;
    int32_t* kept_idx = s.n_dev ? (int32_t*)e->kept_idx.p : nullptr;
    const int32_t* count = (const int32_t*)e->count.p;
    if (per_frame) {
        e->row_frame.alloc((size_t)n * 2 * 4);
        e->seg.alloc((size_t)(2 * n_frames + 1) * 4);
        row_frame = (int32_t*)e->row_frame.p;
        seg_first = (int32_t*)e->seg.p;
        seg_kept = seg_first + n_frames + 1;
        if (is_list)
            hipLaunchKernelGGL(k_eye_row_frames_list, (unsigned)((n + 255) / 256), 256, 0, st, n, s.orig_index, src.list->win_frame_dev, (int)src.list->n_windows,
                               row_frame);
        else
            hipLaunchKernelGGL(k_eye_row_frames, (unsigned)((n + 255) / 256), 256, 0, st, n, s.orig_index, (int)s.period, row_frame);
        HG_HIP(hipGetLastError());
    }
    eyes_run(e, src, s.boxes, s.angles, s.conf, n, nullptr, nullptr, nullptr, nullptr, (double*)e->rows.p, (int32_t*)e->count.p, st, s.n_dev, row_src, row_frame);
    if (!per_frame) {
        launch_purge((const double*)e->rows.p, n, count, (double*)e->purged.p, (int32_t*)e->count.p + 1, e->scratch.p, st, kept_idx);
    } else {
        if (is_list)
            hipLaunchKernelGGL(k_frame_segments_list, 1, 1024, 0, st, (const int32_t*)row_src, count, s.orig_index, src.list->win_frame_dev,
                               (int)src.list->n_windows, n_frames, seg_first);
        else
            hipLaunchKernelGGL(k_frame_segments, 1, 1024, 0, st, (const int32_t*)row_src, count, s.orig_index, (int)s.period, n_frames, seg_first);
        if (kept_idx)
            hipLaunchKernelGGL(k_purge_frames_kept, (unsigned)n_frames, 1024, 0, st, (const double*)e->rows.p, (const int32_t*)seg_first, (double*)e->purged.p,
                               seg_kept, (char*)e->scratch.p, kept_idx);
        else
            hipLaunchKernelGGL(k_purge_frames, (unsigned)n_frames, 1024, 0, st, (const double*)e->rows.p, (const int32_t*)seg_first, (double*)e->purged.p, seg_kept,
                               (char*)e->scratch.p);
        HG_HIP(hipGetLastError());
    }
    return EyeTail{(const double*)e->purged.p, count, seg_first, seg_kept, row_src, kept_idx, n_frames, n};
}

void eyes_tail_read(hg_eyes* e, const EyeTail& t, double* out_rows, int64_t out_cap, int64_t* n_out, int64_t* n_before_purge, hipStream_t st) {
    *n_out = 0;
    if (n_before_purge) *n_before_purge = 0;
    if (t.n == 0) return;
    HG_HIP(hipMemcpyAsync(e->host_words, t.counts, 8, hipMemcpyDeviceToHost, st));
    HG_HIP(hipStreamSynchronize(st));
    const int64_t kept = e->host_words[1];
    if (n_before_purge) *n_before_purge = e->host_words[0];
    if (kept > out_cap) fail(HG_ERR_ARG, "%lld faces but room for %lld", (long long)kept, (long long)out_cap);
    if (kept > 0) {
        if (!out_rows) fail(HG_ERR_ARG, "null output rows");
        HG_HIP(hipMemcpyAsync(out_rows, t.purged, (size_t)kept * 80, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
    }
    *n_out = kept;
}

// (the bounds of the segment words and the placement of the rows are host-only code: hg_frame_list.hpp)
void eyes_tail_read_frames(const EyeTail& t, double* out_rows, int64_t out_cap, int32_t* frame_first, int32_t* n_before_purge, hipStream_t st) {
    if (!frame_first) fail(HG_ERR_ARG, "null argument");
    for (int f = 0; f <= t.n_frames; ++f) frame_first[f] = 0;
    for (int f = 0; f < t.n_frames && n_before_purge; ++f) n_before_purge[f] = 0;
    if (t.n == 0) return;
    std::vector<int32_t> seg((size_t)2 * t.n_frames + 1);
    std::vector<double> purged((size_t)(t.n + t.n_frames) * 10);
    HG_HIP(hipMemcpyAsync(seg.data(), t.seg_first, seg.size() * 4, hipMemcpyDeviceToHost, st));
    HG_HIP(hipMemcpyAsync(purged.data(), t.purged, purged.size() * 8, hipMemcpyDeviceToHost, st));      // (rows no frame wrote are never looked at)
    HG_HIP(hipStreamSynchronize(st));
    int64_t kept = 0;
    const std::string bad = tail_segments_refusal(seg.data(), t.n_frames, t.n, &kept);
    if (!bad.empty()) fail(HG_ERR_STATE, "%s", bad.c_str());
    if (kept > out_cap) fail(HG_ERR_ARG, "%lld faces but room for %lld", (long long)kept, (long long)out_cap);
    if (kept > 0 && !out_rows) fail(HG_ERR_ARG, "null output rows");
    tail_place(seg.data(), purged.data(), t.n_frames, out_rows, frame_first, n_before_purge);
}

int eyes_device(const hg_eyes* e) { return e ? e->device : -1; }
int eyes_filter(const hg_eyes* e) { return e ? e->filter : HG_FILTER_NEAREST; }
}  // namespace hg

extern "C" {

int hg_eyes_create(hg_flow* flow_x, hg_gauss* clf_x, hg_flow* flow_y, hg_gauss* clf_y, const hg_eye_consts* consts, int device, hg_eyes** out) {
    return guarded([&] {
        if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
        *out = nullptr;
        // in argument order: constants, flows (shape, then device), classifiers — like hg_cascade_create
        if (!consts) hg::fail(HG_ERR_ARG, "null constants");
        const hg_eye_consts& c = *consts;
        if (c.eye_w <= 0 || c.eye_h <= 0 || (int64_t)c.eye_w * c.eye_h > 65536)
            hg::fail(HG_ERR_ARG, "bad eye patch size %d x %d (at most 65536 pixels: N S2 stays exact in a double)", c.eye_w, c.eye_h);
        if (c.n_features <= 0 || c.n_features > 256) hg::fail(HG_ERR_ARG, "bad feature count %d", c.n_features);
        if (!(c.eye_regression_width > 0.0) || !(c.eye_regression_height > 0.0) || !(c.eye_sampling > 0.0) || !(c.face_sampling > 0.0) ||
            !(c.target_std > 0.0) || !std::isfinite(c.target_mean) || !std::isfinite(c.tolerance))
            hg::fail(HG_ERR_ARG, "bad eye constants");
        if (!flow_x || !flow_y) hg::fail(HG_ERR_ARG, "null eye flow");
        for (hg_flow* f : {flow_x, flow_y}) {
            hg_info info{};
            if (hg_flow_info(f, &info) != HG_OK) hg::fail(HG_ERR_ARG, "%s", hg_last_error());
            if (info.input_dim != (int64_t)c.eye_w * c.eye_h)
                hg::fail(HG_ERR_DIM, "eye flow reads %lld columns, patches have %d x %d", (long long)info.input_dim, c.eye_w, c.eye_h);
            if (info.output_dim < c.n_features) hg::fail(HG_ERR_DIM, "eye flow gives %lld features, %d kept", (long long)info.output_dim, c.n_features);
            if (info.device != device) hg::fail(HG_ERR_ARG, "eye flow lives on device %d, not %d", info.device, device);
        }
        if (!clf_x || !clf_y) hg::fail(HG_ERR_ARG, "null eye classifier");
        for (hg_gauss* g : {clf_x, clf_y}) {
            const hg::GaussParams P = hg::gauss_params(g);
            if (P.d > c.n_features) hg::fail(HG_ERR_DIM, "eye classifier reads %d features, %d kept", P.d, c.n_features);
        }
        set_dev(device);
        auto e = std::make_unique<hg_eyes>();
        e->device = device;
        e->fx = flow_x; e->fy = flow_y; e->gx = clf_x; e->gy = clf_y;
        e->c = c;
        if (hg_patcher_create(device, &e->patcher) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        HG_HIP(hipHostMalloc((void**)&e->host_words, 64, hipHostMallocDefault));
        *out = e.release();
    });
}

int hg_eyes_set_interpolation(hg_eyes* e, int filter) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null eye handle");
        if (filter != HG_FILTER_NEAREST && filter != HG_FILTER_BILINEAR && filter != HG_FILTER_BICUBIC)
            hg::fail(HG_ERR_ARG, "unknown interpolation filter %d (0 NEAREST, 2 BILINEAR, 3 BICUBIC)", filter);
        e->filter = filter;
    });
}

void hg_eyes_free(hg_eyes* e) {
    if (!e) return;
    if (hipSetDevice(e->device) == hipSuccess) {
        if (e->patcher) hg_patcher_free(e->patcher);
        if (e->host_words) (void)hipHostFree(e->host_words);
    }
    delete e;
}

int hg_eyes_locate_device(hg_eyes* e, const void* frame_dev, int frame_h, int frame_w, int64_t ld, const double* boxes_dev, const double* angles_dev,
                          int64_t n, double* eye_coords_dev, uint8_t* too_far_dev, float* patches_dev, double* reg_dev, void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null eye handle");
        if (n < 0 || n > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "bad face count");
        if (n > 0 && (!frame_dev || !boxes_dev || !angles_dev || !eye_coords_dev || !too_far_dev)) hg::fail(HG_ERR_ARG, "null data pointer");
        if (frame_h <= 0 || frame_w <= 0 || ld < frame_w) hg::fail(HG_ERR_ARG, "bad frame shape");
        set_dev(e->device);
        eyes_run(e, hg::FrameSource::one(frame_dev, frame_h, frame_w, ld), boxes_dev, angles_dev, nullptr, n, eye_coords_dev, too_far_dev, patches_dev, reg_dev,
                 nullptr, nullptr, (hipStream_t)stream);
    });
}

int hg_eyes_boxes_device(hg_eyes* e, const double* boxes_dev, const double* angles_dev, int64_t n, double* eye_boxes_dev, double* delta_angs_dev,
                         void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null eye handle");
        if (n < 0 || n > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "bad face count");
        if (n > 0 && (!boxes_dev || !angles_dev || !eye_boxes_dev)) hg::fail(HG_ERR_ARG, "null data pointer");
        set_dev(e->device);
        if (n == 0) return;
        hipLaunchKernelGGL(k_eye_boxes, (unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream, n, (const int32_t*)nullptr, boxes_dev, angles_dev, e->c, eye_boxes_dev,
                           delta_angs_dev);
        HG_HIP(hipGetLastError());
    });
}

int hg_purge_detections_device(int device, const double* rows_dev, int64_t n, double* out_rows_dev, int32_t* count_dev, void* stream) {
    return guarded([&] {
        if (n < 0 || n > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "bad row count");
        if (!count_dev || (n > 0 && (!rows_dev || !out_rows_dev))) hg::fail(HG_ERR_ARG, "null data pointer");
        set_dev(device);
        hipStream_t st = (hipStream_t)stream;
        hg::DevBuf scratch;
        scratch.alloc((size_t)(n + 1) * 16);
        launch_purge(rows_dev, n, nullptr, out_rows_dev, count_dev, scratch.p, st);
        HG_HIP(hipStreamSynchronize(st));      // the scratch buffer lives until here
    });
}

}  // extern "C"
