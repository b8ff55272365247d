// Cascade glue on the device: what the reference's stage loop does between two calls of the hot path,
//     reg_out = classifiers[k].regression(sl[:, 0:d], avg_labels)                          FaceDetectUpdated.py:719
//     curr_subimage_coordinates, curr_angles = update_current_subimage_coordinates(...)    :728   (face_analysis.py:803-840)
//     new_wrong_images = identify_patches_to_discard(...)                                  :733   (face_analysis.py:842-887)
//     boolean-mask compaction of coordinates, angles, indices, sl, subimages_arr           :739-759
// so that extract -> execute -> regression -> update -> discard -> compaction chain on one stream without a host copy of any
// per-candidate array (the host reads back ONE integer, the survivor count, where it needs a launch size).
// All arithmetic is float64 in the reference's operation order, compiled without contraction (see the pragma below), so
// coordinates follow the numpy path bit for bit given the same regression outputs.  Candidates of all pyramid levels may share one batch (the author's note
// FaceDetectUpdated.py:599): the per-level constants max_Dx_diff, max_Dy_diff, base_side travel per ORIGINAL window.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "hg_common.hpp"
#include "hg_frame_format.hpp"
#include "hg_frame_list.hpp"
#include "hg_gauss_dev.hpp"

namespace hg { void set_last_error(const std::string& s); }

// No contraction anywhere below (hg_gauss_dev.hpp, the regression, is included above and keeps the build's default): under hipcc's
// -ffp-contract=fast-honor-pragmas the __dadd_rn / __dmul_rn of the HIP headers are plain operators, so `oa + net_Dang * tol` or
// `dx * dx + dy * dy` could become one fma and move a discard decision that sits on its threshold by one ulp.  The helpers are defined
// under the pragma: each operation rounds on its own, as numpy's do (tests/test_fp_contract.py checks the fma count).
#pragma clang fp contract(off)
namespace {
__device__ __forceinline__ double d_add(double a, double b) { return a + b; }
__device__ __forceinline__ double d_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double d_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double d_div(double a, double b) { return a / b; }

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

// One candidate through one stage: update_current_subimage_coordinates (face_analysis.py:803-840; Disc leaves the window as it is)
// and identify_patches_to_discard (:842-887).  Returns the discard flag.  k_cascade_update and the group launches share it.
__device__ __forceinline__ bool update_one(int type, const hg_cascade_consts& c, double& x0, double& y0, double& x1, double& y1, double& ang,
                                            double r, const double* oc, double oa, const double* lvl) {
    switch (type) {
        case HG_STAGE_DISC: return r >= c.cut_off_face;
        case HG_STAGE_POSX: {
            const double ro = d_div(d_mul(r, d_sub(x1, x0)), c.regression_width);
            x0 = d_sub(x0, ro);
            x1 = d_sub(x1, ro);
            const double d = d_sub(d_div(d_add(x1, x0), 2.0), d_div(d_add(oc[2], oc[0]), 2.0));
            return fabs(d) > d_mul(lvl[0], c.tolerance_posxy_deviation);
        }
        case HG_STAGE_POSY: {
            const double ro = d_div(d_mul(r, d_sub(y1, y0)), c.regression_height);
            y0 = d_sub(y0, ro);
            y1 = d_sub(y1, ro);
            const double d = d_sub(d_div(d_add(y1, y0), 2.0), d_div(d_add(oc[3], oc[1]), 2.0));
            return fabs(d) > d_mul(lvl[1], c.tolerance_posxy_deviation);
        }
        case HG_STAGE_PANG: {
            ang = d_add(ang, r);
            const double lim = d_mul(c.net_Dang, c.tolerance_angle_deviation);
            return ang > d_add(oa, lim) || ang < d_sub(oa, lim);
        }
        default: {
            const double ow = d_sub(x1, x0), oh = d_sub(y1, y0);
            const double xc = d_div(d_add(x1, x0), 2.0), yc = d_div(d_add(y1, y0), 2.0);
            const double w = d_mul(d_div(ow, r), c.desired_sampling), h = d_mul(d_div(oh, r), c.desired_sampling);
            x0 = d_sub(xc, d_div(w, 2.0));
            x1 = d_add(xc, d_div(w, 2.0));
            y0 = d_sub(yc, d_div(h, 2.0));
            y1 = d_add(yc, d_div(h, 2.0));
            const double dx = d_sub(x0, x1), dy = d_sub(y0, y1);
            const double ratio = d_div(__dsqrt_rn(d_add(d_mul(dx, dx), d_mul(dy, dy))), lvl[2]);
            return ratio > d_mul(c.max_scale_radio, c.tolerance_scale_deviation) || ratio < d_div(c.min_scale_radio, c.tolerance_scale_deviation);
        }
    }
}

__global__ void k_cascade_update(int type, hg_cascade_consts c, int64_t n, double* __restrict__ coords, double* __restrict__ angles,
                                 const double* __restrict__ reg, const int32_t* __restrict__ orig_index, const double* __restrict__ orig_coords,
                                 const double* __restrict__ orig_angles, const double* __restrict__ orig_level, uint8_t* __restrict__ discard) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x0 = coords[i * 4], y0 = coords[i * 4 + 1], x1 = coords[i * 4 + 2], y1 = coords[i * 4 + 3], ang = angles[i];
    const int32_t oi = orig_index[i];
    const bool wrong = update_one(type, c, x0, y0, x1, y1, ang, reg[i], orig_coords + (size_t)oi * 4, orig_angles[oi], orig_level + (size_t)oi * 3);
    coords[i * 4] = x0; coords[i * 4 + 1] = y0; coords[i * 4 + 2] = x1; coords[i * 4 + 3] = y1;
    angles[i] = ang;
    discard[i] = wrong ? 1 : 0;
}

// map[j] = index of the j-th kept row, *count = number of kept rows.  One workgroup walks the flags in chunks of its size
// with a running offset (a real frame has <= a few thousand candidates: one or two chunks).
__global__ void __launch_bounds__(1024) k_cascade_compact(const uint8_t* __restrict__ discard, int64_t n, int32_t* __restrict__ map,
                                                           int32_t* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += blockDim.x) {
        const int64_t i = i0 + tid;
        const int keep = (i < n && discard[i] == 0) ? 1 : 0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) map[off + before] = (int32_t)i;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// dst[j, :] = src[map[j], :] for j < *count; rows of row_bytes bytes (multiple of 4), 16-byte vectors where alignment allows.
__global__ void __launch_bounds__(256) k_gather_rows(const char* __restrict__ src, char* __restrict__ dst, int64_t row_bytes,
                                                      const int32_t* __restrict__ map, const int32_t* __restrict__ count, int vec16) {
    const int cnt = *count;
    for (int64_t j = blockIdx.x; j < cnt; j += gridDim.x) {
        const char* s = src + (int64_t)map[j] * row_bytes;
        char* d = dst + j * row_bytes;
        if (vec16) {
            for (int64_t o = (int64_t)threadIdx.x * 16; o < row_bytes; o += (int64_t)blockDim.x * 16) *(int4*)(d + o) = *(const int4*)(s + o);
        } else {
            for (int64_t o = (int64_t)threadIdx.x * 4; o < row_bytes; o += (int64_t)blockDim.x * 4) *(int32_t*)(d + o) = *(const int32_t*)(s + o);
        }
    }
}

// One cascade stage's glue in ONE launch of ONE workgroup (a frame has at most a few thousand candidates): update + discard
// test per candidate (update_one, as k_cascade_update), order-preserving compaction, and the gather of every small
// per-candidate array into the other half of its ping-pong pair.  The candidate count comes from device memory (the previous
// stage's output), so stages chain without a host round trip; the new count goes to device memory and, for the caller that
// wants it, to a pinned host word.
struct StageArrays {
    double *coords[2], *angles[2], *conf[2], *neg_angles;   // [cur / nxt]
    int32_t* oidx[2];
    float* sl[2];
    const double *reg, *orig_coords, *orig_angles, *orig_level;
    uint8_t* discard;
    int32_t* map;
    int32_t *count_in, *count_out;
    int32_t k_feat, cur, n_max;
    int32_t pad_to;      // > 0 (a tracked frame): rows [new count, pad_to) of the nxt arrays get a defined window (k_cascade_group)
};

// What the host polls instead of synchronising the stream (pinned, device-visible): word 0 = survivor count, word 1 = sequence
// number of the stage that wrote it (written last, system scope).  A stream synchronisation costs the caller 20-40 us before it
// has caught up with the device again; a poll sees the word 2-3 us after the store.
__device__ __forceinline__ void publish_count(int32_t* host_count, int cnt, int seq) {
    host_count[0] = cnt;
    __threadfence_system();
    __hip_atomic_store(host_count + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The final survivors for the host, written by the last stage's kernel into pinned memory (a handful of rows): the call ends with
// a poll of the count word instead of four device-to-host copies and a stream synchronisation.
struct HostResults {
    double* coords;      // [cap][4]
    double* angles;      // [cap]
    double* conf;        // [cap]
    int32_t* oidx;       // [cap]
    int32_t cap;
};

// Start of a frame: candidate i = original window i (the host copied the boxes into orig_coords); replaces five small copies /
// memsets and the synchronisation that kept their host temporaries alive.
__global__ void k_cascade_init(int n, const double* __restrict__ orig_coords, double* __restrict__ coords, double* __restrict__ angles,
                               double* __restrict__ neg, double* __restrict__ conf, int32_t* __restrict__ oidx, int32_t* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = n;
    if (i >= n) return;
    for (int q = 0; q < 4; ++q) coords[(size_t)i * 4 + q] = orig_coords[(size_t)i * 4 + q];
    angles[i] = 0.0;
    neg[i] = 0.0;
    conf[i] = 0.0;
    oidx[i] = i;
}

// The same start with the windows computed HERE from the grid's closed form (round 5; the boxes and level constants of a 1080p
// frame were 97 KB of pageable host memory copied per frame): level L holds ny x nx windows, y-major, at
// numpy.linspace(0, stop, n) positions — i * (stop / (n - 1)), the last one `stop` itself, a single one 0.0 — and a window is
// (posX, posY, posX + pw - 1, posY + ph - 1)  (face_analysis.py:630-646, :661-669; grid.level_boxes).  float64 in numpy's
// operation order, no contraction (pragma above): the boxes equal the host's bit for bit (tests/test_cascade.py).
constexpr int kMaxLevels = 32;
struct LevelTable {
    int32_t n_levels, pad;
    int32_t first[kMaxLevels + 1];      // first window of every level, and the total
    hg_cascade_level lv[kMaxLevels];
};

// Window i of the grid of T: its box into b[0..4), and its level (shared by k_cascade_init_grid and k_cascade_init_list: one arithmetic)
__device__ __forceinline__ const hg_cascade_level& grid_window(const LevelTable& T, int i, double* b) {
    int L = 0;
    while (L + 1 < T.n_levels && i >= T.first[L + 1]) ++L;
    const hg_cascade_level& V = T.lv[L];
    const int k = i - T.first[L], iy = k / V.nx, ix = k - iy * V.nx;
    auto lin = [](int j, int num, double stop) -> double {
        if (num <= 1 || j == 0) return 0.0;
        if (j == num - 1) return stop;
        return d_mul((double)j, d_div(stop, (double)(num - 1)));
    };
    const double x0 = lin(ix, V.nx, V.x_stop), y0 = lin(iy, V.ny, V.y_stop);
    b[0] = x0;
    b[1] = y0;
    b[2] = d_sub(d_add(x0, V.patch_w), 1.0);
    b[3] = d_sub(d_add(y0, V.patch_h), 1.0);
    return V;
}

__global__ void k_cascade_init_grid(LevelTable T, double* __restrict__ orig_coords, double* __restrict__ orig_level, double* __restrict__ coords,
                                    double* __restrict__ angles, double* __restrict__ neg, double* __restrict__ conf, int32_t* __restrict__ oidx,
                                    int32_t* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = T.first[T.n_levels];
    if (i == 0 && count) *count = n;
    if (i >= n) return;
    double b[4];
    const hg_cascade_level& V = grid_window(T, i, b);
    for (int q = 0; q < 4; ++q) orig_coords[(size_t)i * 4 + q] = b[q];
    orig_level[(size_t)i * 3] = V.max_dx;
    orig_level[(size_t)i * 3 + 1] = V.max_dy;
    orig_level[(size_t)i * 3 + 2] = V.base_side;
    if (coords) {
        for (int q = 0; q < 4; ++q) coords[(size_t)i * 4 + q] = b[q];
        angles[i] = 0.0;
        neg[i] = 0.0;
        conf[i] = 0.0;
        oidx[i] = i;
    }
}

// The start of a STACK of same-size frames (hg_cascade_detect_frames_device), after k_cascade_init_grid has laid out ONE frame's grid:
// window f * n0 + j is window j of frame f — the same box and level constants, a candidate index of its own, from which the frame of a
// row follows wherever it travels (index / n0).  Rows [n0, n) are written from rows [0, n0), which this kernel only reads.
__global__ void k_cascade_init_frames(int n0, int n, double* __restrict__ orig_coords, double* __restrict__ orig_level, double* __restrict__ coords,
                                      double* __restrict__ angles, double* __restrict__ neg, double* __restrict__ conf, int32_t* __restrict__ oidx,
                                      int32_t* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = n;
    if (i < n0 || i >= n) return;
    const int j = i % n0;
    for (int q = 0; q < 4; ++q) {
        const double v = orig_coords[(size_t)j * 4 + q];
        orig_coords[(size_t)i * 4 + q] = v;
        coords[(size_t)i * 4 + q] = v;
    }
    for (int q = 0; q < 3; ++q) orig_level[(size_t)i * 3 + q] = orig_level[(size_t)j * 3 + q];
    angles[i] = 0.0;
    neg[i] = 0.0;
    conf[i] = 0.0;
    oidx[i] = i;
}

// The start of a LIST of frames of different sizes (hg_cascade_detect_frame_list_device): the candidates are the concatenation of the
// frames' grids — window desc[f].first + j is window j of frame f, laid out by grid_window from frame f's level table, tables[grid_of[f]]
// (one table per DISTINCT grid) — and win_frame[i] = f, the frame of original window i, which every later kernel that needs a row's frame
// reads through the row's original index.  first[] ascends strictly (a grid has at least one window): a binary search per thread.
__global__ void k_cascade_init_list(const LevelTable* __restrict__ tables, const hg::FrameDesc* __restrict__ desc, const int32_t* __restrict__ grid_of,
                                    int n_frames, int n, double* __restrict__ orig_coords, double* __restrict__ orig_level, double* __restrict__ coords,
                                    double* __restrict__ angles, double* __restrict__ neg, double* __restrict__ conf, int32_t* __restrict__ oidx,
                                    int32_t* __restrict__ count, int32_t* __restrict__ win_frame) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = n;
    if (i >= n) return;
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].first <= i) lo = mid;
        else hi = mid - 1;
    }
    double b[4];
    const hg_cascade_level& V = grid_window(tables[grid_of[lo]], i - desc[lo].first, b);
    for (int q = 0; q < 4; ++q) {
        orig_coords[(size_t)i * 4 + q] = b[q];
        coords[(size_t)i * 4 + q] = b[q];
    }
    orig_level[(size_t)i * 3] = V.max_dx;
    orig_level[(size_t)i * 3 + 1] = V.max_dy;
    orig_level[(size_t)i * 3 + 2] = V.base_side;
    angles[i] = 0.0;
    neg[i] = 0.0;
    conf[i] = 0.0;
    oidx[i] = i;
    win_frame[i] = lo;
}

// The start of a TRACKED frame (the reference's track_single_face branch with a face found on the previous frame): nine windows from
// the four doubles of the tracked box, which the previous frame's last kernel left in device memory — one sampling value from the
// box's size (face_analysis.py:576-585), posX = (x0, x0 + sepx, x0 - sepx), posY = (y0, y0, y0) (:611-623), their product y-major
// (:661-669: the three distinct windows, three times), the level constants (:650-651, FaceDetectUpdated.py:603-604).  float64 in the
// reference's operation order, no contraction (pragma above): equal to grid.tracked_boxes / cascade.tracked_windows and to the
// reference's own outputs bit for bit (tests/golden/reference_tracking.npz).  One workgroup; writes what k_cascade_init_grid writes.
constexpr int kTracked = 9;
// window i (0..8) of the face at face[0..3], written as row o of the outputs
__device__ __forceinline__ void tracked_window(const hg_tracked_consts& t, const double* __restrict__ face, int i, int o, double* __restrict__ orig_coords,
                                               double* __restrict__ orig_level, double* __restrict__ coords, double* __restrict__ angles,
                                               double* __restrict__ neg, double* __restrict__ conf, int32_t* __restrict__ oidx) {
    const double fx0 = face[0], fy0 = face[1], fx1 = face[2], fy1 = face[3];
    const double face_size = d_add(d_mul(0.5, fabs(d_sub(fx1, fx0))), d_mul(0.5, fabs(d_sub(fy1, fy0))));      // :582
    const double s = d_div(d_mul(face_size, 1.0), t.subimage_width);                                                // :583
    const double pw = d_mul(t.subimage_width, s), ph = d_mul(t.subimage_height, s);                                   // :612-613
    const double sepx = d_div(d_mul(d_mul(t.net_Dx, 2.0), pw), t.regression_width);                               // :615
    const int ix = i % 3;                                                                                                // y-major, three per row
    const double x0 = ix == 0 ? fx0 : (ix == 1 ? d_add(fx0, sepx) : d_sub(fx0, sepx)), y0 = fy0;                   // :622-623
    const double b[4] = {x0, y0, d_sub(d_add(x0, pw), 1.0), d_sub(d_add(y0, ph), 1.0)};                       // :668
    for (int q = 0; q < 4; ++q) orig_coords[(size_t)o * 4 + q] = b[q];
    orig_level[(size_t)o * 3] = d_div(d_mul(t.net_Dx, pw), t.regression_width);                                      // :650
    orig_level[(size_t)o * 3 + 1] = d_div(d_mul(t.net_Dy, ph), t.regression_height);                                 // :651
    orig_level[(size_t)o * 3 + 2] = __dsqrt_rn(d_add(d_mul(pw, pw), d_mul(ph, ph)));                            // FaceDetectUpdated.py:603-604
    if (coords) {
        for (int q = 0; q < 4; ++q) coords[(size_t)o * 4 + q] = b[q];
        angles[o] = 0.0;
        neg[o] = 0.0;
        conf[o] = 0.0;
        oidx[o] = o;
    }
}

__global__ void k_cascade_init_tracked(hg_tracked_consts t, const double* __restrict__ face, double* __restrict__ orig_coords, double* __restrict__ orig_level,
                                       double* __restrict__ coords, double* __restrict__ angles, double* __restrict__ neg, double* __restrict__ conf,
                                       int32_t* __restrict__ oidx, int32_t* __restrict__ count) {
    const int i = threadIdx.x;
    if (i == 0 && count) *count = kTracked;
    if (i >= kTracked) return;
    tracked_window(t, face, i, i, orig_coords, orig_level, coords, angles, neg, conf, oidx);
}

// The same start for K held faces (what every tracker's frame launches; K = 1 under max_faces = 1): window 9 s + i is window i of face s, faces (K, 4) on the device in the
// order the previous frame's hand-over carried them.  K is known on the host (the previous step's one wait fetched it), so the launch
// holds 9 K windows exactly and the count word is 9 K: no filler row at the first stage.  Rows are independent, so the nine windows
// of a face are the bits k_cascade_init_tracked writes for that face alone.
__global__ void __launch_bounds__(64) k_cascade_init_tracked_multi(hg_tracked_consts t, const double* __restrict__ faces, int n_faces,
                                                                   double* __restrict__ orig_coords, double* __restrict__ orig_level,
                                                                   double* __restrict__ coords, double* __restrict__ angles, double* __restrict__ neg,
                                                                   double* __restrict__ conf, int32_t* __restrict__ oidx, int32_t* __restrict__ count) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x, n = kTracked * n_faces;
    if (o == 0 && count) *count = n;
    if (o >= n) return;
    const int s = o / kTracked;
    tracked_window(t, faces + (size_t)s * 4, o - s * kTracked, o, orig_coords, orig_level, coords, angles, neg, conf, oidx);
}

// The last kernel of a tracker's frame: the purged rows become the tracked faces (FaceDetectUpdated.py:1189-1195, row 0 there).
// Candidates are the first min(kept, max_faces) rows; those whose four box numbers are all finite are carried, in purge order, compacted
// into the tracker's device state, where the next frame's k_cascade_init_tracked_multi reads them; the carried count goes beside them.
// With max_faces = 1 that is row 0 or nothing.  For a tracked frame everything the host needs goes to pinned memory: the kept rows, the
// two counts, the carried count, a slot per kept row and, last, the sequence number the host waits for.
// counts: {faces after the discard, faces after the purge}.
// slot[j]: the held face (index in the previous hand-over's carried order) whose nine windows kept row j came from — kept row -> the
// assembled row it is (k_purge's kept[]) -> the cascade survivor that row was made from (k_eyes_glue) -> its original window / 9.  The
// purge may append its first row a second time; both copies have the same kept[] entry, so the same slot.
struct TrackerResults {
    int32_t* words;      // pinned: {kept, before the purge, carried, sequence number}; null: no read-back (the host has the rows already)
    double* rows;        // pinned: [cap][10]
    int32_t* slots;      // pinned: [cap]
    int32_t cap;
};
struct SlotChain {
    const int32_t *kept_idx, *row_src, *oidx;
};
constexpr int kMaxFaces = 64;      // one wave's ballot compacts the candidates; 576 windows stay inside k_cascade_group's single-workgroup path
__global__ void __launch_bounds__(128) k_tracker_handover(const double* __restrict__ purged, const int32_t* __restrict__ counts, double* __restrict__ boxes,
                                                          int32_t* __restrict__ held, int max_faces, SlotChain S, TrackerResults R, int seq) {
    __shared__ int carried_s;
    const int tid = threadIdx.x;
    const int kept = counts[1];
    const int ncand = kept < max_faces ? kept : max_faces;
    if (tid < 64) {      // the first wave: max_faces <= 64
        bool ok = tid < ncand;
        if (ok)
            for (int q = 0; q < 4; ++q) ok = ok && isfinite(purged[(size_t)tid * 10 + q]);
        const unsigned long long m = __ballot(ok ? 1 : 0);
        if (ok) {
            const int pos = __popcll(m & ((1ull << tid) - 1ull));
            for (int q = 0; q < 4; ++q) boxes[(size_t)pos * 4 + q] = purged[(size_t)tid * 10 + q];
        }
        if (tid == 0) {
            carried_s = __popcll(m);
            *held = carried_s;
        }
    }
    if (!R.words) return;
    const int nrow = kept < R.cap ? kept : R.cap;
    for (int q = tid; q < nrow * 10; q += blockDim.x) R.rows[q] = purged[q];
    for (int j = tid; j < nrow; j += blockDim.x) R.slots[j] = S.oidx[S.row_src[S.kept_idx[j]]] / kTracked;
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        R.words[0] = kept;
        R.words[1] = counts[0];
        R.words[2] = carried_s;
        __threadfence_system();
        __hip_atomic_store(R.words + 3, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- a SET of streams tracked in one pooled pass (hg_stream_tracker) ------------------------------------------------------------------
// The start of the tracked pass: the nine windows of every held face of every stream, from the set's device state — faces
// (n_streams, max_faces, 4) and held (n_streams) counts, clamped to 0 .. max_faces.  Original window o = s * 9 * max_faces + 9 j + i is
// window i of held face j of stream s: orig_coords / orig_level are indexed by o with a fixed period per stream, so a row's stream is
// o / (9 max_faces) wherever it travels — the divisor the stack machinery divides by already (StagePass::period, FrameSel::div,
// k_eye_row_frames, k_frame_segments) — and its slot (o % (9 max_faces)) / 9.  The entries of faces not held are holes: never written,
// never read.  The candidate arrays (coords .. oidx, nullable as everywhere) get the live rows COMPACTED, in order of o, with
// oidx = o, and *count their number, 9 * sum of held: exactly the host's bound, no filler row at the first stage.  Every window comes
// from tracked_window(): the bits k_cascade_init_tracked_multi writes for that face.  One workgroup of 1024 threads (n_streams <= 1024:
// one thread per stream scans the counts; the windows are walked in steps of the workgroup's size).
__global__ void __launch_bounds__(1024) k_cascade_init_tracked_streams(hg_tracked_consts t, const double* __restrict__ faces, const int32_t* __restrict__ held,
                                                                       int n_streams, int max_faces, double* orig_coords, double* orig_level,
                                                                       double* __restrict__ coords, double* __restrict__ angles, double* __restrict__ neg,
                                                                       double* __restrict__ conf, int32_t* __restrict__ oidx, int32_t* __restrict__ count) {
    __shared__ int first[1025];      // first[s]: held faces of the streams before s; first[n_streams]: all
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int h = 0;
    if (tid < n_streams) {
        h = held[tid];
        h = h < 0 ? 0 : (h > max_faces ? max_faces : h);
    }
    int incl = h;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (tid < n_streams) first[tid] = off + incl - h;
    if (tid == n_streams - 1) first[n_streams] = off + incl;
    __syncthreads();
    if (tid == 0 && count) *count = kTracked * first[n_streams];
    const int per = kTracked * max_faces;
    const int64_t n = (int64_t)per * n_streams;
    for (int64_t o = tid; o < n; o += blockDim.x) {
        const int s = (int)(o / per), r = (int)(o - (int64_t)s * per), j = r / kTracked, i = r - j * kTracked;
        if (j >= first[s + 1] - first[s]) continue;
        tracked_window(t, faces + ((size_t)s * max_faces + j) * 4, i, (int)o, orig_coords, orig_level, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (coords) {
            const size_t p = (size_t)kTracked * (first[s] + j) + i;
            for (int q = 0; q < 4; ++q) coords[p * 4 + q] = orig_coords[(size_t)o * 4 + q];
            angles[p] = 0.0;
            neg[p] = 0.0;
            conf[p] = 0.0;
            oidx[p] = (int32_t)o;
        }
    }
}

// The hand-over of a stream set, one workgroup per segment f of a per-frame purge (k_purge_frames / k_purge_frames_kept: segment f's kept
// rows start at row seg_first[f] + f of `purged`, seg_kept[f] of them, from seg_first[f + 1] - seg_first[f] assembled rows).  The
// segment belongs to stream stream_of[f] (null: f) and k_tracker_handover's rule runs on it: the first min(kept, max_faces) rows with
// a finite box are carried, in order, into that stream's boxes of the state, their count beside them.  With R.words (the tracked pass)
// everything the host needs goes to the stream's part of pinned memory: words {kept, before the purge, carried, 0}, the kept rows
// (R.cap per stream) and a slot per kept row, kept row -> assembled row (S.kept_idx, relative to the segment) -> cascade survivor
// (S.row_src) -> original window (S.oidx), whose position within its stream's period of `per` windows / 9 is the held face.
// The sequence word is NOT written here: k_publish_seq behind this kernel, in stream order, publishes all workgroups' stores at once.
__global__ void __launch_bounds__(128) k_stream_handover(const double* __restrict__ purged, const int32_t* __restrict__ seg_first,
                                                         const int32_t* __restrict__ seg_kept, const int32_t* __restrict__ stream_of,
                                                         double* __restrict__ boxes, int32_t* __restrict__ held, int max_faces, SlotChain S, int per,
                                                         TrackerResults R) {
    __shared__ int carried_s;
    const int tid = threadIdx.x, f = blockIdx.x;
    const int s = stream_of ? stream_of[f] : f;
    const int lo = seg_first[f], kept = seg_kept[f], before = seg_first[f + 1] - lo;
    const double* rows = purged + (size_t)(lo + f) * 10;
    const int ncand = kept < max_faces ? kept : max_faces;
    if (tid < 64) {      // the first wave: max_faces <= 64
        bool ok = tid < ncand;
        if (ok)
            for (int q = 0; q < 4; ++q) ok = ok && isfinite(rows[(size_t)tid * 10 + q]);
        const unsigned long long m = __ballot(ok ? 1 : 0);
        if (ok) {
            const int pos = __popcll(m & ((1ull << tid) - 1ull));
            for (int q = 0; q < 4; ++q) boxes[((size_t)s * max_faces + pos) * 4 + q] = rows[(size_t)tid * 10 + q];
        }
        if (tid == 0) {
            carried_s = __popcll(m);
            held[s] = carried_s;
        }
    }
    if (!R.words) return;
    const int nrow = kept < R.cap ? kept : R.cap;
    double* out = R.rows + (size_t)s * R.cap * 10;
    int32_t* slots = R.slots + (size_t)s * R.cap;
    for (int q = tid; q < nrow * 10; q += blockDim.x) out[q] = rows[q];
    for (int j = tid; j < nrow; j += blockDim.x) slots[j] = (S.oidx[S.row_src[lo + S.kept_idx[lo + f + j]]] % per) / kTracked;
    __syncthreads();
    if (tid == 0) {
        R.words[s * 4] = kept;
        R.words[s * 4 + 1] = before;
        R.words[s * 4 + 2] = carried_s;
    }
    __threadfence_system();
}

// One thread behind k_stream_handover in stream order: every workgroup's pinned stores are complete when this kernel starts; the
// sequence number the host polls goes out last, at system scope (as k_tracker_handover's).
__global__ void k_publish_seq(int32_t* word, int seq) {
    __threadfence_system();
    __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A GROUP of stages (round 5): a stage that owns a network and the stages behind it whose network is None read the SAME sl
// (FaceDetectUpdated.py:678-682, :704-706; Pipelines/Pipeline_experimental.txt:8-19: PosX owns the flow, PosY / PAng / Scale
// reuse it).  Rows are independent and a discard is per row, so the reference's m rounds of (regression, update, discard,
// compaction) are ONE regression launch on the group's rows (hg_gauss_regression_multi_device: reg[s * stride + i]) and ONE glue
// launch that applies the m updates and discard tests to every row in stage order — a row discarded at stage s takes no part in
// the later ones, exactly as if it had been compacted away — and compacts once: the same survivors in the same order with the
// same bits.  Survivor counts after every stage of the group are still produced (the reference counts them, :707).
constexpr int kMaxGroup = hg::kGaussMaxMulti;
struct GroupDesc {
    int32_t m, pad;
    int32_t type[kMaxGroup];
    double cut[kMaxGroup];      // cut_offs_face[serial] of a Disc stage
};

// candidate i through the group's stages; returns whether it survives all of them, alive_after bit s = alive after stage s
// (requesting the regression values of ALL the group's stages and the original window's nine numbers up front, so that the loads
// overlap, was measured late in round 5: k_cascade_group 62.8 -> 70.1 us per frame — most candidates die at the group's first stage
// and never needed them.  Not kept.)
__device__ __forceinline__ bool group_one(const GroupDesc& G, const hg_cascade_consts& c0, const StageArrays& A, int64_t reg_stride, int i, double& x0,
                                          double& y0, double& x1, double& y1, double& ang, double& cf, int32_t oi, unsigned& alive_after) {
    bool alive = true;
    alive_after = 0;
    for (int s = 0; s < G.m; ++s) {
        if (alive) {
            const double r = A.reg[(size_t)s * reg_stride + i];
            hg_cascade_consts c = c0;
            c.cut_off_face = G.cut[s];
            const bool wrong = update_one(G.type[s], c, x0, y0, x1, y1, ang, r, A.orig_coords + (size_t)oi * 4, A.orig_angles[oi], A.orig_level + (size_t)oi * 3);
            if (G.type[s] == HG_STAGE_DISC) cf = r;      // FaceDetectUpdated.py:758-759
            alive = !wrong;
        }
        alive_after |= (alive ? 1u : 0u) << s;
    }
    return alive;
}

// host_count (pinned): {count, sequence number, survivors after stage 0 .. m-1 of the group}
__device__ __forceinline__ void publish_group(int32_t* host_count, const int* scount, int m, int cnt, int seq) {
    for (int s = 0; s + 1 < m; ++s) host_count[2 + s] = scount[s];
    host_count[2 + m - 1] = cnt;
    publish_count(host_count, cnt, seq);
}

// One workgroup of 1024 threads (a frame has at most a few thousand candidates).
__global__ void __launch_bounds__(1024) k_cascade_group(GroupDesc G, hg_cascade_consts c, StageArrays A, int64_t reg_stride, int32_t* host_count, int seq, HostResults H) {
    __shared__ int wsum[16];
    __shared__ int base;
    __shared__ int scount[kMaxGroup];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(*A.count_in, A.n_max);
    const int cur = A.cur, nxt = 1 - cur;
    if (tid == 0) base = 0;
    if (tid < kMaxGroup) scount[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += blockDim.x) {
        const int i = i0 + tid;
        int keep = 0;
        double x0 = 0, y0 = 0, x1 = 0, y1 = 0, ang = 0, cf = 0;
        int32_t oi = 0;
        unsigned after = 0;
        if (i < n) {
            x0 = A.coords[cur][i * 4]; y0 = A.coords[cur][i * 4 + 1]; x1 = A.coords[cur][i * 4 + 2]; y1 = A.coords[cur][i * 4 + 3];
            ang = A.angles[cur][i];
            cf = A.conf[cur][i];
            oi = A.oidx[cur][i];
            keep = group_one(G, c, A, reg_stride, i, x0, y0, x1, y1, ang, cf, oi, after) ? 1 : 0;
        }
        for (int s = 0; s + 1 < G.m; ++s) {      // survivors after the group's inner stages (the last stage's count is the compaction's)
            const unsigned long long ms = __ballot((after >> s) & 1u);
            if (lane == 0 && ms) atomicAdd(&scount[s], (int)__popcll(ms));
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) {
            const int j = off + before;
            A.map[j] = i;
            A.coords[nxt][j * 4] = x0; A.coords[nxt][j * 4 + 1] = y0; A.coords[nxt][j * 4 + 2] = x1; A.coords[nxt][j * 4 + 3] = y1;
            A.angles[nxt][j] = ang;
            A.neg_angles[j] = -ang;                                         // what the next extraction is called with (face_analysis.py:782)
            A.oidx[nxt][j] = oi;
            A.conf[nxt][j] = cf;
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    const int cnt = base;
    // features of the survivors (map is complete: barriers above)
    const int kf = A.k_feat;
    for (int e = tid; e < cnt * kf; e += blockDim.x) {
        const int j = e / kf, f = e - j * kf;
        A.sl[nxt][(size_t)j * kf + f] = A.sl[cur][(size_t)A.map[j] * kf + f];
    }
    // A tracked frame sizes the next launches by its bound, not by this count: the rows between them, which a compaction leaves as
    // they were, get a defined, finite window (the frame's first pixel, no rotation) and zero features, so that the extraction, the
    // network and the regression of the next group read defined data; the next glue launch skips them by the device count.
    if (A.pad_to > cnt) {
        for (int j = cnt + tid; j < A.pad_to; j += blockDim.x) {
            A.coords[nxt][(size_t)j * 4] = 0.0; A.coords[nxt][(size_t)j * 4 + 1] = 0.0; A.coords[nxt][(size_t)j * 4 + 2] = 1.0; A.coords[nxt][(size_t)j * 4 + 3] = 1.0;
            A.angles[nxt][j] = 0.0;
            A.neg_angles[j] = 0.0;
            A.oidx[nxt][j] = 0;
            A.conf[nxt][j] = 0.0;
        }
        for (int e = cnt * kf + tid; e < A.pad_to * kf; e += blockDim.x) A.sl[nxt][e] = 0.0f;
    }
    if (H.cap > 0 && cnt <= H.cap) {      // last group: the survivors themselves, for the host (nxt[] is complete: barrier)
        __syncthreads();
        for (int j = tid; j < cnt; j += blockDim.x) {
            for (int q = 0; q < 4; ++q) H.coords[(size_t)j * 4 + q] = A.coords[nxt][(size_t)j * 4 + q];
            H.angles[j] = A.angles[nxt][j];
            H.conf[j] = A.conf[nxt][j];
            H.oidx[j] = A.oidx[nxt][j];
        }
        __threadfence_system();
        __syncthreads();
    }
    if (tid == 0) {
        *A.count_out = cnt;
        if (host_count) publish_group(host_count, scount, G.m, cnt, seq);
    }
}

// (Round 4 measured regression AND glue of a stage as ONE launch — a workgroup per R candidates runs the regression of its rows,
// publishes them with write-through stores, draws a ticket, and the workgroup with the last ticket runs the glue: 16 us per stage
// against 8.7 + 5.4 for the two launches (1.57 against 1.49 ms per frame; with a device-scope fence instead of write-through
// stores 1.66: the fence writes back the whole L2 of the workgroup's XCD).  Not kept.)

// The same group for batches of many frames' windows (the single workgroup above walks 1024 candidates per step): two launches
// of one workgroup per kChunk candidates.  `mark` updates every candidate IN PLACE in the cur arrays (nobody else reads them any
// more), writes its keep flag and the chunk's survivor counts (one per stage of the group); `scatter` turns the chunk counts into
// its base offset (a sum over the chunks before it), repeats the chunk-local scan on the flags and moves the survivors, order
// preserved, into the nxt arrays.
constexpr int kChunk = 4096;

__global__ void __launch_bounds__(1024) k_cascade_group_mark(GroupDesc G, hg_cascade_consts c, StageArrays A, int64_t reg_stride, int32_t* __restrict__ chunk_count) {
    __shared__ int scount[kMaxGroup];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = min(*A.count_in, A.n_max), cur = A.cur;
    const int lo = blockIdx.x * kChunk, hi = min(n, lo + kChunk);
    if (tid < kMaxGroup) scount[tid] = 0;
    __syncthreads();
    for (int i0 = lo; i0 < hi; i0 += blockDim.x) {
        const int i = i0 + tid;
        unsigned after = 0;
        if (i < hi) {
            double x0 = A.coords[cur][(size_t)i * 4], y0 = A.coords[cur][(size_t)i * 4 + 1], x1 = A.coords[cur][(size_t)i * 4 + 2], y1 = A.coords[cur][(size_t)i * 4 + 3];
            double ang = A.angles[cur][i], cf = A.conf[cur][i];
            const int32_t oi = A.oidx[cur][i];
            const bool keep = group_one(G, c, A, reg_stride, i, x0, y0, x1, y1, ang, cf, oi, after);
            A.coords[cur][(size_t)i * 4] = x0; A.coords[cur][(size_t)i * 4 + 1] = y0; A.coords[cur][(size_t)i * 4 + 2] = x1; A.coords[cur][(size_t)i * 4 + 3] = y1;
            A.angles[cur][i] = ang;
            A.conf[cur][i] = cf;
            A.discard[i] = keep ? 0 : 1;
        }
        for (int s = 0; s < G.m; ++s) {
            const unsigned long long ms = __ballot((after >> s) & 1u);
            if (lane == 0 && ms) atomicAdd(&scount[s], (int)__popcll(ms));
        }
    }
    __syncthreads();
    if (tid < kMaxGroup) chunk_count[blockIdx.x * kMaxGroup + tid] = scount[tid];
}

__global__ void __launch_bounds__(1024) k_cascade_group_scatter(int m, StageArrays A, const int32_t* __restrict__ chunk_count, int32_t* host_count, int seq) {
    __shared__ int wsum[16];
    __shared__ int base;
    __shared__ int stot[kMaxGroup];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(*A.count_in, A.n_max), cur = A.cur, nxt = 1 - cur;
    const int lo = blockIdx.x * kChunk, hi = min(n, lo + kChunk);
    // base = survivors of the chunks before this one (the last workgroup also learns the totals)
    int part = 0;
    for (int b = tid; b < (int)blockIdx.x; b += blockDim.x) part += chunk_count[b * kMaxGroup + m - 1];
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
        base = t;
    }
    __syncthreads();
    const int kf = A.k_feat;
    for (int i0 = lo; i0 < hi; i0 += blockDim.x) {
        const int i = i0 + tid;
        const int keep = (i < hi && A.discard[i] == 0) ? 1 : 0;
        const unsigned long long mk = __ballot(keep);
        const int before = __popcll(mk & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(mk);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) {
            const int j = off + before;
            const double ang = A.angles[cur][i];
            A.map[j] = i;
            for (int q = 0; q < 4; ++q) A.coords[nxt][(size_t)j * 4 + q] = A.coords[cur][(size_t)i * 4 + q];
            A.angles[nxt][j] = ang;
            A.neg_angles[j] = -ang;
            A.oidx[nxt][j] = A.oidx[cur][i];
            A.conf[nxt][j] = A.conf[cur][i];
            for (int f = 0; f < kf; ++f) A.sl[nxt][(size_t)j * kf + f] = A.sl[cur][(size_t)i * kf + f];
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1) {      // the last chunk's end offset is the total
        if (host_count) {      // totals of the inner stages, for the host
            if (tid < kMaxGroup) stot[tid] = 0;
            __syncthreads();
            for (int s = 0; s + 1 < m; ++s) {
                int t = 0;
                for (int b = tid; b < (int)gridDim.x; b += blockDim.x) t += chunk_count[b * kMaxGroup + s];
                for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
                if (lane == 0 && t) atomicAdd(&stot[s], t);
            }
            __syncthreads();
        }
        if (tid == 0) {
            *A.count_out = base;
            if (host_count) publish_group(host_count, stot, m, base, seq);
        }
    }
}

void set_dev(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        hg::fail(HG_ERR_DEVICE, "no HIP device available (this library has no CPU execution path)");
    if (device < 0 || device >= count) hg::fail(HG_ERR_DEVICE, "device %d out of range (0..%d)", device, count - 1);
    HG_HIP(hipSetDevice(device));
}

}  // namespace

extern "C" {

int hg_cascade_update_device(int device, int stage_type, const hg_cascade_consts* c, int64_t n, double* coords_dev, double* angles_dev,
                             const double* reg_dev, const int32_t* orig_index_dev, const double* orig_coords_dev,
                             const double* orig_angles_dev, const double* orig_level_dev, uint8_t* discard_dev, void* stream) {
    return guarded([&] {
        if (!c) hg::fail(HG_ERR_ARG, "null constants");
        if (stage_type < HG_STAGE_DISC || stage_type > HG_STAGE_SCALE) hg::fail(HG_ERR_ARG, "unknown stage type %d", stage_type);
        if (n < 0) hg::fail(HG_ERR_ARG, "negative candidate count");
        if (n > 0 && (!coords_dev || !angles_dev || !reg_dev || !orig_index_dev || !orig_coords_dev || !orig_angles_dev || !orig_level_dev || !discard_dev))
            hg::fail(HG_ERR_ARG, "null data pointer");
        set_dev(device);
        if (n == 0) return;
        hipLaunchKernelGGL(k_cascade_update, (unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream, stage_type, *c, n, coords_dev, angles_dev, reg_dev,
                           orig_index_dev, orig_coords_dev, orig_angles_dev, orig_level_dev, discard_dev);
        HG_HIP(hipGetLastError());
    });
}

int hg_cascade_compact_device(int device, const uint8_t* discard_dev, int64_t n, int32_t* map_dev, int32_t* count_dev, void* stream) {
    return guarded([&] {
        if (n < 0 || n > 0x7fffffffll) hg::fail(HG_ERR_ARG, "bad candidate count");
        if (!count_dev || (n > 0 && (!discard_dev || !map_dev))) hg::fail(HG_ERR_ARG, "null data pointer");
        set_dev(device);
        hipLaunchKernelGGL(k_cascade_compact, 1, 1024, 0, (hipStream_t)stream, discard_dev, n, map_dev, count_dev);
        HG_HIP(hipGetLastError());
    });
}

int hg_gather_rows_device(int device, const void* src_dev, void* dst_dev, int64_t row_bytes, const int32_t* map_dev,
                          const int32_t* count_dev, int64_t n_max, void* stream) {
    return guarded([&] {
        if (row_bytes <= 0 || (row_bytes & 3)) hg::fail(HG_ERR_ARG, "row_bytes must be a positive multiple of 4");
        if (n_max < 0) hg::fail(HG_ERR_ARG, "negative row count");
        if (!count_dev || (n_max > 0 && (!src_dev || !dst_dev || !map_dev))) hg::fail(HG_ERR_ARG, "null data pointer");
        if (src_dev == dst_dev && n_max > 0) hg::fail(HG_ERR_ARG, "gather must be out of place");
        set_dev(device);
        if (n_max == 0) return;
        const int vec16 = (row_bytes % 16 == 0 && ((uintptr_t)src_dev % 16) == 0 && ((uintptr_t)dst_dev % 16) == 0) ? 1 : 0;
        const unsigned threads = row_bytes >= 4096 ? 256 : 64;
        hipLaunchKernelGGL(k_gather_rows, (unsigned)std::min<int64_t>(n_max, 16384), threads, 0, (hipStream_t)stream, (const char*)src_dev, (char*)dst_dev,
                           row_bytes, map_dev, count_dev, vec16);
        HG_HIP(hipGetLastError());
    });
}

// ---- the whole stage loop as one host call ---------------------------------------------------------------------------
struct hg_cascade {
    int device = 0, w = 0, h = 0, k = 0;
    std::vector<hg_cascade_stage> stages;
    hg_cascade_consts base{};
    double cut_offs[10];
    int32_t interp[10] = {};             // enum hg_filter per serial (hg_cascade_set_interpolation); NEAREST until set
    hg_patcher* patcher = nullptr;
    int64_t cap = 0;
    hg::DevBuf coords[2], angles[2], conf[2], oidx[2], sl[2], subs[2], neg, reg, discard, map, count, orig_coords, orig_level, orig_angles, chunk_count;
    hg::DevBuf pre_box, pre_frame;       // hg_cascade_detect_frame_device: the box of the whole frame and the prescaled frame
    int pre_src_w = 0, pre_src_h = 0;    // ... the frame size pre_box was written for
    int frame_format = HG_FRAME_L;       // hg_cascade_set_frame_format: how frame_dev / ld of the detect entries are read
    hg::DevBuf gray_frame;               // a colour frame that is not prescaled, converted (grows on demand, like pre_frame)
    hg::DevBuf frame_stack;              // hg_cascade_detect_frames_device: the prescaled / converted grey frames of a stack, dense, one after the other
    // hg_cascade_detect_frame_list_device: the grey slots of the frames that are prescaled / converted; the descriptor table; the frame of
    // every original window; and what depends on the list's geometry alone, kept under the key of the whole list (hg_frame_list.hpp) —
    // the distinct level tables, every frame's whole-frame box and grid number
    hg::DevBuf list_gray, list_desc, list_win, list_meta;
    uint64_t list_key = 0;
    int prescale_filter = HG_RESAMPLE_NEAREST;      // hg_cascade_set_prescale_filter (enum hg_resample)
    int32_t* host_count = nullptr;       // pinned, device-visible: {count, sequence number} (publish_count)
    int32_t seq = 0;                     // sequence number of the last read-back asked for
    char* host_res = nullptr;            // pinned: the final survivors (HostResults), kResCap rows
    static constexpr int kResCap = 4096;

    void reserve(int64_t n0) {
        if (n0 <= cap) return;
        for (int b = 0; b < 2; ++b) {
            coords[b].alloc((size_t)n0 * 32);
            angles[b].alloc((size_t)n0 * 8);
            conf[b].alloc((size_t)n0 * 8);
            oidx[b].alloc((size_t)n0 * 4);
            sl[b].alloc((size_t)n0 * k * 4);
            subs[b].alloc((size_t)n0 * w * h);
        }
        neg.alloc((size_t)n0 * 8);
        reg.alloc((size_t)n0 * 8 * kMaxGroup);      // regressions of a group of stages: [stage of the group][candidate], stride = cap
        discard.alloc((size_t)n0);
        map.alloc((size_t)n0 * 4);
        count.alloc(16);
        orig_coords.alloc((size_t)n0 * 32);
        orig_level.alloc((size_t)n0 * 24);
        orig_angles.alloc((size_t)n0 * 8);
        HG_HIP(hipMemset(orig_angles.p, 0, (size_t)n0 * 8));
        for (auto& st : stages)
            if (st.flow && hg_flow_reserve(st.flow, n0) != HG_OK) hg::fail(HG_ERR_NOMEM, "%s", hg_last_error());
        cap = n0;
    }
};

int hg_cascade_create(const hg_cascade_stage* stages, int n_stages, int sub_w, int sub_h, int n_features, const hg_cascade_consts* consts,
                      const double* cut_offs_face, int n_cut_offs, int device, hg_cascade** out) {
    return guarded([&] {
        if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
        *out = nullptr;
        if (!stages || n_stages <= 0 || n_stages > 64 || !consts || !cut_offs_face) hg::fail(HG_ERR_ARG, "bad stage list");
        if (sub_w <= 0 || sub_h <= 0 || (sub_w * sub_h) % 4 || n_features <= 0 || n_features > 256) hg::fail(HG_ERR_ARG, "bad sub-image size / feature count");
        for (int k = 0; k < n_stages; ++k) {
            if (stages[k].type < HG_STAGE_DISC || stages[k].type > HG_STAGE_SCALE) hg::fail(HG_ERR_ARG, "stage %d: unknown type %d", k, stages[k].type);
            if (stages[k].serial < 0 || stages[k].serial >= n_cut_offs || n_cut_offs > 10) hg::fail(HG_ERR_ARG, "stage %d: serial %d has no cut-off", k, stages[k].serial);
            if (!stages[k].classifier) hg::fail(HG_ERR_ARG, "stage %d: no classifier", k);
            if (k == 0 && !stages[k].flow) hg::fail(HG_ERR_ARG, "the first stage needs a network");
        }
        set_dev(device);
        auto c = std::make_unique<hg_cascade>();
        c->device = device;
        c->w = sub_w;
        c->h = sub_h;
        c->k = n_features;
        c->stages.assign(stages, stages + n_stages);
        c->base = *consts;
        for (int i = 0; i < 10; ++i) c->cut_offs[i] = i < n_cut_offs ? cut_offs_face[i] : 0.0;
        if (hg_patcher_create(device, &c->patcher) != HG_OK) hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        HG_HIP(hipHostMalloc((void**)&c->host_count, 64, hipHostMallocDefault));
        c->host_count[0] = c->host_count[1] = 0;
        HG_HIP(hipHostMalloc((void**)&c->host_res, (size_t)hg_cascade::kResCap * 52, hipHostMallocDefault));
        *out = c.release();
    });
}

int hg_cascade_set_interpolation(hg_cascade* c, const int32_t* filters, int n) {
    return guarded([&] {
        if (!c || !filters || n <= 0) hg::fail(HG_ERR_ARG, "null cascade handle or empty filter list");
        for (int i = 0; i < n; ++i)
            if (filters[i] != HG_FILTER_NEAREST && filters[i] != HG_FILTER_BILINEAR && filters[i] != HG_FILTER_BICUBIC)
                hg::fail(HG_ERR_ARG, "entry %d: unknown interpolation filter %d (0 NEAREST, 2 BILINEAR, 3 BICUBIC)", i, filters[i]);
        for (size_t k = 0; k < c->stages.size(); ++k)
            if (c->stages[k].serial >= n) hg::fail(HG_ERR_ARG, "stage %d: serial %d has no interpolation filter", (int)k, c->stages[k].serial);
        for (int i = 0; i < 10; ++i) c->interp[i] = i < n ? filters[i] : HG_FILTER_NEAREST;      // (serials are < 10: hg_cascade_create)
    });
}

int hg_cascade_set_frame_format(hg_cascade* c, int format) {
    return guarded([&] {
        if (!c) hg::fail(HG_ERR_ARG, "null cascade handle");
        if (!hg::frame_bpp(format)) hg::fail(HG_ERR_ARG, "unknown frame format %d (0 L, 1 RGB, 2 BGR, 3 RGBA, 4 BGRA)", format);
        c->frame_format = format;
    });
}

int hg_cascade_set_prescale_filter(hg_cascade* c, int filter) {
    return guarded([&] {
        if (!c) hg::fail(HG_ERR_ARG, "null cascade handle");
        if (filter < HG_RESAMPLE_NEAREST || filter > HG_RESAMPLE_HAMMING)
            hg::fail(HG_ERR_ARG, "unknown resize filter %d (0 NEAREST, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)", filter);
        c->prescale_filter = filter;
    });
}

void hg_cascade_free(hg_cascade* c) {
    if (!c) return;
    if (hipSetDevice(c->device) == hipSuccess) {
        if (c->patcher) hg_patcher_free(c->patcher);
        if (c->host_count) (void)hipHostFree(c->host_count);
        if (c->host_res) (void)hipHostFree(c->host_res);
    }
    delete c;
}

}  // extern "C"

namespace {

LevelTable make_level_table(const hg_cascade_level* levels, int n_levels) {
    if (!levels || n_levels < 1 || n_levels > kMaxLevels) hg::fail(HG_ERR_ARG, "1..%d pyramid levels", kMaxLevels);
    LevelTable T{};
    T.n_levels = n_levels;
    int64_t tot = 0;
    for (int L = 0; L < n_levels; ++L) {
        const hg_cascade_level& v = levels[L];
        if (v.nx < 1 || v.ny < 1 || (int64_t)v.nx * v.ny > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "level %d: bad grid %d x %d", L, v.nx, v.ny);
        T.first[L] = (int32_t)tot;
        tot += (int64_t)v.nx * v.ny;
        if (tot > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "too many windows");
        T.lv[L] = v;
    }
    T.first[n_levels] = (int32_t)tot;
    return T;
}

// FNV-1a over a plain struct: the key under which the patcher keeps index tables of boxes that depend on sizes only
uint64_t key_of(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h ? h : 1;
}

// Every frame-reading entry of this file refuses a bad frame as a bad ARGUMENT, before it launches or writes anything: a row stride
// below the width (a broadcast view has 0) would have every row read its neighbours' pixels.
void check_frame_geometry(int frame_h, int frame_w, int64_t ld, int bpp = 1) {
    if (frame_h <= 0 || frame_w <= 0 || ld < (int64_t)frame_w * bpp)
        hg::fail(HG_ERR_ARG, "bad frame geometry: %d rows of %d pixels of %d byte(s), %lld apart", frame_h, frame_w, bpp, (long long)ld);
}

// What a LIST of frames of different sizes keeps on the device (list_frames): the list itself, one level table per DISTINCT grid, the
// grid number of every frame, and room for the frame of every original window, which k_cascade_init_list writes.
struct ListRun {
    hg::FrameList fl;
    const LevelTable* tables_dev;
    const int32_t* grid_of_dev;
    int32_t* win_frame_dev;
};

// ---- one pass of the stage loop: where the windows come from, which frames the rows are cut from, what becomes of the survivors ----
// The loop is the same for all of them: rows are independent and the compaction keeps their order, so the survivors of several frames
// come out by frame and, inside a frame, in the order the frame alone gives.
struct StagePass {
    enum Windows {
        HOST_BOXES,      // n0 boxes and level constants in host memory, copied in (k_cascade_init)
        GRID,            // the closed form of level table T over ONE frame (k_cascade_init_grid)
        GRID_STACK,      // a STACK of frames: n_frames copies of T's grid, window f * period + j = window j of frame f (k_cascade_init_frames);
                         //   every extraction cuts row i from frame orig_index[i] / period
        GRID_LIST,       // a LIST of frames: the concatenated grids (k_cascade_init_list), row i's frame is win_frame[orig_index[i]]
        // TRACKED frames: nine windows per held face (tracked_window), from boxes the previous frame's last kernel left on the device; the
        // candidate count never visits the host.  n0 = 9 * n_faces bounds it from the start, so every launch of every group is sized by
        // that bound and the glue kernels take the live count from the device word they already carry (A.count_in under A.n_max).  Rows
        // between the live count and the bound: k_cascade_group gives them a defined window and zero features after every compaction
        // (A.pad_to), so each extraction reads finite boxes and each network defined pixels; the sub-images carried over a Disc stage are
        // gathered by the device count (k_gather_rows) and the rows past it keep earlier bytes — any byte is a pixel, rows are independent,
        // and the next glue launch skips them by the count.  A live count of 0 is a normal case: every later launch runs on filler rows
        // and compacts none.  pad_to exists on k_cascade_group's single-workgroup path only: the bound stays at or under 2 * kChunk.
        TRACKED,         // ONE stream: n_faces boxes at face_dev, n_faces known on the host (k_cascade_init_tracked_multi)
        TRACKED_STREAMS  // a SET of streams over a stack of n_frames = n_streams frames: faces (n_streams, max_faces, 4), held_dev their
                         //   n_streams counts, n_faces the host's mirror of their sum; period = 9 * max_faces original windows per stream,
                         //   orig_coords / orig_level indexed over the whole set's period (k_cascade_init_tracked_streams)
    };
    enum Survivors {
        TO_HOST,         // copied to the host arrays of `host` (each nullable), their number to *host.n_out; more than host.cap is refused
        ON_DEVICE,       // left in coords[cur], angles[cur], conf[cur], oidx[cur] until the next call; the host knows their number
        BOUNDED          // left there, and their number in a device word: nothing is read back in the whole pass, no poll runs,
                         //   stage_counts is -1 throughout and the host knows the bound n0 only (what the tracked passes ask for)
    };
    Windows windows;
    hg::FrameSource frames;
    int64_t n0;                  // windows the pass starts with
    Survivors survivors = ON_DEVICE;
    struct {
        double *coords, *angles;
        int32_t* orig_index;
        double* confidence;
        int64_t cap, *n_out;
    } host{};
    const double *boxes_host = nullptr, *level_host = nullptr;      // HOST_BOXES
    const LevelTable* T = nullptr;                                     // GRID, GRID_STACK: one frame's
    const ListRun* list = nullptr;                                     // GRID_LIST
    const double* face_dev = nullptr;                                  // TRACKED, TRACKED_STREAMS
    const int32_t* held_dev = nullptr;
    int n_faces = 0, max_faces = 0;
    hg_tracked_consts tc{};

    int64_t period() const { return windows == GRID_STACK ? T->first[T->n_levels] : windows == TRACKED_STREAMS ? (int64_t)kTracked * max_faces : 0; }
    // the key of the first stage's boxes where they are a function of sizes alone (their index tables are kept)
    uint64_t table_key() const { return windows == GRID || windows == GRID_STACK ? key_of(T, sizeof *T) : windows == GRID_LIST ? list->fl.key : 0; }

    static StagePass boxes(const hg::FrameSource& one, const double* boxes_host, const double* level_host, int64_t n0) {
        StagePass P{HOST_BOXES, one, n0};
        P.boxes_host = boxes_host;
        P.level_host = level_host;
        return P;
    }
    static StagePass grid(const hg::FrameSource& fr, const LevelTable& T) {      // over one frame, or over every frame of a stack
        const bool stack = fr.kind == hg::FrameSource::STACK;
        StagePass P{stack ? GRID_STACK : GRID, fr, (int64_t)T.first[T.n_levels] * (stack ? fr.n_frames : 1)};
        P.T = &T;
        return P;
    }
    static StagePass grid_list(const ListRun& R) {
        StagePass P{GRID_LIST, hg::FrameSource::of_list(R.fl), R.fl.n_windows};
        P.list = &R;
        return P;
    }
    static StagePass tracked(const hg::FrameSource& fr, const hg_tracked_consts& tc, const double* face_dev, int n_faces, const int32_t* held_dev = nullptr,
                             int max_faces = 0) {      // held_dev: a stream set over the stack fr
        StagePass P{held_dev ? TRACKED_STREAMS : TRACKED, fr, (int64_t)kTracked * n_faces, BOUNDED};
        P.face_dev = face_dev;
        P.held_dev = held_dev;
        P.n_faces = n_faces;
        P.max_faces = max_faces;
        P.tc = tc;
        return P;
    }
    StagePass& to_host(double* coords, double* angles, int32_t* orig_index, double* confidence, int64_t cap, int64_t* n_out) {
        survivors = TO_HOST;
        host = {coords, angles, orig_index, confidence, cap, n_out};
        return *this;
    }
};
// n: the survivors (BOUNDED: their bound); they are in the cur half of the ping-pong arrays; count_dev: the device word of their number
struct PassResult {
    int64_t n;
    int cur;
    const int32_t* count_dev;
    int64_t rows;              // rows the networks executed
    bool on_host;              // the last group's kernel has written the survivors to pinned memory (host_results) already
};

// The refusals of a pass: values only — what kind of pass it is cannot be wrong
void check_pass(const hg_cascade* c, const StagePass& P) {
    const hg::FrameSource& F = P.frames;
    const int64_t n0 = P.n0;
    if (!c || (P.survivors == StagePass::TO_HOST && !P.host.n_out)) hg::fail(HG_ERR_ARG, "null argument");
    if (n0 < 0 || n0 > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "bad window count");
    if (n0 > 0 && (!F.px || (P.windows == StagePass::HOST_BOXES && (!P.boxes_host || !P.level_host)))) hg::fail(HG_ERR_ARG, "null data pointer");
    // here, not by the patcher in the middle of the stage loop (whose refusal came back as HG_ERR_DEVICE after the grid kernel had run)
    if (n0 > 0) check_frame_geometry(F.h, F.w, F.ld);
    switch (P.windows) {
        case StagePass::GRID_LIST:
            if (F.n_frames < 1 || n0 != P.list->fl.n_windows || !P.list->tables_dev || !P.list->win_frame_dev) hg::fail(HG_ERR_ARG, "bad frame list");
            break;
        case StagePass::GRID_STACK:
            if (F.n_frames < 1 || P.period() < 1 || n0 != P.period() * F.n_frames) hg::fail(HG_ERR_ARG, "bad frame stack");
            break;
        case StagePass::TRACKED:      // a positive multiple of nine matching the held count; beyond kMaxFaces the two-launch chunk path, which has no pad_to, would come near
            if (P.n_faces < 1 || P.n_faces > kMaxFaces || n0 != (int64_t)kTracked * P.n_faces || !P.face_dev) hg::fail(HG_ERR_ARG, "bad tracked frame");
            break;
        case StagePass::TRACKED_STREAMS:      // the bound 9 * sum of held lies under the windows of the whole set, and those inside k_cascade_group's single-workgroup path (pad_to)
            if (F.n_frames < 1 || P.max_faces < 1 || P.max_faces > kMaxFaces || P.period() * F.n_frames > 2 * kChunk || P.n_faces < 1 ||
                n0 != (int64_t)kTracked * P.n_faces || n0 > P.period() * F.n_frames || !P.face_dev || !P.held_dev)
                hg::fail(HG_ERR_ARG, "bad tracked stream set");
            break;
        default: break;
    }
}

// The start of a pass: original windows, their level constants and the first candidates, by the kind of window source
void launch_init(hg_cascade* c, const StagePass& P, hipStream_t st) {
    const int64_t n0 = P.n0;
    double *oc = (double*)c->orig_coords.p, *ol = (double*)c->orig_level.p, *co = (double*)c->coords[0].p, *an = (double*)c->angles[0].p, *ng = (double*)c->neg.p,
           *cf = (double*)c->conf[0].p;
    int32_t *oi = (int32_t*)c->oidx[0].p, *cnt = (int32_t*)c->count.p;
    const unsigned blocks = (unsigned)((n0 + 255) / 256);
    switch (P.windows) {
        case StagePass::TRACKED_STREAMS:
            hipLaunchKernelGGL(k_cascade_init_tracked_streams, 1, 1024, 0, st, P.tc, P.face_dev, P.held_dev, P.frames.n_frames, P.max_faces, oc, ol, co, an, ng, cf, oi, cnt);
            break;
        case StagePass::TRACKED:
            hipLaunchKernelGGL(k_cascade_init_tracked_multi, (unsigned)((n0 + 63) / 64), 64, 0, st, P.tc, P.face_dev, P.n_faces, oc, ol, co, an, ng, cf, oi, cnt);
            break;
        case StagePass::GRID_LIST:
            hipLaunchKernelGGL(k_cascade_init_list, blocks, 256, 0, st, P.list->tables_dev, P.list->fl.dev, P.list->grid_of_dev, P.list->fl.n_frames, (int)n0, oc, ol, co,
                               an, ng, cf, oi, cnt, P.list->win_frame_dev);
            break;
        case StagePass::GRID:
        case StagePass::GRID_STACK:
            hipLaunchKernelGGL(k_cascade_init_grid, blocks, 256, 0, st, *P.T, oc, ol, co, an, ng, cf, oi, cnt);
            if (P.windows == StagePass::GRID_STACK && P.frames.n_frames > 1)
                hipLaunchKernelGGL(k_cascade_init_frames, blocks, 256, 0, st, (int)P.period(), (int)n0, oc, ol, co, an, ng, cf, oi, cnt);
            break;
        case StagePass::HOST_BOXES:
            HG_HIP(hipMemcpyAsync(oc, P.boxes_host, (size_t)n0 * 32, hipMemcpyHostToDevice, st));
            HG_HIP(hipMemcpyAsync(ol, P.level_host, (size_t)n0 * 24, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_cascade_init, blocks, 256, 0, st, (int)n0, (const double*)oc, co, an, ng, cf, oi, cnt);
            break;
    }
    HG_HIP(hipGetLastError());
}

// The host's wait for a pinned sequence word a kernel writes last, at system scope (publish_count): polled, never a stream
// synchronisation, which costs the caller 20-40 us more before it has caught up with the device again.  A deadline guards against a
// device that never answers: then one synchronisation, one more look, and `what` as the failure.
void wait_for_seq(const int32_t* word, int32_t seq, hipStream_t st, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0; __atomic_load_n(word, __ATOMIC_ACQUIRE) != seq; ++spins) {
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
            HG_HIP(hipStreamSynchronize(st));
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return;
            hg::fail(HG_ERR_DEVICE, "%s", what);
        }
        __builtin_ia32_pause();
    }
}

HostResults host_results(const hg_cascade* c) {
    constexpr size_t cap = hg_cascade::kResCap;
    return HostResults{(double*)c->host_res, (double*)(c->host_res + cap * 32), (double*)(c->host_res + cap * 40), (int32_t*)(c->host_res + cap * 48), 0};
}

// The stage loop proper, group by group, from the candidates launch_init left; stage_counts (nullable): survivors after every stage
PassResult run_groups(hg_cascade* c, const StagePass& P, int32_t* stage_counts, hipStream_t st) {
    const int ns = (int)c->stages.size();
    const bool bounded = P.survivors == StagePass::BOUNDED;
    const hg::RowFrames row_frames{(const int32_t*)nullptr, true, P.period()};
    bool results_on_host = false;
    int cur = 0, cnt_slot = 0;
    int sb = 0;                                    // which of subs[] holds the extracted sub-images, row-aligned with the candidates
    int64_t n_bound = P.n0, rows = 0;              // n_bound: host-side upper bound of the candidate count (exact after a Disc stage)
    const size_t row = (size_t)c->w * c->h;
    // The reference compacts subimages_arr after EVERY stage (FaceDetectUpdated.py:753) and reuses it in a stage that follows a
    // Disc stage and owns a network (:674-681).  Here the rows travel only while a later stage will read them before the next
    // extraction replaces them: carry[k] = "stage k's survivors' sub-images are needed again".  (In the shipped pipeline that is
    // after Disc1 / Disc3 / Disc5 / Disc7 only; a pipeline such as PosX(net), Disc(None), PosX(net) carries them through two stages.)
    std::vector<char> carry((size_t)ns, 0);
    {
        bool need = false;                         // need at the entry of stage k + 1
        for (int k = ns - 1; k >= 0; --k) {
            carry[(size_t)k] = need;
            const bool prev_disc = k > 0 && c->stages[k - 1].type == HG_STAGE_DISC;
            if (c->stages[k].flow) need = prev_disc;          // reuses them (needs them at entry) or extracts afresh (does not)
        }
    }
    const bool no_groups = getenv("HIGSFA_CASCADE_NO_GROUPS") != nullptr;      // every stage a group of its own (tests, A/B); read per frame
    for (int k = 0; k < ns;) {
        // the group: stage k and the stages behind it that have no network of their own (they read the same sl), at most kMaxGroup
        int m = 1;
        while (!no_groups && k + m < ns && m < kMaxGroup && !c->stages[k + m].flow) ++m;
        const hg_cascade_stage& S = c->stages[k];
        if (n_bound == 0) {
            for (int s = 0; s < m && stage_counts; ++s) stage_counts[k + s] = 0;
            k += m;
            continue;
        }
        const bool skip_extract = (k > 0 && c->stages[k - 1].type == HG_STAGE_DISC) || !S.flow;      // FaceDetectUpdated.py:674-681
        if (!skip_extract) {
            // (the first stage's angles are all zero: the plain EXTENT kernel — a window with delta_ang == 0 is cut from the frame itself —
            // and where the windows come from level tables they are a function of those alone: their index tables are kept)
            // the stage's filter: interpolation_formats[network_serial] (FaceDetectUpdated.py:671, :686)
            hg::RowFrames rf = row_frames;
            rf.index_dev = (const int32_t*)c->oidx[cur].p;
            if (hg::patcher_extract_source(c->patcher, P.frames, k == 0 ? P.table_key() : 0, rf, c->interp[S.serial], (const double*)c->coords[cur].p,
                                           k == 0 ? nullptr : (const double*)c->neg.p, n_bound, c->w, c->h, c->subs[sb].p, HG_U8, (int64_t)row, st) != HG_OK)
                hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        }
        if (S.flow) {
            if (hg_flow_execute_device(S.flow, c->subs[sb].p, HG_U8, n_bound, (int64_t)row, c->sl[cur].p, HG_F32, c->k, c->k, st) != HG_OK)
                hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
            rows += n_bound;
        }
        GroupDesc G{};
        G.m = m;
        hg_gauss* clf[kMaxGroup] = {};
        bool any_disc = false;
        for (int s = 0; s < m; ++s) {
            const hg_cascade_stage& Ss = c->stages[k + s];
            G.type[s] = Ss.type;
            G.cut[s] = c->cut_offs[Ss.serial];
            clf[s] = Ss.classifier;
            any_disc = any_disc || Ss.type == HG_STAGE_DISC;
        }
        // the group's regressions, all on the rows of sl[cur]: reg[s * cap + i]
        if (hg_gauss_regression_multi_device(clf, m, c->sl[cur].p, HG_F32, n_bound, c->k, (double*)c->reg.p, c->cap, st) != HG_OK)
            hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        StageArrays A{};
        for (int b = 0; b < 2; ++b) {
            A.coords[b] = (double*)c->coords[b].p;
            A.angles[b] = (double*)c->angles[b].p;
            A.conf[b] = (double*)c->conf[b].p;
            A.oidx[b] = (int32_t*)c->oidx[b].p;
            A.sl[b] = (float*)c->sl[b].p;
        }
        A.neg_angles = (double*)c->neg.p;
        A.reg = (const double*)c->reg.p;
        A.orig_coords = (const double*)c->orig_coords.p;
        A.orig_angles = (const double*)c->orig_angles.p;
        A.orig_level = (const double*)c->orig_level.p;
        A.discard = (uint8_t*)c->discard.p;
        A.map = (int32_t*)c->map.p;
        A.count_in = (int32_t*)c->count.p + cnt_slot;
        A.count_out = (int32_t*)c->count.p + (1 - cnt_slot);
        A.k_feat = c->k;
        A.cur = cur;
        A.n_max = (int32_t)n_bound;
        A.pad_to = bounded ? (int32_t)n_bound : 0;
        // the host needs the exact count where it shrinks and sizes the next launches: after every group with a Disc stage (the
        // read-back is a poll of a pinned word, cheap enough for the small stages too), and at the end
        const bool last = k + m == ns;
        const bool want_count = !bounded && (any_disc || last);      // a bounded pass: the bound sizes the launches, nothing is read back
        const int32_t seq = want_count ? ++c->seq : 0;
        HostResults Hk{};
        if (n_bound > 2 * kChunk) {      // many frames' windows (never a bounded pass: no pad_to here): one workgroup per kChunk candidates, two launches
            const unsigned chunks = (unsigned)((n_bound + kChunk - 1) / kChunk);
            c->chunk_count.alloc((size_t)chunks * kMaxGroup * 4);
            hipLaunchKernelGGL(k_cascade_group_mark, chunks, 1024, 0, st, G, c->base, A, c->cap, (int32_t*)c->chunk_count.p);
            hipLaunchKernelGGL(k_cascade_group_scatter, chunks, 1024, 0, st, m, A, (const int32_t*)c->chunk_count.p, want_count ? c->host_count : nullptr, seq);
        } else {
            if (last && !bounded && n_bound <= hg_cascade::kResCap) {
                Hk = host_results(c);
                Hk.cap = hg_cascade::kResCap;
                results_on_host = true;
            }
            hipLaunchKernelGGL(k_cascade_group, 1, 1024, 0, st, G, c->base, A, c->cap, want_count ? c->host_count : nullptr, seq, Hk);
        }
        if (carry[(size_t)(k + m - 1)]) {       // the group's compaction applied to the sub-images as well (:753)
            const int vec16 = row % 16 == 0 ? 1 : 0;
            hipLaunchKernelGGL(k_gather_rows, (unsigned)std::min<int64_t>(n_bound, 16384), 256, 0, st, (const char*)c->subs[sb].p, (char*)c->subs[1 - sb].p,
                               (int64_t)row, (const int32_t*)c->map.p, (const int32_t*)A.count_out, vec16);
            sb = 1 - sb;
        }
        HG_HIP(hipGetLastError());
        cur = 1 - cur;
        cnt_slot = 1 - cnt_slot;
        if (want_count) {
            wait_for_seq(c->host_count + 1, seq, st, "cascade stage did not report its survivor count");
            n_bound = c->host_count[0];
            for (int s = 0; s < m && stage_counts; ++s) stage_counts[k + s] = c->host_count[2 + s];      // written before the sequence number
        } else {
            for (int s = 0; s < m && stage_counts; ++s) stage_counts[k + s] = -1;      // not read back (no stage of the group discards by a cut-off: bound of the last Disc stage)
        }
        k += m;
    }
    return PassResult{n_bound, cur, (const int32_t*)c->count.p + cnt_slot, rows, results_on_host};
}

// TO_HOST: the survivors into the caller's arrays — from pinned memory where the last group's kernel wrote them before it published
// the count, else four copies and a synchronisation
void read_survivors(hg_cascade* c, const StagePass& P, const PassResult& r, hipStream_t st) {
    const auto& o = P.host;
    const size_t n = (size_t)r.n;
    if (r.n > o.cap) hg::fail(HG_ERR_ARG, "%lld detections but room for %lld", (long long)r.n, (long long)o.cap);
    if (r.n > 0 && r.on_host) {
        const HostResults H = host_results(c);
        if (o.coords) memcpy(o.coords, H.coords, n * 32);
        if (o.angles) memcpy(o.angles, H.angles, n * 8);
        if (o.orig_index) memcpy(o.orig_index, H.oidx, n * 4);
        if (o.confidence) memcpy(o.confidence, H.conf, n * 8);
    } else if (r.n > 0) {
        if (o.coords) HG_HIP(hipMemcpyAsync(o.coords, c->coords[r.cur].p, n * 32, hipMemcpyDeviceToHost, st));
        if (o.angles) HG_HIP(hipMemcpyAsync(o.angles, c->angles[r.cur].p, n * 8, hipMemcpyDeviceToHost, st));
        if (o.orig_index) HG_HIP(hipMemcpyAsync(o.orig_index, c->oidx[r.cur].p, n * 4, hipMemcpyDeviceToHost, st));
        if (o.confidence) HG_HIP(hipMemcpyAsync(o.confidence, c->conf[r.cur].p, n * 8, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
    }
    *o.n_out = r.n;
}

// One pass: the checks, the init kernel, the group loop, the read-back.  rows_executed (nullable) is zeroed, like *host.n_out, once the
// pass is accepted and written at the end.
PassResult run_pass(hg_cascade* c, const StagePass& P, int32_t* stage_counts, int64_t* rows_executed, void* stream) {
    check_pass(c, P);
    set_dev(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (P.survivors == StagePass::TO_HOST) *P.host.n_out = 0;
    if (rows_executed) *rows_executed = 0;
    if (P.n0 == 0) {
        for (size_t k = 0; k < c->stages.size() && stage_counts; ++k) stage_counts[k] = 0;
        return PassResult{};
    }
    const int64_t set_windows = P.period() * P.frames.n_frames;      // (a stream set: orig_coords / orig_level are indexed over the whole set's period)
    c->reserve(P.windows == StagePass::TRACKED_STREAMS ? set_windows : P.n0);
    launch_init(c, P, st);
    const PassResult r = run_groups(c, P, stage_counts, st);
    if (P.survivors == StagePass::TO_HOST) read_survivors(c, P, r, st);
    if (rows_executed) *rows_executed = r.rows;
    return r;
}

// the survivors a pass left on the device, for the eye tail (hg_eyes.hip)
hg::EyeSurvivors survivors_of(const hg_cascade* c, const StagePass& P, const PassResult& r) {
    return hg::EyeSurvivors{(const double*)c->coords[r.cur].p, (const double*)c->angles[r.cur].p, (const double*)c->conf[r.cur].p, (const int32_t*)c->oidx[r.cur].p,
                            P.period(), r.n, P.survivors == StagePass::BOUNDED ? r.count_dev : nullptr};
}

// FaceDetectUpdated.py:551-561: im.resize((w, h), NEAREST) before the grid is laid out — PIL's nearest resize is the EXTENT rule over
// the whole frame (tested against PIL), so the patcher does it, into a buffer that lives with the cascade (prescale_w = 0: none).
// fr / fh / fw / fld: the frame the grid and the stage loop read — always grey.  A colour frame (hg_cascade_set_frame_format) is
// prescaled by the same whole-frame box through the format gather, which converts the sampled pixels only; one that needs no
// prescale is converted as a whole (gray_frame_of).
// dst (here and in prescale_frame): where the grey frame goes instead of the cascade's single-frame buffer — a slot of a frame stack
void gray_frame_of(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, void* stream, const void*& fr, int64_t& fld, void* dst = nullptr) {
    check_frame_geometry(frame_h, frame_w, ld, hg::frame_bpp(c->frame_format));
    set_dev(c->device);
    if (!dst) {
        c->gray_frame.alloc((size_t)frame_h * frame_w);
        dst = c->gray_frame.p;
    }
    if (hg_frame_to_gray_device(c->device, frame_dev, c->frame_format, frame_h, frame_w, ld, (uint8_t*)dst, frame_w, stream) != HG_OK)
        hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
    fr = dst;
    fld = frame_w;
}

hg::FrameSource prescale_frame(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h, void* stream,
                               void* dst = nullptr, const double* box_dev = nullptr) {
    if (prescale_w > 0 || prescale_h > 0) {
        if (prescale_w <= 0 || prescale_h <= 0 || !frame_dev) hg::fail(HG_ERR_ARG, "bad prescale size %d x %d", prescale_w, prescale_h);
        check_frame_geometry(frame_h, frame_w, ld, hg::frame_bpp(c->frame_format));
        set_dev(c->device);
        if (!box_dev && (c->pre_src_w != frame_w || c->pre_src_h != frame_h)) {      // (box_dev: the whole-frame box of a list's frame, kept with the list)
            const double box[4] = {0.0, 0.0, (double)frame_w, (double)frame_h};
            c->pre_box.upload(box, sizeof box);
            c->pre_src_w = frame_w;
            c->pre_src_h = frame_h;
        }
        if (!dst) {
            c->pre_frame.alloc((size_t)prescale_w * prescale_h);
            dst = c->pre_frame.p;
        }
        if (c->prescale_filter != HG_RESAMPLE_NEAREST) {      // im.convert("L").resize((w, h), filter): PIL's antialiased resize (hg_resample.hip)
            const int rc = hg_patcher_resize_device(c->patcher, c->prescale_filter, 0, frame_dev, c->frame_format, frame_h, frame_w, ld, HG_FRAME_L,
                                                    dst, prescale_h, prescale_w, prescale_w, stream);
            if (rc != HG_OK) hg::fail(rc, "%s", hg_last_error());
            return hg::FrameSource::one(dst, prescale_h, prescale_w, prescale_w);
        }
        const int32_t pre_shape[4] = {frame_w, frame_h, prescale_w, prescale_h};      // the whole-frame box depends on these alone
        if (hg::patcher_extract_format(c->patcher, key_of(pre_shape, sizeof pre_shape, 0x9e3779b97f4a7c15ull), c->frame_format, frame_dev, frame_h, frame_w, ld,
                                       box_dev ? box_dev : (const double*)c->pre_box.p, 1, prescale_w, prescale_h, dst, HG_U8, (int64_t)prescale_w * prescale_h,
                                       stream) != HG_OK)
            hg::fail(HG_ERR_DEVICE, "%s", hg_last_error());
        return hg::FrameSource::one(dst, prescale_h, prescale_w, prescale_w);
    }
    hg::FrameSource fr = hg::FrameSource::one(frame_dev, frame_h, frame_w, ld);
    if (c->frame_format != HG_FRAME_L && frame_dev) gray_frame_of(c, frame_dev, frame_h, frame_w, ld, stream, fr.px, fr.ld, dst);      // (a null frame: check_pass's refusal)
    return fr;
}

// ---- a stack of same-size frames through one pooled pass (include/higsfa.h, hg_cascade_detect_frames_device) ----------------------
// What both stack entries refuse, before anything is launched or written; returns the level table and the window count of ONE frame.
LevelTable check_frame_stack(const hg_cascade* c, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld,
                             int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels, int64_t out_cap, const int32_t* frame_first) {
    if (!c || !frame_first) hg::fail(HG_ERR_ARG, "null argument");
    if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) hg::fail(HG_ERR_ARG, "%d frames in a stack (1..%d)", n_frames, HG_MAX_STACK_FRAMES);
    if (out_cap < 0) hg::fail(HG_ERR_ARG, "negative output capacity");
    const LevelTable T = make_level_table(levels, n_levels);
    if ((int64_t)n_frames * T.first[T.n_levels] > 0x7fffffffll / 64) hg::fail(HG_ERR_ARG, "too many windows: %d frames of %d", n_frames, T.first[T.n_levels]);
    const int bpp = hg::frame_bpp(c->frame_format);
    check_frame_geometry(frame_h, frame_w, ld, bpp);
    if (frame_stride < (int64_t)(frame_h - 1) * ld + (int64_t)frame_w * bpp)
        hg::fail(HG_ERR_ARG, "frames %lld bytes apart, a frame reaches over %lld", (long long)frame_stride, (long long)((int64_t)(frame_h - 1) * ld + (int64_t)frame_w * bpp));
    if (!frames_dev) hg::fail(HG_ERR_ARG, "null data pointer");
    if ((prescale_w > 0 || prescale_h > 0) && (prescale_w <= 0 || prescale_h <= 0)) hg::fail(HG_ERR_ARG, "bad prescale size %d x %d", prescale_w, prescale_h);
    return T;
}

// The grey frames the pooled stage loop reads: grey frames without a prescale in place; otherwise every frame through prescale_frame —
// the code a single frame runs, one pass per frame — into its slot of the cascade's dense grey stack.
hg::FrameSource stack_frames(hg_cascade* c, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, int prescale_w,
                             int prescale_h, void* stream) {
    const bool pre = prescale_w > 0 || prescale_h > 0;
    if (!pre && c->frame_format == HG_FRAME_L) return hg::FrameSource::stack(frames_dev, frame_h, frame_w, ld, n_frames, frame_stride);
    const int oh = pre ? prescale_h : frame_h, ow = pre ? prescale_w : frame_w;
    const size_t slot = (size_t)oh * ow;
    set_dev(c->device);
    c->frame_stack.alloc(slot * n_frames);
    hg::FrameSource one;
    for (int f = 0; f < n_frames; ++f)
        one = prescale_frame(c, (const char*)frames_dev + (int64_t)f * frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, stream,
                             (char*)c->frame_stack.p + slot * f);
    return hg::FrameSource::stack(c->frame_stack.p, one.h, one.w, one.ld, n_frames, (int64_t)slot);
}

// The "fetch orig_index even if the caller does not want it" of the pooled entries: a survivor's frame is read off its index
int32_t* index_room(int32_t* out_orig_index, std::vector<int32_t>& own, int64_t out_cap, int64_t total) {
    if (out_orig_index) return out_orig_index;
    own.resize((size_t)std::min<int64_t>(out_cap, total));
    return own.data();
}

// ---- a list of frames of different sizes through one pooled pass (include/higsfa.h, hg_cascade_detect_frame_list_device) -----------
// What both list entries refuse, before anything is launched or written, and the layout of the list (hg_frame_list.hpp)
// e (nullable): the eye handle of the faces entry, whose patches are rotated windows too
hg::ListLayout check_frame_list(const hg_cascade* c, const hg_eyes* e, const hg_cascade_frame* frames, int n_frames, int64_t out_cap, const int32_t* frame_first) {
    if (!c || !frames || !frame_first) hg::fail(HG_ERR_ARG, "null argument");
    if (out_cap < 0) hg::fail(HG_ERR_ARG, "negative output capacity");
    // a stage behind the first that extracts (run_groups' skip_extract) with NEAREST, or a NEAREST eye step, cuts rotated NEAREST windows:
    // a frame outside PIL's fixed-point range is refused here, not by the patcher in the middle of the stage loop
    bool rotated_nearest = e && hg::eyes_filter(e) == HG_FILTER_NEAREST;
    for (size_t k = 1; k < c->stages.size(); ++k)
        if (c->stages[k].flow && c->stages[k - 1].type != HG_STAGE_DISC && c->interp[c->stages[k].serial] == HG_FILTER_NEAREST) rotated_nearest = true;
    hg::ListLayout L;
    const std::string why = hg::list_layout(frames, n_frames, hg::frame_bpp(c->frame_format), &L, rotated_nearest);
    if (!why.empty()) hg::fail(HG_ERR_ARG, "%s", why.c_str());
    return L;
}

// The grey frames the list's stage loop reads and everything it needs on the device.  Every frame goes through prescale_frame — the code
// a single frame runs, one pass per frame, each to its own size — into its slot of list_gray (16-byte aligned); a grey frame that needs
// no prescale is read where it is.  `desc` (the caller's, alive while R is used): the descriptors, sent to the device in stream order.
void list_frames(hg_cascade* c, const hg_cascade_frame* frames, int n_frames, const hg::ListLayout& L, void* stream, std::vector<hg::FrameDesc>& desc,
                 ListRun& R) {
    set_dev(c->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = L.first[(size_t)n_frames];
    const size_t n_grids = L.grid_frame.size();
    const size_t off_box = n_grids * sizeof(LevelTable), off_grid = off_box + (size_t)n_frames * 32, meta_bytes = off_grid + (size_t)n_frames * 4;
    if (c->list_key != L.key || c->list_meta.bytes < meta_bytes) {      // what depends on the list's geometry alone: once per list, not per call
        std::vector<char> meta(meta_bytes);
        for (size_t g = 0; g < n_grids; ++g) {
            const hg_cascade_frame& F = frames[L.grid_frame[g]];
            const LevelTable T = make_level_table(F.levels, F.n_levels);
            memcpy(meta.data() + g * sizeof(LevelTable), &T, sizeof T);
        }
        for (int f = 0; f < n_frames; ++f) {
            const double box[4] = {0.0, 0.0, (double)frames[f].frame_w, (double)frames[f].frame_h};
            memcpy(meta.data() + off_box + (size_t)f * 32, box, 32);
            memcpy(meta.data() + off_grid + (size_t)f * 4, &L.grid[(size_t)f], 4);
        }
        HG_HIP(hipStreamSynchronize(st));      // nothing of an earlier list may still read the buffer
        c->list_key = 0;
        c->list_meta.upload(meta.data(), meta_bytes);
        c->list_key = L.key;
    }
    size_t gray = 0;
    std::vector<size_t> slot((size_t)n_frames, 0);
    for (int f = 0; f < n_frames; ++f) {
        const bool pre = frames[f].prescale_w > 0;
        if (!pre && c->frame_format == HG_FRAME_L) continue;
        slot[(size_t)f] = gray;
        gray += ((size_t)L.gw[(size_t)f] * L.gh[(size_t)f] + 15) & ~(size_t)15;
    }
    c->list_gray.alloc(gray);
    c->list_desc.alloc((size_t)n_frames * sizeof(hg::FrameDesc));
    c->list_win.alloc((size_t)total * 4);
    desc.resize((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const hg_cascade_frame& F = frames[f];
        const hg::FrameSource one = prescale_frame(c, F.frame_dev, F.frame_h, F.frame_w, F.ld, F.prescale_w, F.prescale_h, stream,
                                                   (char*)c->list_gray.p + slot[(size_t)f], (const double*)((const char*)c->list_meta.p + off_box) + (size_t)f * 4);
        desc[(size_t)f] = hg::FrameDesc{(const uint8_t*)one.px, one.ld, one.w, one.h, L.first[(size_t)f], L.tab_row[(size_t)f]};
    }
    hg::put_frame_descs(desc.data(), n_frames, (hg::FrameDesc*)c->list_desc.p, st);
    R.fl = hg::FrameList{desc.data(), (const hg::FrameDesc*)c->list_desc.p, n_frames, (const int32_t*)c->list_win.p, total, L.key, L.tab_rows};
    R.tables_dev = (const LevelTable*)c->list_meta.p;
    R.grid_of_dev = (const int32_t*)((const char*)c->list_meta.p + off_grid);
    R.win_frame_dev = (int32_t*)c->list_win.p;
}

}  // namespace

extern "C" {

int hg_cascade_detect_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, const double* boxes_host,
                             const double* level_host, int64_t n0, double* out_coords, double* out_angles, int32_t* out_orig_index,
                             double* out_confidence, int64_t out_cap, int64_t* n_out, int32_t* stage_counts, int64_t* rows_executed,
                             void* stream) {
    return guarded([&] {
        if (c && c->frame_format != HG_FRAME_L && frame_dev && n0 > 0) gray_frame_of(c, frame_dev, frame_h, frame_w, ld, stream, frame_dev, ld);
        run_pass(c, StagePass::boxes(hg::FrameSource::one(frame_dev, frame_h, frame_w, ld), boxes_host, level_host, n0)
                        .to_host(out_coords, out_angles, out_orig_index, out_confidence, out_cap, n_out),
                 stage_counts, rows_executed, stream);
    });
}

int hg_cascade_detect_levels_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, const hg_cascade_level* levels,
                                    int n_levels, double* out_coords, double* out_angles, int32_t* out_orig_index, double* out_confidence,
                                    int64_t out_cap, int64_t* n_out, int32_t* stage_counts, int64_t* rows_executed, void* stream) {
    return guarded([&] {
        const LevelTable T = make_level_table(levels, n_levels);
        if (c && c->frame_format != HG_FRAME_L && frame_dev && T.first[T.n_levels] > 0) gray_frame_of(c, frame_dev, frame_h, frame_w, ld, stream, frame_dev, ld);
        run_pass(c, StagePass::grid(hg::FrameSource::one(frame_dev, frame_h, frame_w, ld), T).to_host(out_coords, out_angles, out_orig_index, out_confidence, out_cap, n_out),
                 stage_counts, rows_executed, stream);
    });
}

int hg_cascade_detect_frame_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h,
                                   const hg_cascade_level* levels, int n_levels, double* out_coords, double* out_angles, int32_t* out_orig_index,
                                   double* out_confidence, int64_t out_cap, int64_t* n_out, int32_t* stage_counts, int64_t* rows_executed, void* stream) {
    return guarded([&] {
        if (!c) hg::fail(HG_ERR_ARG, "null argument");
        const LevelTable T = make_level_table(levels, n_levels);
        const hg::FrameSource fr = prescale_frame(c, frame_dev, frame_h, frame_w, ld, prescale_w, prescale_h, stream);
        run_pass(c, StagePass::grid(fr, T).to_host(out_coords, out_angles, out_orig_index, out_confidence, out_cap, n_out), stage_counts, rows_executed, stream);
    });
}

// prescale + grid + stage loop (as hg_cascade_detect_frame_device), then the eyes, the discard, the rows and the purge on the survivors
// left on the device (hg_eyes.hip), on the frame the cascade read (FaceDetectUpdated.py:947-1041, :1180)
int hg_cascade_detect_faces_frame_device(hg_cascade* c, hg_eyes* e, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w,
                                         int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out,
                                         int64_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed, void* stream) {
    return guarded([&] {
        if (!c || !e || !n_out) hg::fail(HG_ERR_ARG, "null argument");
        if (out_cap < 0) hg::fail(HG_ERR_ARG, "negative output capacity");
        if (hg::eyes_device(e) != c->device) hg::fail(HG_ERR_ARG, "eye handle on device %d, cascade on device %d", hg::eyes_device(e), c->device);
        const LevelTable T = make_level_table(levels, n_levels);
        const StagePass P = StagePass::grid(prescale_frame(c, frame_dev, frame_h, frame_w, ld, prescale_w, prescale_h, stream), T);
        const PassResult r = run_pass(c, P, stage_counts, rows_executed, stream);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, P.frames, survivors_of(c, P, r), (hipStream_t)stream);
        hg::eyes_tail_read(e, tail, out_rows, out_cap, n_out, n_before_purge, (hipStream_t)stream);
    });
}

int hg_cascade_detect_frames_device(hg_cascade* c, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld,
                                    int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_coords, double* out_angles,
                                    int32_t* out_orig_index, double* out_confidence, int64_t out_cap, int32_t* frame_first, int32_t* stage_counts,
                                    int64_t* rows_executed, void* stream) {
    return guarded([&] {
        const LevelTable T = check_frame_stack(c, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_cap,
                                               frame_first);
        StagePass P = StagePass::grid(stack_frames(c, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, stream), T);
        std::vector<int32_t> own_index, first((size_t)n_frames);
        out_orig_index = index_room(out_orig_index, own_index, out_cap, P.n0);
        int64_t n = 0;
        run_pass(c, P.to_host(out_coords, out_angles, out_orig_index, out_confidence, out_cap, &n), stage_counts, rows_executed, stream);
        for (int f = 0; f < n_frames; ++f) first[(size_t)f] = (int32_t)(f * P.period());
        hg::split_by_first(out_orig_index, n, first.data(), n_frames, frame_first);
    });
}

// the pooled stage loop, then the eye step on ALL survivors as one batch and the purge per frame, on the grey stack the cascade read; as
// in hg_cascade_detect_faces_frame_device the host reads nothing between the stage loop's last survivor count and the one read-back of
// the per-frame counts and the rows
int hg_cascade_detect_faces_frames_device(hg_cascade* c, hg_eyes* e, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w,
                                          int64_t ld, int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_rows,
                                          int64_t out_cap, int32_t* frame_first, int32_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed,
                                          void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null argument");
        const LevelTable T = check_frame_stack(c, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_cap,
                                               frame_first);
        if (hg::eyes_device(e) != c->device) hg::fail(HG_ERR_ARG, "eye handle on device %d, cascade on device %d", hg::eyes_device(e), c->device);
        const StagePass P = StagePass::grid(stack_frames(c, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, stream), T);
        const PassResult r = run_pass(c, P, stage_counts, rows_executed, stream);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, P.frames, survivors_of(c, P, r), (hipStream_t)stream);
        hg::eyes_tail_read_frames(tail, out_rows, out_cap, frame_first, n_before_purge, (hipStream_t)stream);
    });
}

int hg_cascade_detect_frame_list_device(hg_cascade* c, const hg_cascade_frame* frames, int n_frames, double* out_coords, double* out_angles,
                                        int32_t* out_orig_index, double* out_confidence, int64_t out_cap, int32_t* frame_first, int32_t* stage_counts,
                                        int64_t* rows_executed, void* stream) {
    return guarded([&] {
        const hg::ListLayout L = check_frame_list(c, nullptr, frames, n_frames, out_cap, frame_first);
        std::vector<hg::FrameDesc> desc;
        ListRun R{};
        list_frames(c, frames, n_frames, L, stream, desc, R);
        StagePass P = StagePass::grid_list(R);
        std::vector<int32_t> own_index;
        out_orig_index = index_room(out_orig_index, own_index, out_cap, P.n0);
        int64_t n = 0;
        run_pass(c, P.to_host(out_coords, out_angles, out_orig_index, out_confidence, out_cap, &n), stage_counts, rows_executed, stream);
        hg::split_by_first(out_orig_index, n, L.first.data(), n_frames, frame_first);
    });
}

// the list's pooled stage loop, then the eye step on ALL survivors as one batch, every eye row cut from its face's own grey frame, and
// the purge per frame
int hg_cascade_detect_faces_frame_list_device(hg_cascade* c, hg_eyes* e, const hg_cascade_frame* frames, int n_frames, double* out_rows, int64_t out_cap,
                                              int32_t* frame_first, int32_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed, void* stream) {
    return guarded([&] {
        if (!e) hg::fail(HG_ERR_ARG, "null argument");
        const hg::ListLayout L = check_frame_list(c, e, frames, n_frames, out_cap, frame_first);
        if (hg::eyes_device(e) != c->device) hg::fail(HG_ERR_ARG, "eye handle on device %d, cascade on device %d", hg::eyes_device(e), c->device);
        std::vector<hg::FrameDesc> desc;
        ListRun R{};
        list_frames(c, frames, n_frames, L, stream, desc, R);
        const StagePass P = StagePass::grid_list(R);
        const PassResult r = run_pass(c, P, stage_counts, rows_executed, stream);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, P.frames, survivors_of(c, P, r), (hipStream_t)stream);
        hg::eyes_tail_read_frames(tail, out_rows, out_cap, frame_first, n_before_purge, (hipStream_t)stream);
    });
}

int hg_cascade_grid_device(int device, const hg_cascade_level* levels, int n_levels, double* boxes_dev, double* level_dev, int64_t cap, int64_t* n0,
                           void* stream) {
    return guarded([&] {
        const LevelTable T = make_level_table(levels, n_levels);
        const int64_t n = T.first[T.n_levels];
        if (n0) *n0 = n;
        if (!boxes_dev && !level_dev) return;      // a query of the window count
        if (!boxes_dev || !level_dev || cap < n) hg::fail(HG_ERR_ARG, "room for %lld windows, the grid has %lld", (long long)cap, (long long)n);
        set_dev(device);
        hipLaunchKernelGGL(k_cascade_init_grid, (unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream, T, boxes_dev, level_dev, (double*)nullptr,
                           (double*)nullptr, (double*)nullptr, (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        HG_HIP(hipGetLastError());
    });
}

}  // extern "C"

// ---- tracking faces across a frame stream (include/higsfa.h) --------------------------------------------------------------------
struct hg_tracker {
    hg_cascade* c = nullptr;
    hg_eyes* e = nullptr;
    hg_tracked_consts tc{};
    int max_faces = 1, rescan_every = 0;
    hg::DevBuf state;                // device: the held boxes (max_faces x 4 doubles), then the carried count (int32)
    int held = 0;                    // host mirror of the carried count: decides which path the next step takes and sizes it
    int tracked_run = 0;             // consecutive tracked steps since the last full-grid step (rescan_every)
    int w = 0, h = 0;                // prescaled frame size the boxes belong to
    char* host_res = nullptr;        // pinned: words {kept, before the purge, carried, sequence number} at 0, rows at 64, slots behind the rows
    int32_t seq = 0;
    int rows_cap() const { return kTracked * max_faces + 1; }      // the purge may keep n + 1 rows
    double* box_dev() const { return (double*)state.p; }
    int32_t* held_dev() const { return (int32_t*)((char*)state.p + (size_t)max_faces * 32); }
};

namespace {
void check_finite_consts(const hg_tracked_consts& t) {
    const double v[6] = {t.subimage_width, t.subimage_height, t.regression_width, t.regression_height, t.net_Dx, t.net_Dy};
    for (double x : v)
        if (!(x > 0.0) || !std::isfinite(x)) hg::fail(HG_ERR_ARG, "tracked-grid constants must be positive and finite");
}

// The hand-over's rule (k_tracker_handover, k_stream_handover) on rows the host has already: of the first min(n, max_faces) rows, those
// whose four box numbers are all finite are carried
int carried_rows(const double* rows, int64_t n, int max_faces) {
    int carried = 0;
    for (int64_t j = 0; j < n && j < max_faces; ++j) {
        bool ok = true;
        for (int q = 0; q < 4 && ok; ++q) ok = std::isfinite(rows[j * 10 + q]);
        carried += ok ? 1 : 0;
    }
    return carried;
}

void tracker_create(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, int max_faces, int rescan_every, hg_tracker** out) {
    if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    // the two numbers first: refused before any handle is looked at
    if (max_faces < 1 || max_faces > kMaxFaces) hg::fail(HG_ERR_ARG, "max_faces %d outside 1..%d", max_faces, kMaxFaces);
    if (rescan_every < 0) hg::fail(HG_ERR_ARG, "negative rescan_every %d", rescan_every);
    if (!c || !e || !consts) hg::fail(HG_ERR_ARG, "null argument");
    check_finite_consts(*consts);
    if (consts->subimage_width != (double)c->w || consts->subimage_height != (double)c->h)
        hg::fail(HG_ERR_ARG, "tracked-grid sub-image %g x %g, the cascade's is %d x %d", consts->subimage_width, consts->subimage_height, c->w, c->h);
    if (hg::eyes_device(e) != c->device) hg::fail(HG_ERR_ARG, "eye handle on device %d, cascade on device %d", hg::eyes_device(e), c->device);
    set_dev(c->device);
    auto t = std::make_unique<hg_tracker>();
    t->c = c;
    t->e = e;
    t->tc = *consts;
    t->max_faces = max_faces;
    t->rescan_every = rescan_every;
    const size_t state_bytes = (size_t)max_faces * 32 + 16;
    t->state.alloc(state_bytes);
    HG_HIP(hipMemset(t->state.p, 0, state_bytes));
    HG_HIP(hipHostMalloc((void**)&t->host_res, 64 + (size_t)t->rows_cap() * 84, hipHostMallocDefault));
    memset(t->host_res, 0, 64);
    *out = t.release();
}

void tracker_step(hg_tracker* t, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h, const hg_cascade_level* levels,
                  int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out, int64_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed,
                  int* used_tracked_grid, int32_t* slots, int* n_held, void* stream) {
    if (!t || !n_out) hg::fail(HG_ERR_ARG, "null argument");
    if (out_cap < 0) hg::fail(HG_ERR_ARG, "negative output capacity");
    hg_cascade* c = t->c;
    hg_eyes* e = t->e;
    hipStream_t st = (hipStream_t)stream;
    *n_out = 0;
    if (n_before_purge) *n_before_purge = 0;
    if (used_tracked_grid) *used_tracked_grid = 0;
    const hg::FrameSource fr = prescale_frame(c, frame_dev, frame_h, frame_w, ld, prescale_w, prescale_h, stream);
    if (t->held && (fr.w != t->w || fr.h != t->h)) t->held = 0;      // the boxes mean nothing on another frame size
    if (n_held) *n_held = t->held;
    // the path rule, on the host: nothing held (a size change drops every box), or rescan_every tracked steps in a row behind us
    if (!t->held || (t->rescan_every > 0 && t->tracked_run >= t->rescan_every)) {
        // what hg_cascade_detect_faces_frame_device runs, then the first rows (if any) become the tracked faces
        const LevelTable T = make_level_table(levels, n_levels);
        const StagePass P = StagePass::grid(fr, T);
        const PassResult r = run_pass(c, P, stage_counts, rows_executed, stream);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, fr, survivors_of(c, P, r), st);
        hg::eyes_tail_read(e, tail, out_rows, out_cap, n_out, n_before_purge, st);
        const int carried = carried_rows(out_rows, *n_out, t->max_faces);
        if (carried) {      // the boxes go from the purge's device rows into the tracker's state, in stream order before the next frame
            hipLaunchKernelGGL(k_tracker_handover, 1, 128, 0, st, tail.purged, tail.counts, t->box_dev(), t->held_dev(), t->max_faces, SlotChain{}, TrackerResults{}, 0);
            HG_HIP(hipGetLastError());
        } else {
            HG_HIP(hipMemsetAsync(t->held_dev(), 0, 4, st));
        }
        t->held = carried;
        t->tracked_run = 0;
        t->w = fr.w;
        t->h = fr.h;
        for (int64_t j = 0; slots && j < *n_out; ++j) slots[j] = -1;      // no held face stands behind a row of the full grid
        if (n_held) *n_held = carried;
        return;
    }
    // the tracked frame: everything enqueued back to back, one wait at the end
    if (used_tracked_grid) *used_tracked_grid = 1;
    const StagePass P = StagePass::tracked(fr, t->tc, t->box_dev(), t->held);
    const PassResult r = run_pass(c, P, stage_counts, rows_executed, stream);
    const hg::EyeTail tail = hg::eyes_tail_enqueue(e, fr, survivors_of(c, P, r), st);
    const SlotChain S{tail.kept_idx, tail.row_src, (const int32_t*)c->oidx[r.cur].p};
    TrackerResults R{};
    R.words = (int32_t*)t->host_res;
    R.rows = (double*)(t->host_res + 64);
    R.cap = t->rows_cap();
    R.slots = (int32_t*)(t->host_res + 64 + (size_t)R.cap * 80);
    const int32_t seq = ++t->seq;
    hipLaunchKernelGGL(k_tracker_handover, 1, 128, 0, st, tail.purged, tail.counts, t->box_dev(), t->held_dev(), t->max_faces, S, R, seq);
    HG_HIP(hipGetLastError());
    try {      // the one wait
        wait_for_seq(R.words + 3, seq, st, "tracked frame did not report its result");
    } catch (...) {
        t->held = 0;
        throw;
    }
    const int64_t kept = R.words[0];
    if (n_before_purge) *n_before_purge = R.words[1];
    t->held = R.words[2];
    ++t->tracked_run;
    if (n_held) *n_held = t->held;      // the hand-over has happened whatever follows
    if (kept > out_cap || kept > R.cap) hg::fail(HG_ERR_ARG, "%lld faces but room for %lld", (long long)kept, (long long)std::min<int64_t>(out_cap, R.cap));
    if (kept > 0) {
        if (!out_rows) hg::fail(HG_ERR_ARG, "null output rows");
        memcpy(out_rows, R.rows, (size_t)kept * 80);
        if (slots) memcpy(slots, R.slots, (size_t)kept * 4);
    }
    *n_out = kept;
}
}  // namespace

extern "C" {

int hg_cascade_tracked_grid_device(int device, const hg_tracked_consts* consts, const double* face_dev, double* boxes_dev, double* level_dev, void* stream) {
    return guarded([&] {
        if (!consts || !face_dev || !boxes_dev || !level_dev) hg::fail(HG_ERR_ARG, "null argument");
        check_finite_consts(*consts);
        set_dev(device);
        hipLaunchKernelGGL(k_cascade_init_tracked, 1, 64, 0, (hipStream_t)stream, *consts, face_dev, boxes_dev, level_dev, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        HG_HIP(hipGetLastError());
    });
}

int hg_cascade_tracked_grid_multi_device(int device, const hg_tracked_consts* consts, const double* faces_dev, int n_faces, double* boxes_dev,
                                         double* level_dev, void* stream) {
    return guarded([&] {
        if (!consts || !faces_dev || !boxes_dev || !level_dev) hg::fail(HG_ERR_ARG, "null argument");
        if (n_faces < 1 || n_faces > 0x7fffffff / kTracked / 4) hg::fail(HG_ERR_ARG, "bad face count %d", n_faces);
        check_finite_consts(*consts);
        set_dev(device);
        hipLaunchKernelGGL(k_cascade_init_tracked_multi, (unsigned)(((int64_t)kTracked * n_faces + 63) / 64), 64, 0, (hipStream_t)stream, *consts, faces_dev,
                           n_faces, boxes_dev, level_dev, (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (int32_t*)nullptr,
                           (int32_t*)nullptr);
        HG_HIP(hipGetLastError());
    });
}

int hg_tracker_create(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, hg_tracker** out) {
    return guarded([&] { tracker_create(c, e, consts, 1, 0, out); });
}

int hg_tracker_create_multi(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, int max_faces, int rescan_every, hg_tracker** out) {
    return guarded([&] { tracker_create(c, e, consts, max_faces, rescan_every, out); });
}

void hg_tracker_free(hg_tracker* t) {
    if (!t) return;
    if (hipSetDevice(t->c->device) == hipSuccess && t->host_res) (void)hipHostFree(t->host_res);
    delete t;
}

int hg_tracker_reset(hg_tracker* t) {
    return guarded([&] {
        if (!t) hg::fail(HG_ERR_ARG, "null tracker handle");
        set_dev(t->c->device);
        HG_HIP(hipMemset(t->held_dev(), 0, 4));      // steps are synchronous: nothing of this tracker is in flight
        t->held = 0;
        t->tracked_run = 0;
        t->w = t->h = 0;
    });
}

int hg_tracker_step_frame_device(hg_tracker* t, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h,
                                 const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out, int64_t* n_before_purge,
                                 int32_t* stage_counts, int64_t* rows_executed, int* used_tracked_grid, void* stream) {
    return guarded([&] {
        tracker_step(t, frame_dev, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_rows, out_cap, n_out, n_before_purge, stage_counts,
                     rows_executed, used_tracked_grid, nullptr, nullptr, stream);
    });
}

int hg_tracker_step_frame_multi_device(hg_tracker* t, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h,
                                       const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out,
                                       int64_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed, int* used_tracked_grid, int32_t* slots,
                                       int* n_held, void* stream) {
    return guarded([&] {
        tracker_step(t, frame_dev, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_rows, out_cap, n_out, n_before_purge, stage_counts,
                     rows_executed, used_tracked_grid, slots, n_held, stream);
    });
}

}  // extern "C"

// ---- tracking faces on a SET of frame streams in one pooled step (include/higsfa.h) ----------------------------------------------------
// Stream s behaves as an hg_tracker of its own fed frame s of every stack.  The streams that hold faces and are not due for a rescan
// (T) share ONE tracked pass — k_cascade_init_tracked_streams, the bounded stage loop over a frame stack, the eye step as one batch, the
// purge per stream, k_stream_handover — enqueued whole; the others (G) share one full-grid pass, what
// hg_cascade_detect_faces_frames_device runs on their frames; the tracked pass's one wait comes last.
struct hg_stream_tracker {
    hg_cascade* c = nullptr;
    hg_eyes* e = nullptr;
    hg_tracked_consts tc{};
    int n_streams = 0, max_faces = 1, rescan_every = 0;
    hg::DevBuf state;                   // device: the held boxes (n_streams x max_faces x 4 doubles), then the carried counts (n_streams int32)
    std::vector<int> held, run;         // per stream: host mirror of the carried count; consecutive tracked steps since the last full-grid step
    int w = 0, h = 0;                   // prescaled frame size the boxes belong to
    // pinned: the sequence word at 0; from 64 on the rows (n_streams x rows_cap x 10 doubles), the words (n_streams x {kept, before the
    // purge, carried, 0}), the slots (n_streams x rows_cap) and the streams of the full-grid pass's segments (n_streams)
    char* host_res = nullptr;
    int32_t seq = 0;
    int rows_cap() const { return kTracked * max_faces + 1; }      // the purge may keep n + 1 rows of a stream
    double* box_dev() const { return (double*)state.p; }
    int32_t* held_dev() const { return (int32_t*)((char*)state.p + (size_t)n_streams * max_faces * 32); }
    double* res_rows() const { return (double*)(host_res + 64); }
    int32_t* res_words() const { return (int32_t*)(host_res + 64 + (size_t)n_streams * rows_cap() * 80); }
    int32_t* res_slots() const { return res_words() + (size_t)n_streams * 4; }
    int32_t* res_gmap() const { return res_slots() + (size_t)n_streams * rows_cap(); }
    size_t res_bytes() const { return 64 + (size_t)n_streams * rows_cap() * 84 + (size_t)n_streams * 20; }
    void forget() {      // after a failed step: nothing is held anywhere (the device counts go to 0 in stream order, best effort)
        std::fill(held.begin(), held.end(), 0);
        std::fill(run.begin(), run.end(), 0);
        w = h = 0;
        if (state.p) (void)hipMemset(held_dev(), 0, (size_t)n_streams * 4);
    }
};

namespace {
// the numbers of a stream set, refused before any handle is looked at
void check_stream_set(int n_streams, int max_faces, int rescan_every) {
    if (n_streams < 1 || n_streams > HG_MAX_STACK_FRAMES) hg::fail(HG_ERR_ARG, "n_streams %d outside 1..%d", n_streams, HG_MAX_STACK_FRAMES);
    if (max_faces < 1 || max_faces > kMaxFaces) hg::fail(HG_ERR_ARG, "max_faces %d outside 1..%d", max_faces, kMaxFaces);
    // the bounded stage loop pads its filler rows on k_cascade_group's single-workgroup path only (pad_to); above 2 * kChunk
    // candidates run_groups takes the two-launch chunk path, which has no padding
    if ((int64_t)kTracked * n_streams * max_faces > HG_MAX_STREAM_WINDOWS)
        hg::fail(HG_ERR_ARG, "%d streams of %d faces: %lld tracked windows, at most %d", n_streams, max_faces, (long long)kTracked * n_streams * max_faces,
                 HG_MAX_STREAM_WINDOWS);
    if (rescan_every < 0) hg::fail(HG_ERR_ARG, "negative rescan_every %d", rescan_every);
}
static_assert(HG_MAX_STREAM_WINDOWS == 2 * kChunk, "the stream set's window bound is k_cascade_group's single-workgroup path");

void stream_tracker_step(hg_stream_tracker* t, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld, int prescale_w,
                         int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int32_t* stream_first,
                         int32_t* n_before_purge, int32_t* used_tracked_grid, int32_t* n_held, int32_t* slots, int64_t* rows_executed, void* stream) {
    const int Bn = t->n_streams, K = t->max_faces;
    hg_cascade* c = t->c;
    hg_eyes* e = t->e;
    hipStream_t st = (hipStream_t)stream;
    const LevelTable T = check_frame_stack(c, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_cap,
                                           stream_first);
    set_dev(c->device);
    const bool pre = prescale_w > 0 || prescale_h > 0, conv = pre || c->frame_format != HG_FRAME_L;
    const int oh = pre ? prescale_h : frame_h, ow = pre ? prescale_w : frame_w;
    const size_t slot = (size_t)oh * ow;
    // a change of the prescaled size drops every stream's boxes: they mean nothing on another size
    if (ow != t->w || oh != t->h) {
        bool any = false;
        for (int s = 0; s < Bn; ++s) any = any || t->held[(size_t)s];
        if (any) HG_HIP(hipMemsetAsync(t->held_dev(), 0, (size_t)Bn * 4, st));
        std::fill(t->held.begin(), t->held.end(), 0);
    }
    t->w = ow;
    t->h = oh;
    // the path rule per stream, on the host: nothing held, or rescan_every tracked steps in a row behind it
    std::vector<int> in_g((size_t)Bn), gs;      // gs: the streams of the full-grid pass, in order
    int64_t held_sum = 0;
    for (int s = 0; s < Bn; ++s) {
        in_g[(size_t)s] = !t->held[(size_t)s] || (t->rescan_every > 0 && t->run[(size_t)s] >= t->rescan_every);
        if (in_g[(size_t)s]) gs.push_back(s);
        else held_sum += t->held[(size_t)s];
    }
    const int nG = (int)gs.size(), nT = Bn - nG;
    // the grey frames both passes read.  The tracked pass cuts row i from frame (its stream), so stream s's frame is frame s of its stack;
    // the full-grid pass reads a dense stack of ITS streams' frames.  Prescaled / converted: every frame goes through prescale_frame once,
    // a tracked stream's into slot s, a full-grid stream's into slot n_streams + its position.  Grey frames as they are: read in place,
    // and the full-grid pass's copied together unless they are all the frames or one
    const void *fr_t = frames_dev, *fr_g = frames_dev;
    int64_t stride_t = frame_stride, stride_g = frame_stride, fld_t = ld, fld_g = ld;
    if (conv) {
        c->frame_stack.alloc(slot * 2 * Bn);
        for (int s = 0, g = 0; s < Bn; ++s) {
            const size_t at = in_g[(size_t)s] ? (size_t)Bn + g++ : (size_t)s;
            prescale_frame(c, (const char*)frames_dev + (int64_t)s * frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, stream,
                           (char*)c->frame_stack.p + slot * at);
        }
        fr_t = c->frame_stack.p;
        fr_g = (const char*)c->frame_stack.p + slot * Bn;
        stride_t = stride_g = (int64_t)slot;
        fld_t = fld_g = ow;
    } else if (nG == 1) {
        fr_g = (const char*)frames_dev + (int64_t)gs[0] * frame_stride;
    } else if (nG > 0 && nG < Bn) {
        c->frame_stack.alloc(slot * Bn);
        for (int g = 0; g < nG; ++g)
            HG_HIP(hipMemcpy2DAsync((char*)c->frame_stack.p + slot * g, (size_t)ow, (const char*)frames_dev + (int64_t)gs[(size_t)g] * frame_stride, (size_t)ld,
                                    (size_t)ow, (size_t)oh, hipMemcpyDeviceToDevice, st));
        fr_g = c->frame_stack.p;
        stride_g = (int64_t)slot;
        fld_g = ow;
    }
    int64_t rows_t = 0, rows_g = 0;
    const int cap = t->rows_cap();
    int32_t seq = 0;
    // 1. the tracked pass, enqueued whole: no count is read back, its one wait is the last thing this call does
    if (nT) {
        for (int s : gs)      // due for a rescan: its boxes take no part (the full-grid pass's hand-over writes the count again)
            if (t->held[(size_t)s]) HG_HIP(hipMemsetAsync(t->held_dev() + s, 0, 4, st));
        const StagePass P = StagePass::tracked(hg::FrameSource::stack(fr_t, oh, ow, fld_t, Bn, stride_t), t->tc, t->box_dev(), (int)held_sum, t->held_dev(), K);
        const PassResult r = run_pass(c, P, nullptr, &rows_t, stream);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, P.frames, survivors_of(c, P, r), st);
        const SlotChain S{tail.kept_idx, tail.row_src, (const int32_t*)c->oidx[r.cur].p};
        TrackerResults R{};
        R.words = t->res_words();
        R.rows = t->res_rows();
        R.slots = t->res_slots();
        R.cap = cap;
        seq = ++t->seq;
        hipLaunchKernelGGL(k_stream_handover, (unsigned)Bn, 128, 0, st, tail.purged, tail.seg_first, tail.seg_kept, (const int32_t*)nullptr, t->box_dev(), t->held_dev(),
                           K, S, (int)P.period(), R);
        hipLaunchKernelGGL(k_publish_seq, 1, 1, 0, st, (int32_t*)t->host_res, seq);
        HG_HIP(hipGetLastError());
    }
    // 2. the full-grid pass on the other streams' frames; its kernels follow the tracked pass's hand-over in stream order, so the
    // workspaces of the two handles serve both
    std::vector<double> g_rows;
    std::vector<int32_t> g_first((size_t)nG + 1, 0), g_before((size_t)nG, 0);
    if (nG) {
        const StagePass P = StagePass::grid(hg::FrameSource::stack(fr_g, oh, ow, fld_g, nG, stride_g), T);
        const PassResult r = run_pass(c, P, nullptr, &rows_g, stream);
        g_rows.resize((size_t)(r.n + nG) * 10);
        const hg::EyeTail tail = hg::eyes_tail_enqueue(e, P.frames, survivors_of(c, P, r), st);
        hg::eyes_tail_read_frames(tail, g_rows.data(), r.n + nG, g_first.data(), g_before.data(), st);
        if (r.n > 0) {      // the first rows of every stream become its held faces: the purge's device rows into the state, in stream order
            int32_t* gmap = t->res_gmap();      // (the read above has synchronised the stream: no earlier kernel still reads it)
            for (int g = 0; g < nG; ++g) gmap[g] = gs[(size_t)g];
            hipLaunchKernelGGL(k_stream_handover, (unsigned)nG, 128, 0, st, tail.purged, tail.seg_first, tail.seg_kept, (const int32_t*)gmap, t->box_dev(),
                               t->held_dev(), K, SlotChain{}, kTracked * K, TrackerResults{});
            HG_HIP(hipGetLastError());
        } else if (nG == Bn) {
            HG_HIP(hipMemsetAsync(t->held_dev(), 0, (size_t)Bn * 4, st));
        } else {
            for (int s : gs) HG_HIP(hipMemsetAsync(t->held_dev() + s, 0, 4, st));
        }
        for (int g = 0; g < nG; ++g) {
            const int s = gs[(size_t)g];
            t->held[(size_t)s] = carried_rows(g_rows.data() + (size_t)g_first[(size_t)g] * 10, g_first[(size_t)g + 1] - g_first[(size_t)g], K);
            t->run[(size_t)s] = 0;
        }
    }
    // 3. the one wait of the tracked pass
    if (nT) {
        wait_for_seq((const int32_t*)t->host_res, seq, st, "tracked pass did not report its result");
        const int32_t* words = t->res_words();
        for (int s = 0; s < Bn; ++s) {
            if (in_g[(size_t)s]) continue;
            const int32_t kept = words[s * 4], before = words[s * 4 + 1], carried = words[s * 4 + 2];
            if (kept < 0 || kept > cap || before < 0 || carried < 0 || carried > K) hg::fail(HG_ERR_STATE, "stream %d: bad counts from the device", s);
            t->held[(size_t)s] = carried;
            ++t->run[(size_t)s];
        }
    }
    // both hand-overs have happened: the state is valid whatever follows
    int64_t total_kept = 0;
    for (int s = 0, g = 0; s < Bn; ++s) {
        if (n_held) n_held[s] = t->held[(size_t)s];
        if (used_tracked_grid) used_tracked_grid[s] = in_g[(size_t)s] ? 0 : 1;
        total_kept += in_g[(size_t)s] ? g_first[(size_t)g + 1] - g_first[(size_t)g] : t->res_words()[s * 4];
        g += in_g[(size_t)s];
    }
    if (rows_executed) *rows_executed = rows_t + rows_g;
    if (total_kept > out_cap) {
        for (int s = 0; s <= Bn; ++s) stream_first[s] = 0;
        hg::fail(HG_ERR_ARG, "%lld faces but room for %lld", (long long)total_kept, (long long)out_cap);
    }
    if (total_kept > 0 && !out_rows) hg::fail(HG_ERR_ARG, "null output rows");
    int64_t at = 0;
    for (int s = 0, g = 0; s < Bn; ++s) {
        stream_first[s] = (int32_t)at;
        if (in_g[(size_t)s]) {
            const int64_t lo = g_first[(size_t)g], m = g_first[(size_t)g + 1] - lo;
            if (m) memcpy(out_rows + at * 10, g_rows.data() + (size_t)lo * 10, (size_t)m * 80);
            for (int64_t j = 0; slots && j < m; ++j) slots[at + j] = -1;      // no held face stands behind a row of the full grid
            if (n_before_purge) n_before_purge[s] = g_before[(size_t)g];
            at += m;
            ++g;
        } else {
            const int64_t m = t->res_words()[s * 4];
            if (m) memcpy(out_rows + at * 10, t->res_rows() + (size_t)s * cap * 10, (size_t)m * 80);
            if (m && slots) memcpy(slots + at, t->res_slots() + (size_t)s * cap, (size_t)m * 4);
            if (n_before_purge) n_before_purge[s] = t->res_words()[s * 4 + 1];
            at += m;
        }
    }
    stream_first[Bn] = (int32_t)at;
}
}  // namespace

extern "C" {

int hg_cascade_tracked_grid_streams_device(int device, const hg_tracked_consts* consts, const double* faces_dev, const int32_t* held_dev, int n_streams,
                                           int max_faces, double* boxes_dev, double* level_dev, void* stream) {
    return guarded([&] {
        if (n_streams < 1 || n_streams > HG_MAX_STACK_FRAMES) hg::fail(HG_ERR_ARG, "n_streams %d outside 1..%d", n_streams, HG_MAX_STACK_FRAMES);
        if (max_faces < 1 || max_faces > kMaxFaces) hg::fail(HG_ERR_ARG, "max_faces %d outside 1..%d", max_faces, kMaxFaces);
        if (!consts || !faces_dev || !held_dev || !boxes_dev || !level_dev) hg::fail(HG_ERR_ARG, "null argument");
        check_finite_consts(*consts);
        set_dev(device);
        hipLaunchKernelGGL(k_cascade_init_tracked_streams, 1, 1024, 0, (hipStream_t)stream, *consts, faces_dev, held_dev, n_streams, max_faces, boxes_dev, level_dev,
                           (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        HG_HIP(hipGetLastError());
    });
}

int hg_stream_tracker_create(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, int n_streams, int max_faces, int rescan_every,
                             hg_stream_tracker** out) {
    return guarded([&] {
        if (!out) hg::fail(HG_ERR_ARG, "null output handle pointer");
        *out = nullptr;
        check_stream_set(n_streams, max_faces, rescan_every);
        if (!c || !e || !consts) hg::fail(HG_ERR_ARG, "null argument");
        check_finite_consts(*consts);
        if (consts->subimage_width != (double)c->w || consts->subimage_height != (double)c->h)
            hg::fail(HG_ERR_ARG, "tracked-grid sub-image %g x %g, the cascade's is %d x %d", consts->subimage_width, consts->subimage_height, c->w, c->h);
        if (hg::eyes_device(e) != c->device) hg::fail(HG_ERR_ARG, "eye handle on device %d, cascade on device %d", hg::eyes_device(e), c->device);
        set_dev(c->device);
        auto t = std::make_unique<hg_stream_tracker>();
        t->c = c;
        t->e = e;
        t->tc = *consts;
        t->n_streams = n_streams;
        t->max_faces = max_faces;
        t->rescan_every = rescan_every;
        t->held.assign((size_t)n_streams, 0);
        t->run.assign((size_t)n_streams, 0);
        const size_t state_bytes = (size_t)n_streams * max_faces * 32 + (size_t)n_streams * 4;
        t->state.alloc(state_bytes);
        HG_HIP(hipMemset(t->state.p, 0, state_bytes));
        HG_HIP(hipHostMalloc((void**)&t->host_res, t->res_bytes(), hipHostMallocDefault));
        memset(t->host_res, 0, t->res_bytes());
        *out = t.release();
    });
}

void hg_stream_tracker_free(hg_stream_tracker* t) {
    if (!t) return;
    if (hipSetDevice(t->c->device) == hipSuccess && t->host_res) (void)hipHostFree(t->host_res);
    delete t;
}

int hg_stream_tracker_reset(hg_stream_tracker* t, int stream_index) {
    return guarded([&] {
        if (!t) hg::fail(HG_ERR_ARG, "null tracker handle");
        if (stream_index < -1 || stream_index >= t->n_streams) hg::fail(HG_ERR_ARG, "stream %d of %d (-1: all)", stream_index, t->n_streams);
        set_dev(t->c->device);
        if (stream_index < 0) {      // steps are synchronous: nothing of this tracker is in flight
            HG_HIP(hipMemset(t->held_dev(), 0, (size_t)t->n_streams * 4));
            std::fill(t->held.begin(), t->held.end(), 0);
            std::fill(t->run.begin(), t->run.end(), 0);
            t->w = t->h = 0;
        } else {
            HG_HIP(hipMemset(t->held_dev() + stream_index, 0, 4));
            t->held[(size_t)stream_index] = 0;
            t->run[(size_t)stream_index] = 0;
        }
    });
}

int hg_stream_tracker_step_frames_device(hg_stream_tracker* t, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w, int64_t ld,
                                         int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap,
                                         int32_t* stream_first, int32_t* n_before_purge, int32_t* used_tracked_grid, int32_t* n_held, int32_t* slots,
                                         int64_t* rows_executed, void* stream) {
    return guarded([&] {
        // the numbers first, then the handle
        if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) hg::fail(HG_ERR_ARG, "%d frames in a stack (1..%d)", n_frames, HG_MAX_STACK_FRAMES);
        check_frame_geometry(frame_h, frame_w, ld);
        if (frame_stride < (int64_t)(frame_h - 1) * ld + frame_w)
            hg::fail(HG_ERR_ARG, "frames %lld bytes apart, a frame reaches over %lld", (long long)frame_stride, (long long)((int64_t)(frame_h - 1) * ld + frame_w));
        if (out_cap < 0) hg::fail(HG_ERR_ARG, "negative output capacity");
        if (!t || !stream_first) hg::fail(HG_ERR_ARG, "null argument");
        if (n_frames != t->n_streams) hg::fail(HG_ERR_ARG, "%d frames for a set of %d streams", n_frames, t->n_streams);
        try {
            stream_tracker_step(t, frames_dev, n_frames, frame_stride, frame_h, frame_w, ld, prescale_w, prescale_h, levels, n_levels, out_rows, out_cap,
                                stream_first, n_before_purge, used_tracked_grid, n_held, slots, rows_executed, stream);
        } catch (const hg::Error& err) {
            if (err.code != HG_ERR_ARG) t->forget();      // (a refused argument launched nothing, or came after both hand-overs)
            throw;
        } catch (...) {
            t->forget();
            throw;
        }
    });
}

}  // extern "C"
