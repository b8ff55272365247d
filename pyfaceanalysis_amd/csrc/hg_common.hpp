// Shared host-side definitions: error reporting, the parsed flow tree, the executor interface.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/higsfa.h"

namespace hg {

// ---- errors ---------------------------------------------------------------------------------
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(code, buf);
}

#define HG_HIP(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            ::hg::fail(HG_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                       __FILE__, __LINE__);                                                \
    } while (0)

// ---- parsed flow tree (mirrors pyfaceanalysis_amd/blob.py) -----------------------------------
enum NodeKind : uint32_t {
    K_FLOW = 1, K_SWITCHBOARD = 2, K_LAYER = 3, K_CLONELAYER = 4, K_AFFINE = 5, K_EXPANSION = 6,
    K_IGSFA = 7, K_IDENTITY = 8, K_HEAD = 9, K_CUTOFF = 10, K_FLOWNODE = 11
};
enum ExpKind : uint32_t { E_IDENTITY = 0, E_ABS_POW = 1, E_SIGNED_POW = 2, E_QUADRATIC = 3, E_PAIR_ADJ = 4, E_PAIR_BAND = 5 };
// E_PAIR_ADJ / E_PAIR_BAND: the two readings of cuicuilco's pair_prodsadj{k}_ex (nodes.pair_prodsadj_ex): x_i x_{i+k} only, or the
// reflexive band of offsets 0 .. k-1 stacked offset-major (squares first)

struct ExpFunc {
    uint32_t kind, sel, k;
    double expo;
    // columns the function reads: the first `sel` (cuicuilco's sel_exp(n, f) slices x[:, :n], which numpy clamps), 0 = all.
    // Compared unsigned: a huge sel clamps to d instead of turning negative.
    int used(int d) const { return sel > 0 && sel < (uint32_t)d ? (int)sel : d; }
    int out_dim(int d) const {
        int u = used(d);
        if (kind <= E_SIGNED_POW) return u;
        if (kind == E_QUADRATIC) return u * (u + 1) / 2;
        if (kind == E_PAIR_BAND) {
            int w = 0;
            for (int off = 0; off < (int)k && off < u; ++off) w += u - off;
            return w;
        }
        return u - (int)k > 0 ? u - (int)k : 0;
    }
};

struct TNode {
    uint32_t kind = 0, in_dim = 0, out_dim = 0, aux = 0;
    std::vector<std::unique_ptr<TNode>> ch;  // FLOW / LAYER / FLOWNODE children; CLONELAYER: one
    std::vector<int32_t> conn;               // SWITCHBOARD
    std::vector<double> a, W, b;             // AFFINE: y = (x - a) W + b, W row-major in x out
    std::vector<ExpFunc> funcs;              // EXPANSION
    std::vector<double> x_mean, magn;        // IGSFA
    std::unique_ptr<TNode> exp_node, sfa, lr, pca;
    double lo = 0, hi = 0;                   // CUTOFF
};

std::unique_ptr<TNode> parse_blob(const void* blob, size_t nbytes);
int64_t tree_flops(const TNode& n);
const char* kind_name(uint32_t kind);

// ---- executor interface ----------------------------------------------------------------------
struct StageProfile {
    std::string name;
    double total_ms = 0;
    int64_t launches = 0;
};

class Executor {
public:
    virtual ~Executor() {}
    virtual int plan_kind() const = 0;
    virtual int n_stages() const = 0;
    virtual std::string stage_name(int i) const = 0;
    virtual std::string describe() const = 0;
    virtual int64_t weight_bytes() const = 0;
    virtual int64_t padded_flops_per_row() const { return 0; }
    virtual int64_t workspace_bytes() const = 0;
    virtual void to_device() = 0;                 // current device already set
    virtual void reserve(int64_t rows) = 0;
    // Enqueue on `stream`.  When ev != nullptr it holds n_stages()+1 events to record around stages.
    virtual void run(const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype,
                     int64_t y_cols, int64_t ldy, hipStream_t stream, hipEvent_t* ev) = 0;
    // Lanes (hg_flow_set_lanes): n copies of everything a call WRITES — activation workspace, tile-queue counters and their
    // host-tracked base, the host-visible error word — over one copy of what it only reads (weights, tables, plans), so that
    // run_lane(0, ...) and run_lane(1, ...) may be in flight on two streams at once.  run() is run_lane(0, ...).  false: this
    // plan keeps one set of state (the caller stays serial).  Only called while nothing of this executor is in flight.
    virtual bool set_lanes(int n) { return n == 1; }
    virtual int lanes() const { return 1; }
    // Never profiled.  A lane whose workspace has to grow waits for `stream` first: the lane's earlier steps ran there.
    virtual void run_lane(int lane, const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype, int64_t y_cols,
                          int64_t ldy, hipStream_t stream) {
        if (lane != 0) fail(HG_ERR_STATE, "this plan has one lane");
        run(x, x_dtype, n, ldx, y, y_dtype, y_cols, ldy, stream, nullptr);
    }
    virtual void check_errors() {}                // after a synchronisation: did a kernel of an earlier run (any lane) report a failure?
    virtual void release() = 0;                   // free device memory
};

std::unique_ptr<Executor> make_generic_executor(const TNode& root);
// Returns nullptr (and a reason) when the flow does not have the regular structure the fused
// MFMA kernels need; the caller then falls back to the generic executor.
std::unique_ptr<Executor> make_fused_executor(const TNode& root, std::string* why_not);

inline size_t dtype_size(int dt) {
    switch (dt) {
        case HG_U8: return 1;
        case HG_F32: return 4;
        case HG_F64: return 8;
        default: fail(HG_ERR_ARG, "unknown dtype %d", dt);
    }
}

// RAII device buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    void alloc(size_t n) {
        if (n <= bytes && p) return;
        free();
        if (n == 0) return;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            bytes = 0;
            fail(HG_ERR_NOMEM, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        }
        bytes = n;
    }
    void upload(const void* src, size_t n) {
        alloc(n);
        if (n) HG_HIP(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    }
    void free() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    ~DevBuf() { free(); }
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// hg_extract.hip: the one place that chooses the extraction kernels, for the C entries and for hg_cascade.hip.  filter NEAREST: the
// existing entries (hg_patcher_extract_keyed_device when key != 0 and there are no angles, else hg_patcher_extract_rotate_device);
// BILINEAR / BICUBIC: the filtered tables and gathers, with the same per-key table reuse for unrotated boxes (key = 0: none).
int patcher_extract(hg_patcher* p, uint64_t key, int filter, const void* frame_dev, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                    const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo,
                    void* stream);
// hg_extract.hip: the same dispatch over a STACK of n_frames grey uint8 frames of one size, frame_stride bytes apart
// (hg_patcher_extract_frames_device): row i is cut from frame row_frame_dev[i] / row_div, a row whose frame lies outside the stack is
// all zero.  key != 0, no angles and 0 < tab_n < n: the boxes repeat with period tab_n (one frame's grid copied per frame) and the keyed
// tables of the first tab_n serve all of them.  The pooled cascade passes its original-window indices with row_div = n0, the pooled eye
// step a frame index per eye row with row_div = 1.
int patcher_extract_frames(hg_patcher* p, uint64_t key, int64_t tab_n, int filter, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                           int frame_w, int64_t ld, const double* boxes_dev, const double* delta_angs_dev, const int32_t* row_frame_dev, int row_div, int64_t n,
                           int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);
// hg_extract.hip: the same dispatch over a LIST of grey uint8 frames of DIFFERENT sizes (hg_patcher_extract_frame_list_device, and the
// list pass of hg_cascade.hip / hg_eyes.hip).  One descriptor per frame, the same struct on the host and in the device table.
struct FrameDesc {
    const uint8_t* px;      // the frame's first pixel (device memory)
    int64_t ld;             // row stride
    int32_t w, h;
    int32_t first;          // the frame's first original window in the concatenated grids (0 where the caller has none)
    int32_t tab_row;        // the first row of the frame's grid in the list's shared first-stage tables
};
struct FrameList {
    const FrameDesc* host;           // n_frames descriptors, read before the call returns
    const FrameDesc* dev;            // the same table on the device, or nullptr: the call sends `host` itself, in stream order
    int n_frames;
    const int32_t* win_frame_dev;    // original window -> frame (n_windows entries): row_frame_dev then holds original-window indices;
    int64_t n_windows;               //   nullptr: row_frame_dev holds the frame index of every row
    // key != 0 (never with angles): boxes_dev holds the n_windows concatenated grids themselves, row i = original window i.  Their
    // tables — tab_rows rows, frame f's from tab_row on, shared by frames of equal grids — are kept in ONE buffer for the whole call
    // (not in the keyed ring, which has four slots and evicts) and across calls while the key, a key of the whole list, stays.
    uint64_t key;
    int64_t tab_rows;
};
// descriptors in host memory -> a device table, carried in kernel arguments (consumed at the launch, ordered on the stream)
void put_frame_descs(const FrameDesc* host, int n_frames, FrameDesc* dev, hipStream_t st);
int patcher_extract_frame_list(hg_patcher* p, const FrameList& fl, int filter, const double* boxes_dev, const double* delta_angs_dev,
                               const int32_t* row_frame_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);

// The grey uint8 frames a pass reads (the cascade's stage loop, the eye step), one of: ONE frame; a STACK of n_frames frames of one
// size, `stride` bytes apart, px its frame 0 (a stack of one frame is still a stack: it runs the stack's kernels); a LIST of frames
// of different sizes, alive while the source is used — px .. ld are then its frame 0's, what the kernels' own frame arguments carry.
struct FrameSource {
    enum Kind { ONE, STACK, LIST } kind = ONE;
    const void* px = nullptr;
    int h = 0, w = 0;
    int64_t ld = 0;
    int n_frames = 1;
    int64_t stride = 0;
    const FrameList* list = nullptr;
    static FrameSource one(const void* px, int h, int w, int64_t ld) { return {ONE, px, h, w, ld}; }
    static FrameSource stack(const void* px, int h, int w, int64_t ld, int n_frames, int64_t stride) { return {STACK, px, h, w, ld, n_frames, stride}; }
    static FrameSource of_list(const FrameList& fl) {
        const FrameDesc d0 = fl.host && fl.n_frames > 0 ? fl.host[0] : FrameDesc{};
        return {LIST, d0.px, d0.h, d0.w, d0.ld, fl.n_frames, 0, &fl};
    }
};
// How row i of a batch finds its frame in a source of several.  windows: index_dev holds the cascade's original-window indices — a
// stack's frame is index / period (period: the windows of one frame, and under a key the tables of the first `period` boxes serve every
// frame's copy of them), a list's is win_frame_dev[index]; else (the eye step) index_dev holds the frame index of every row itself.
struct RowFrames {
    const int32_t* index_dev;
    bool windows;
    int64_t period;
};
// hg_extract.hip: whichever of the three dispatches above the source calls for.  key (0: none): as for patcher_extract; a list's shared
// first-stage tables are kept under it (the key of the whole list) and are not looked at without it.  A single frame ignores `rows`.
int patcher_extract_source(hg_patcher* p, const FrameSource& src, uint64_t key, RowFrames rows, int filter, const double* boxes_dev, const double* delta_angs_dev,
                           int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);
// hg_extract.hip: NEAREST, unrotated windows from a frame of format HG_FRAME_* (ld_bytes: row stride in bytes), the tables kept under
// `key` as above.  What hg_patcher_extract_format_device (key = 0) and the cascade's prescale of a colour frame call.
int patcher_extract_format(hg_patcher* p, uint64_t key, int format, const void* frame_dev, int frame_h, int frame_w, int64_t ld_bytes, const double* boxes_dev,
                           int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);

// hg_resample.hip: PIL's filtered resize (hg_patcher_resize_device).  Its state hangs off the patcher (hg_extract.hip keeps the pointer and
// frees it with the handle through resample_state_free).
void resample_state_free(void* state);
void*& patcher_resample_state(hg_patcher* p);
int patcher_device(const hg_patcher* p);
// hg_normalize.hip: pose-normalised face crops (hg_patcher_normalize_device); its state hangs off the patcher the same way.
void normalize_state_free(void* state);
void*& patcher_normalize_state(hg_patcher* p);

// hg_eyes.hip: the tail of every faces entry and tracker step of hg_cascade.hip — the eye step on the cascade's survivors as ONE
// batch, the discard, the 10-column rows and the purge, all enqueued on the stream; a reader then fetches the result, or the caller's
// own last kernel does (the trackers' hand-over).  The survivors are device arrays, ordered by frame (the compaction keeps the
// candidates' order).  A row's frame is read off its original window: index / period in a stack, win_frame_dev[index] in a list.
struct EyeSurvivors {
    const double *boxes, *angles, *conf;
    const int32_t* orig_index;
    int64_t period;           // a stack: original windows per frame
    int64_t n;                // their number — or, with n_dev, the host's bound of it (>= 1): every launch is sized by the bound
    const int32_t* n_dev;     // nullable: the live count is this device word and NOTHING is read back.  Rows between the live count and
                              // the bound carry index 0 (frame 0) and a window k_eye_boxes replaces; a live count of 0 runs through
                              // every launch and gives counts of 0.  The kept indices a tracker's slots are made of are written then.
};
// What a tail leaves on the device until the handle's next call.  One frame: the purge ran once, `purged` holds the kept rows (room for
// n + 1) and counts = {faces after the discard, faces after the purge}.  A stack or a list: the purge ran PER FRAME (it is a per-image
// rule), frame f's kept rows start at row seg_first[f] + f of `purged`, seg_kept[f] of them, out of seg_first[f + 1] - seg_first[f]
// assembled rows; seg_kept follows seg_first (n_frames + 1 words) in memory.  row_src: for every assembled row the survivor it was made
// from; kept_idx (with n_dev only): for every kept row the assembled row it is — per frame from entry seg_first[f] + f on and relative
// to the frame's first row.  n == 0: nothing was launched and every pointer is null.
struct EyeTail {
    const double* purged;
    const int32_t *counts, *seg_first, *seg_kept, *row_src, *kept_idx;
    int n_frames;
    int64_t n;
};
EyeTail eyes_tail_enqueue(hg_eyes* e, const FrameSource& src, const EyeSurvivors& s, hipStream_t st);
// The one read-back of a single frame's tail (n_out, n_before_purge: zero when there were no survivors) ...
void eyes_tail_read(hg_eyes* e, const EyeTail& t, double* out_rows, int64_t out_cap, int64_t* n_out, int64_t* n_before_purge, hipStream_t st);
// ... and of a pooled one: frame f's kept rows are out_rows[frame_first[f] .. frame_first[f + 1]); n_before_purge (n_frames, nullable)
void eyes_tail_read_frames(const EyeTail& t, double* out_rows, int64_t out_cap, int32_t* frame_first, int32_t* n_before_purge, hipStream_t st);
int eyes_device(const hg_eyes* e);
int eyes_filter(const hg_eyes* e);

}  // namespace hg
