// The host-only part of the frame-LIST pass (include/higsfa.h, hg_cascade_detect_frame_list_device): what a list of hg_cascade_frame is
// refused for, and the layout of its concatenated grids — first[], the distinct level tables, the rows of the shared first-stage tables
// and the key of the whole list — and what every pooled pass (stack or list) does on the host with what comes back: the split of the
// survivors by frame, the bounds of an eye tail's segment words and the layout of its rows.  No HIP in here: hg_cascade.hip and
// hg_eyes.hip include it, and tests/frame_list_driver.cpp and tests/pass_split_driver.cpp run it under the sanitizers on their own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/higsfa.h"

namespace hg {

constexpr int64_t kListMaxWindows = 0x7fffffffll / 64;      // the window bound of every cascade entry
constexpr int kListMaxLevels = 32;

struct ListLayout {
    std::vector<int32_t> first;         // n_frames + 1: first original window of every frame, and the total
    std::vector<int32_t> grid;          // per frame: which distinct grid it has (0 .. n_grids - 1, numbered by first appearance)
    std::vector<int32_t> tab_row;       // per frame: first row of its grid in the shared tables (equal for frames of one grid)
    std::vector<int32_t> grid_frame;    // per distinct grid: the first frame that has it
    std::vector<int32_t> gw, gh;        // per frame: the size of the frame its grid is laid over (the prescaled size, or the frame's)
    int64_t tab_rows = 0;               // rows of the shared tables: the sum of the distinct grids' windows
    uint64_t key = 0;                   // FNV-1a over every frame's own size, grid size and grid number, and every distinct level table
};

inline uint64_t list_fnv(const void* p, size_t n, uint64_t h) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

// What ANY list entry refuses about frame f of a list (the patcher's hg_frame_ref and the cascade's hg_cascade_frame alike): "" or the
// reason, naming the frame.  bpp: bytes per pixel (ld is in bytes).
inline std::string list_frame_refusal(int f, const void* px, int frame_h, int frame_w, int64_t ld, int bpp) {
    char msg[256];
    if (frame_h <= 0 || frame_w <= 0 || ld < (int64_t)frame_w * bpp) {
        snprintf(msg, sizeof msg, "frame %d of the list: bad frame geometry: %d rows of %d pixels of %d byte(s), %lld apart", f, frame_h, frame_w, bpp, (long long)ld);
        return msg;
    }
    if (!px) {
        snprintf(msg, sizeof msg, "frame %d of the list: null data pointer", f);
        return msg;
    }
    return "";
}
// ... and a rotated NEAREST extraction (PIL's 16.16 fixed point) on a frame of 32768 pixels or more per side
constexpr int kListFixedLimit = 32768;
inline std::string list_rotated_refusal(int f, int w, int h) {
    char msg[256];
    if (w < kListFixedLimit && h < kListFixedLimit) return "";
    snprintf(msg, sizeof msg, "frame %d of the list: rotated NEAREST windows need a frame smaller than %d pixels per side, this one is read as %d x %d", f,
             kListFixedLimit, w, h);
    return msg;
}

// Everything a list is refused for that needs no device: "" and the layout, or the reason (naming the frame) and an untouched layout.
// bpp: bytes per pixel of the cascade's frame format.  rotated_nearest: a stage behind the first (or the eye step) cuts rotated NEAREST
// windows from the frames the grids are laid over, so those must stay inside the fixed-point range — refused here, before any launch,
// not by the patcher in the middle of the stage loop.
inline std::string list_layout(const hg_cascade_frame* frames, int n_frames, int bpp, ListLayout* out, bool rotated_nearest = false) {
    char msg[256];
    if (!frames) return "null frame list";
    if (n_frames < 1 || n_frames > HG_MAX_STACK_FRAMES) {
        snprintf(msg, sizeof msg, "%d frames in a list (1..%d)", n_frames, HG_MAX_STACK_FRAMES);
        return msg;
    }
    ListLayout L;
    L.first.assign((size_t)n_frames + 1, 0);
    L.grid.assign((size_t)n_frames, 0);
    L.tab_row.assign((size_t)n_frames, 0);
    L.gw.assign((size_t)n_frames, 0);
    L.gh.assign((size_t)n_frames, 0);
    int64_t total = 0;
    for (int f = 0; f < n_frames; ++f) {
        const hg_cascade_frame& F = frames[f];
        const std::string bad = list_frame_refusal(f, F.frame_dev, F.frame_h, F.frame_w, F.ld, bpp);
        if (!bad.empty()) return bad;
        if ((F.prescale_w > 0 || F.prescale_h > 0) && (F.prescale_w <= 0 || F.prescale_h <= 0)) {
            snprintf(msg, sizeof msg, "frame %d of the list: bad prescale size %d x %d", f, F.prescale_w, F.prescale_h);
            return msg;
        }
        if (!F.levels || F.n_levels < 1 || F.n_levels > kListMaxLevels) {
            snprintf(msg, sizeof msg, "frame %d of the list: 1..%d pyramid levels", f, kListMaxLevels);
            return msg;
        }
        int64_t n0 = 0;
        for (int v = 0; v < F.n_levels; ++v) {
            const hg_cascade_level& lv = F.levels[v];
            if (lv.nx < 1 || lv.ny < 1 || (int64_t)lv.nx * lv.ny > kListMaxWindows) {
                snprintf(msg, sizeof msg, "frame %d of the list: level %d: bad grid %d x %d", f, v, lv.nx, lv.ny);
                return msg;
            }
            n0 += (int64_t)lv.nx * lv.ny;
            if (n0 > kListMaxWindows) break;
        }
        total += n0;
        if (total > kListMaxWindows) {
            snprintf(msg, sizeof msg, "too many windows: frames 0..%d of the list hold more than %lld", f, (long long)kListMaxWindows);
            return msg;
        }
        L.first[(size_t)f + 1] = (int32_t)total;
        L.gw[(size_t)f] = F.prescale_w > 0 ? F.prescale_w : F.frame_w;
        L.gh[(size_t)f] = F.prescale_w > 0 ? F.prescale_h : F.frame_h;
        if (rotated_nearest) {
            const std::string rot = list_rotated_refusal(f, L.gw[(size_t)f], L.gh[(size_t)f]);
            if (!rot.empty()) return rot;
        }
    }
    // distinct grids: the same size under the grid and the same level table, bytes for bytes (hg_cascade_level has no padding)
    uint64_t key = 1469598103934665603ull;
    for (int f = 0; f < n_frames; ++f) {
        const hg_cascade_frame& F = frames[f];
        int g = -1;
        for (size_t k = 0; k < L.grid_frame.size() && g < 0; ++k) {
            const int o = L.grid_frame[k];
            const hg_cascade_frame& O = frames[o];
            if (L.gw[(size_t)o] == L.gw[(size_t)f] && L.gh[(size_t)o] == L.gh[(size_t)f] && O.n_levels == F.n_levels &&
                memcmp(O.levels, F.levels, (size_t)F.n_levels * sizeof(hg_cascade_level)) == 0)
                g = (int)k;
        }
        if (g < 0) {
            g = (int)L.grid_frame.size();
            L.grid_frame.push_back(f);
            L.tab_row[(size_t)f] = (int32_t)L.tab_rows;
            L.tab_rows += L.first[(size_t)f + 1] - L.first[(size_t)f];
            key = list_fnv(F.levels, (size_t)F.n_levels * sizeof(hg_cascade_level), key);
        } else {
            L.tab_row[(size_t)f] = L.tab_row[(size_t)L.grid_frame[(size_t)g]];
        }
        L.grid[(size_t)f] = g;
        // (the frame's OWN size too: what is kept under the key includes the whole-frame box of its prescale)
        const int32_t rec[5] = {F.frame_w, F.frame_h, L.gw[(size_t)f], L.gh[(size_t)f], g};
        key = list_fnv(rec, sizeof rec, key);
    }
    L.key = key ? key : 1;
    *out = std::move(L);
    return "";
}

// The survivors of a pooled pass, as the caller gets them: orig_index[i] (ascending by frame: the compaction keeps the candidates'
// order) becomes the index within its frame's own grid, and frame_first (n_frames + 1) the first survivor of every frame.  first[f]
// (n_frames entries): frame f's first original window — f * n0 for a stack, ListLayout::first for a list.
inline void split_by_first(int32_t* orig_index, int64_t n, const int32_t* first, int n_frames, int32_t* frame_first) {
    int f = 0;
    frame_first[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        while (f + 1 < n_frames && orig_index[i] >= first[f + 1]) frame_first[++f] = (int32_t)i;
        orig_index[i] -= first[f];
    }
    while (f < n_frames) frame_first[++f] = (int32_t)n;
}

// The segment words a pooled eye tail brings back from the device, seg = first[n_frames + 1] then kept[n_frames]: frame f assembled
// rows [first[f], first[f + 1]) of n and kept kept[f] of them, at most one more than it had (the purge may append its first row a
// second time).  "" and the number of kept rows of all frames, or what is wrong with them.
inline std::string tail_segments_refusal(const int32_t* seg, int n_frames, int64_t n, int64_t* kept) {
    *kept = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int64_t lo = seg[f], nb = seg[f + 1] - lo, kf = seg[n_frames + 1 + f];
        if (lo < 0 || nb < 0 || lo + nb > n || kf < 0 || kf > nb + 1) {
            char msg[96];
            snprintf(msg, sizeof msg, "frame %d: bad row bounds from the device", f);
            return msg;
        }
        *kept += kf;
    }
    return "";
}
// ... and the caller's layout of checked segments: frame f's kept rows, which start at row first[f] + f of `purged`, packed from
// out_rows[frame_first[f]] on; n_before_purge (nullable): its assembled rows.
inline void tail_place(const int32_t* seg, const double* purged, int n_frames, double* out_rows, int32_t* frame_first, int32_t* n_before_purge) {
    int64_t at = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int64_t lo = seg[f], kf = seg[n_frames + 1 + f];
        frame_first[f] = (int32_t)at;
        if (n_before_purge) n_before_purge[f] = (int32_t)(seg[f + 1] - lo);
        if (kf) memcpy(out_rows + at * 10, purged + (size_t)(lo + f) * 10, (size_t)kf * 80);
        at += kf;
    }
    frame_first[n_frames] = (int32_t)at;
}

}  // namespace hg
