// Stand-alone driver of the host-only argument check of the frame-LIST normalise / estimate entries (hg::normalize_frame_list_check,
// hg::normalize_list_check; pyfaceanalysis_amd/csrc/hg_normalize.cpp + hg_frame_list.hpp): the refusals — a null list, n_frames 0 and
// HG_MAX_STACK_FRAMES + 1, a bad frame first, in the middle and last (null pointer, frame_h 0, ld < frame_w), a null face_frame with
// n > 0, a bad output size, ldo below out_w * out_h, a geom built for another frame's size — and good lists, among them faces whose frame
// index lies outside the list.  Built by tests/test_estimate_frame_list_host.py, plain and with -fsanitize=address,undefined: the frame
// "pixels" are a one-byte allocation, so a check that read behind a frame pointer would be reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hg_normalize.hpp"

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, what)                                       \
    do {                                                        \
        ++g_checks;                                             \
        if (!(cond)) {                                          \
            std::printf("FAILED: %s (line %d)\n", what, __LINE__); \
            ++g_bad;                                            \
        }                                                       \
    } while (0)

namespace {

constexpr int kOutW = 17, kOutH = 13;
const int kSizes[3][3] = {{7, 5, 9}, {97, 131, 144}, {40, 61, 40}};      // frame_w, frame_h, ld

struct Case {
    std::unique_ptr<uint8_t[]> pixel{new uint8_t[1]};      // one byte: nothing behind a frame pointer may be read
    std::vector<hg_frame_ref> frames;
    std::vector<hg_norm_geom> geoms;
    std::vector<int32_t> ff;
    uint8_t out_byte = 0;
};

// faces interleaved over the three frames, each geom made for its own frame's size
Case good_case(int faces_per_frame) {
    Case c;
    for (auto& s : kSizes) c.frames.push_back(hg_frame_ref{c.pixel.get(), s[1], s[0], s[2]});
    hg_norm_consts k{};
    k.out_w = kOutW; k.out_h = kOutH; k.method = HG_NORM_AREAZ; k.rotate = 1;
    for (int j = 0; j < faces_per_frame; ++j)
        for (int f = 2; f >= 0; --f) {
            const double w = kSizes[f][0], h = kSizes[f][1];
            const double eyes[4] = {0.3 * w + j, 0.4 * h - j, 0.6 * w + 2 * j, 0.45 * h + j};
            hg_norm_geom g;
            const char* why = hg::normalize_geometry_host(eyes, 1, kSizes[f][0], kSizes[f][1], &k, &g);
            CHECK(why == nullptr && g.status == 0, "geometry of a good face");
            c.geoms.push_back(g);
            c.ff.push_back(f);
        }
    return c;
}

std::string full(const Case& c, const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms, const int32_t* ff, int64_t n, int ow = kOutW, int oh = kOutH,
                 const void* out = (const void*)1, int64_t ldo = kOutW * kOutH) {
    return hg::normalize_frame_list_check(frames, n_frames, geoms, ff, n, ow, oh, out == (const void*)1 ? &c.out_byte : out, ldo);
}

// both checks refuse, and name the frame where `frame` >= 0
void refused(const Case& c, const hg_frame_ref* frames, int n_frames, const int32_t* ff, int64_t n, int frame, const char* what) {
    const std::string a = full(c, frames, n_frames, c.geoms.data(), ff, n);
    const std::string b = hg::normalize_list_check(frames, n_frames, c.geoms.data(), ff, n);
    CHECK(!a.empty() && !b.empty(), what);
    if (frame >= 0) {
        const std::string name = "frame " + std::to_string(frame) + " ";
        CHECK(a.find(name) != std::string::npos && b.find(name) != std::string::npos, what);
    }
}

}  // namespace

int main() {
    Case c = good_case(4);
    const int64_t n = (int64_t)c.geoms.size();
    const hg_frame_ref* fr = c.frames.data();
    const int32_t* ff = c.ff.data();

    // good lists
    CHECK(full(c, fr, 3, c.geoms.data(), ff, n).empty(), "a good list was refused");
    CHECK(hg::normalize_list_check(fr, 3, c.geoms.data(), ff, n).empty(), "a good list was refused (faces alone)");
    CHECK(full(c, fr, 3, nullptr, nullptr, 0, kOutW, kOutH, nullptr).empty(), "n == 0 needs no data pointer");
    {
        std::vector<hg_frame_ref> many((size_t)HG_MAX_STACK_FRAMES, c.frames[1]);
        CHECK(full(c, many.data(), HG_MAX_STACK_FRAMES, nullptr, nullptr, 0).empty(), "the largest list was refused");
        many.push_back(c.frames[1]);
        CHECK(!full(c, many.data(), HG_MAX_STACK_FRAMES + 1, nullptr, nullptr, 0).empty(), "HG_MAX_STACK_FRAMES + 1 frames accepted");
        CHECK(!hg::normalize_list_check(many.data(), HG_MAX_STACK_FRAMES + 1, nullptr, nullptr, 0).empty(), "HG_MAX_STACK_FRAMES + 1 frames accepted (faces alone)");
    }
    {   // indices outside the list: no error, and their geoms are not looked at (one is garbage)
        Case d = good_case(2);
        d.ff[1] = -1; d.ff[2] = 3; d.ff[4] = 8;
        std::memset(&d.geoms[2], 0x7f, sizeof(hg_norm_geom));
        CHECK(full(d, d.frames.data(), 3, d.geoms.data(), d.ff.data(), (int64_t)d.geoms.size()).empty(), "a frame index outside the list is no error");
        CHECK(hg::normalize_list_check(d.frames.data(), 3, d.geoms.data(), d.ff.data(), (int64_t)d.geoms.size()).empty(), "a frame index outside the list is no error (faces alone)");
    }
    {   // a list of one frame, a one-row frame whose ld is its width
        hg_frame_ref one{c.pixel.get(), 1, 7, 7};
        CHECK(full(c, &one, 1, nullptr, nullptr, 0).empty(), "a one-row frame was refused");
    }

    // the list itself
    refused(c, nullptr, 3, ff, n, -1, "a null list accepted");
    refused(c, fr, 0, ff, n, -1, "n_frames 0 accepted");
    refused(c, fr, -1, ff, n, -1, "n_frames -1 accepted");
    refused(c, fr, 3, ff, -1, -1, "n < 0 accepted");
    refused(c, fr, 3, nullptr, n, -1, "a null face_frame with n > 0 accepted");
    CHECK(!full(c, fr, 3, nullptr, ff, n).empty() && !hg::normalize_list_check(fr, 3, nullptr, ff, n).empty(), "null geoms with n > 0 accepted");

    // a bad frame first, in the middle and last; the refusal comes before n == 0
    for (int at = 0; at < 3; ++at) {
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<hg_frame_ref> bad = c.frames;
            if (kind == 0) bad[(size_t)at].frame_dev = nullptr;
            if (kind == 1) bad[(size_t)at].frame_h = 0;
            if (kind == 2) bad[(size_t)at].ld = bad[(size_t)at].frame_w - 1;
            if (kind == 3) bad[(size_t)at].frame_w = -3;
            if (kind == 4) { bad[(size_t)at].frame_w = (1 << 24) + 1; bad[(size_t)at].ld = (1 << 24) + 1; }
            refused(c, bad.data(), 3, ff, n, at, "a bad frame accepted");
            refused(c, bad.data(), 3, ff, 0, at, "a bad frame accepted at n == 0");
        }
    }

    // the output
    CHECK(!full(c, fr, 3, c.geoms.data(), ff, n, 0, kOutH).empty(), "out_w 0 accepted");
    CHECK(!full(c, fr, 3, c.geoms.data(), ff, n, kOutW, 4097).empty(), "out_h 4097 accepted");
    CHECK(!full(c, fr, 3, c.geoms.data(), ff, n, kOutW, kOutH, (const void*)1, kOutW * kOutH - 1).empty(), "ldo below out_w * out_h accepted");
    CHECK(full(c, fr, 3, c.geoms.data(), ff, n, kOutW, kOutH, (const void*)1, kOutW * kOutH + 5).empty(), "ldo above out_w * out_h refused");
    CHECK(!full(c, fr, 3, c.geoms.data(), ff, n, kOutW, kOutH, nullptr).empty(), "a null out with n > 0 accepted");

    // geoms against each face's OWN frame: every face moved to the next frame is refused, whichever face it is
    for (int64_t i = 0; i < n; ++i) {
        std::vector<int32_t> moved = c.ff;
        moved[(size_t)i] = (moved[(size_t)i] + 1) % 3;
        const std::string why = full(c, fr, 3, c.geoms.data(), moved.data(), n);
        CHECK(why.find("another frame size") != std::string::npos, "a geom built for another frame's size accepted");
        CHECK(!hg::normalize_list_check(fr, 3, c.geoms.data(), moved.data(), n).empty(), "a geom built for another frame's size accepted (faces alone)");
    }
    {   // an unknown status
        Case d = good_case(1);
        d.geoms[1].status = 9;
        CHECK(!full(d, d.frames.data(), 3, d.geoms.data(), d.ff.data(), 3).empty(), "status 9 accepted");
    }

    std::printf("estimate_frame_list_driver: %s (%d checks, %d failed)\n", g_bad ? "FAILED" : "ok", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
