// Stand-alone driver of csrc/hg_normalize.cpp for sanitizer builds (tests/test_normalize_host.py builds it with
// -fsanitize=address,undefined and runs it as a program; it is never loaded into Python).  Every buffer is a heap block of exactly the
// bytes the call may touch, so a read past a frame row's end or a write past an image is an AddressSanitizer report; the checks it makes
// itself: a face cut from inside a constant frame is that constant, refused faces are zero with their status set, guard bytes between
// pitched rows and between images survive, both paths (staged, tap by tap) run, the refusals refuse.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../pyfaceanalysis_amd/csrc/hg_normalize.hpp"

namespace {

int g_bad = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            ++g_bad;                           \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                 \
        }                                      \
    } while (0)

uint32_t g_seed = 4321u;
uint8_t next_byte() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (uint8_t)(g_seed >> 24);
}

struct Result {
    std::vector<hg_norm_geom> geoms;
    std::vector<uint8_t> out;
    int64_t ldo = 0;
};

// one geometry + faces call on exact-size heap buffers: rows `pad` bytes apart beyond the width, images `gap` bytes apart beyond their size
Result run(int w, int h, int pad, int constant, const std::vector<double>& eyes, int ow, int oh, int method, int rotate, int gap) {
    const int64_t n = (int64_t)eyes.size() / 4, ld = w + pad;
    const size_t frame_bytes = (size_t)((h - 1) * ld + w);
    uint8_t* frame = (uint8_t*)std::malloc(frame_bytes);
    for (size_t i = 0; i < frame_bytes; ++i) frame[i] = constant >= 0 ? (uint8_t)constant : next_byte();
    Result r;
    r.ldo = (int64_t)ow * oh + gap;
    r.geoms.resize((size_t)n);
    const hg_norm_consts c{ow, oh, method, rotate};
    const char* why = hg::normalize_geometry_host(eyes.data(), n, w, h, &c, r.geoms.data());
    CHECK(!why, "geometry %dx%d: %s", w, h, why ? why : "");
    const size_t out_bytes = n ? (size_t)((n - 1) * r.ldo + (int64_t)ow * oh) : 0;
    uint8_t* out = (uint8_t*)std::malloc(out_bytes ? out_bytes : 1);
    std::memset(out, 0xA5, out_bytes);
    why = hg::normalize_faces_host(frame, h, w, ld, r.geoms.data(), n, ow, oh, out, r.ldo);
    CHECK(!why, "faces %dx%d -> %dx%d: %s", w, h, ow, oh, why ? why : "");
    for (int64_t f = 0; f + 1 < n; ++f)
        for (int64_t x = (int64_t)ow * oh; x < r.ldo; ++x) CHECK(out[f * r.ldo + x] == 0xA5, "guard byte after image %lld changed", (long long)f);
    r.out.assign(out, out + out_bytes);
    std::free(frame);
    std::free(out);
    return r;
}

}  // namespace

int main() {
    int calls = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // noise frames, faces everywhere around them, every output size and method, pitched rows and images
    const int frames[][2] = {{97, 61}, {160, 120}, {64, 64}, {65, 65}, {1, 1}, {3, 200}};
    const int sizes[][3] = {{256, 192, HG_NORM_AREA}, {32, 24, HG_NORM_AREA}, {17, 13, HG_NORM_AREAZ}, {1, 1, HG_NORM_AREAZ}};
    for (const auto& fs : frames) {
        const double w = fs[0], h = fs[1];
        const std::vector<double> eyes = {
            w / 2 - w / 10, h / 2, w / 2 + w / 10, h / 2,            // level
            w / 2 - 5, h / 2 - 7, w / 2 + 6, h / 2 + 4,              // tilted
            w / 2, h / 2, w / 2 + 1, h / 2,                          // one pixel apart
            0, 0, w - 1, h - 1,                                      // the frame's corners
            w / 2, h / 2 - 6, w / 2, h / 2 + 6,                      // vertical, +90
            w / 2, h / 2 + 6, w / 2, h / 2 - 6,                      // vertical, -90
            -0.3 * w, h / 2, 1.3 * w, h / 2 - 2,                     // wider than the frame
            -3 * w, -2 * h, -3 * w + 4, -2 * h + 1,                  // far outside
            5, 5, 4, 5,                                              // refused: swapped
            nan, 1, 2, 3,                                            // refused: not finite
            7, 7, 7, 7,                                              // refused: coincide
            -1e9, -1.135e9, 1e9, -1.135e9 + 3e6,                     // refused: centre out of range
            w / 3, h / 3, w / 3 + 9, h / 3 + 2,
        };
        for (const auto& s : sizes)
            for (int rotate = 0; rotate < 2; ++rotate) {
                const Result r = run(fs[0], fs[1], calls % 3 == 0 ? 0 : calls % 3 == 1 ? 1 : 7, -1, eyes, s[0], s[1], s[2], rotate, calls % 2 ? 0 : 11);
                ++calls;
                const int want[] = {HG_NORM_EYES_SWAPPED, HG_NORM_NOT_FINITE, HG_NORM_ZERO_DISTANCE, HG_NORM_CENTRE_RANGE};
                for (int k = 0; k < 4; ++k) {
                    const size_t f = 8 + (size_t)k;
                    CHECK(r.geoms[f].status == want[k], "face %zu: status %d, expected %d", f, r.geoms[f].status, want[k]);
                    for (int64_t x = 0; x < (int64_t)s[0] * s[1]; ++x) CHECK(r.out[f * r.ldo + x] == 0, "refused face %zu is not zero", f);
                }
                CHECK(r.geoms[0].status == 0 && r.geoms[12].status == 0, "a neighbour of the refused faces was refused");
            }
    }
    // a face cut from well inside a constant frame is that constant, rotated or not, staged (pose size) and tap by tap (tiny output)
    for (int rotate = 0; rotate < 2; ++rotate) {
        const Result a = run(200, 200, 3, 37, {90, 95, 110, 97}, 256, 192, HG_NORM_AREA, rotate, 0);
        for (uint8_t v : a.out) CHECK(v == 37, "constant 37 became %d (staged)", v);
        const Result b = run(200, 200, 0, 201, {15, 60, 185, 62}, 5, 4, HG_NORM_AREA, rotate, 0);      // a 23 x 18 box around (100, 157) cut into 5 x 4
        CHECK((int64_t)b.geoms[0].rect[2] * b.geoms[0].rect[3] > hg::normalize_stage_limit(5, 4), "the tiny output was expected to go tap by tap");
        for (uint8_t v : b.out) CHECK(v == 201, "constant 201 became %d (tap by tap)", v);
        calls += 2;
    }
    run(16, 16, 0, -1, {}, 8, 8, HG_NORM_AREA, 1, 0), ++calls;      // n == 0

    // refusals: each with a message, nothing written
    uint8_t frame[256] = {0}, out[64];
    std::memset(out, 7, sizeof out);
    const double eyes[4] = {2, 3, 5, 3};
    hg_norm_geom g;
    hg_norm_consts c{4, 4, HG_NORM_AREA, 1};
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, &c, &g) == nullptr, "a good geometry call was refused");
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, nullptr, &g) != nullptr, "null consts accepted");
    CHECK(hg::normalize_geometry_host(nullptr, 1, 8, 8, &c, &g) != nullptr, "null eyes accepted");
    CHECK(hg::normalize_geometry_host(eyes, -1, 8, 8, &c, &g) != nullptr, "n < 0 accepted");
    CHECK(hg::normalize_geometry_host(eyes, 1, 0, 8, &c, &g) != nullptr, "frame_w = 0 accepted");
    hg_norm_consts bad = c;
    bad.out_w = 0;
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, &bad, &g) != nullptr, "out_w = 0 accepted");
    bad = c;
    bad.out_h = 4097;
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, &bad, &g) != nullptr, "out_h = 4097 accepted");
    bad = c;
    bad.method = 2;
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, &bad, &g) != nullptr, "method 2 accepted");
    bad = c;
    bad.rotate = 2;
    CHECK(hg::normalize_geometry_host(eyes, 1, 8, 8, &bad, &g) != nullptr, "rotate 2 accepted");
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g, 1, 4, 4, out, 16) == nullptr, "a good faces call was refused");
    std::memset(out, 7, sizeof out);
    CHECK(hg::normalize_faces_host(frame, 8, 8, 7, &g, 1, 4, 4, out, 16) != nullptr, "ld < frame_w accepted");
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g, 1, 4, 4, out, 15) != nullptr, "ldo < out_w * out_h accepted");
    CHECK(hg::normalize_faces_host(nullptr, 8, 8, 8, &g, 1, 4, 4, out, 16) != nullptr, "null frame accepted");
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, nullptr, 1, 4, 4, out, 16) != nullptr, "null geoms accepted");
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g, 1, 4, 4, nullptr, 16) != nullptr, "null out accepted");
    CHECK(hg::normalize_faces_host(frame, 0, 8, 8, &g, 1, 4, 4, out, 16) != nullptr, "frame_h = 0 accepted");
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g, 1, 0, 4, out, 16) != nullptr, "out_w = 0 accepted");
    // (the crop size follows the farther frame edge from the centre pixel (4, 5): a wider or a taller frame moves it, W = 9 -> 15, H = 11 -> 17)
    CHECK(hg::normalize_faces_host(frame, 8, 12, 12, &g, 1, 4, 4, out, 16) != nullptr, "a geom built for another frame width accepted");
    CHECK(hg::normalize_faces_host(frame, 14, 8, 8, &g, 1, 4, 4, out, 16) != nullptr, "a geom built for another frame height accepted");
    hg_norm_geom g2 = g;
    g2.rect[2] = g2.W + 1;
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g2, 1, 4, 4, out, 16) != nullptr, "a rect wider than the crop accepted");
    g2 = g;
    g2.status = 9;
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g2, 1, 4, 4, out, 16) != nullptr, "status 9 accepted");
    for (size_t i = 0; i < sizeof out; ++i) CHECK(out[i] == 7, "a refused call wrote");
    // a hand-made rect inside the crop but smaller than the taps need: clamped reads, no report
    g2 = g;
    if (g2.rect[2] > 1) g2.rect[2] = 1, g2.rect[3] = 1;
    CHECK(hg::normalize_faces_host(frame, 8, 8, 8, &g2, 1, 4, 4, out, 16) == nullptr, "a small hand-made rect was refused");

    std::printf("normalize_driver: %s (%d calls, %d failed checks)\n", g_bad ? "FAILED" : "ok", calls, g_bad);
    return g_bad ? 1 : 0;
}
