// Stand-alone driver of csrc/hg_resample.cpp for sanitizer builds (tests/test_resample_host.py builds it with
// -fsanitize=address,undefined and runs it as a program; it is never loaded into Python).  Every buffer is a heap block of exactly the
// bytes the call may touch, so a read or a write past a row's end is an AddressSanitizer report; the checks it makes itself: a constant
// image stays constant under every filter, guard bytes between pitched rows survive, the refusals refuse.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pyfaceanalysis_amd/csrc/hg_resample.hpp"

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

int bpp_of(int format) { return format == HG_FRAME_L ? 1 : (format == HG_FRAME_RGB || format == HG_FRAME_BGR) ? 3 : 4; }

uint32_t g_seed = 12345u;
uint8_t next_byte() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (uint8_t)(g_seed >> 24);
}

// one call on exact-size heap buffers; pad: bytes between two rows (source and destination), filled with 0xA5 in the destination
void run(int filter, int format, int out_format, int w, int h, int ow, int oh, int pad, int constant) {
    const int bpp = bpp_of(format), obpp = bpp_of(out_format);
    const int64_t ld = (int64_t)w * bpp + pad, dld = (int64_t)ow * obpp + pad;
    const size_t src_bytes = (size_t)((h - 1) * ld + (int64_t)w * bpp), dst_bytes = (size_t)((oh - 1) * dld + (int64_t)ow * obpp);
    uint8_t* src = (uint8_t*)std::malloc(src_bytes);
    uint8_t* dst = (uint8_t*)std::malloc(dst_bytes);
    for (size_t i = 0; i < src_bytes; ++i) src[i] = constant >= 0 ? (uint8_t)constant : next_byte();
    std::memset(dst, 0xA5, dst_bytes);
    const char* why = hg::frame_resize_host(filter, src, format, h, w, ld, out_format, dst, oh, ow, dld);
    CHECK(!why, "filter %d format %d->%d %dx%d -> %dx%d: %s", filter, format, out_format, w, h, ow, oh, why ? why : "");
    for (int y = 0; y < oh && !why; ++y) {
        for (int64_t x = 0; x < (int64_t)ow * obpp; ++x)
            if (constant >= 0) CHECK(dst[y * dld + x] == constant, "filter %d format %d->%d %dx%d -> %dx%d: constant %d became %d", filter, format, out_format, w, h, ow, oh, constant, dst[y * dld + x]);
        for (int64_t x = (int64_t)ow * obpp; x < dld && y + 1 < oh; ++x) CHECK(dst[y * dld + x] == 0xA5, "guard byte changed (row %d)", y);
    }
    std::free(src);
    std::free(dst);
}

}  // namespace

int main() {
    const int shapes[][4] = {{37, 23, 16, 9}, {64, 48, 33, 48}, {50, 40, 50, 17}, {19, 31, 40, 50}, {200, 113, 104, 58}, {129, 7, 3, 5},
                             {5, 5, 1, 1},   {300, 2, 77, 2},   {480, 270, 250, 140}, {130, 70, 65, 17}, {5, 9, 3, 4},    {300, 40, 7, 40},
                             {8, 3000, 4, 100}};
    const int filters[] = {HG_RESAMPLE_BOX, HG_RESAMPLE_BILINEAR, HG_RESAMPLE_HAMMING, HG_RESAMPLE_BICUBIC, HG_RESAMPLE_LANCZOS};
    int calls = 0;
    for (const auto& s : shapes)
        for (int f : filters)
            for (int format = HG_FRAME_L; format <= HG_FRAME_BGRA; ++format)
                for (int colour_out = 0; colour_out < (format == HG_FRAME_L ? 1 : 2); ++colour_out) {
                    const int pad = (calls % 3 == 0) ? 0 : (calls % 3 == 1) ? 1 : 5;
                    // a grey constant survives convert("L") only for grey sources: constants are checked on HG_FRAME_L and colour output
                    const int constant = (format == HG_FRAME_L || colour_out) ? (calls % 2 ? 255 : 37) : -1;
                    run(f, format, colour_out ? format : HG_FRAME_L, s[0], s[1], s[2], s[3], pad, (calls & 4) ? -1 : constant);
                    ++calls;
                }
    for (int format = HG_FRAME_L; format <= HG_FRAME_BGRA; ++format) run(HG_RESAMPLE_NEAREST, format, HG_FRAME_L, 37, 23, 16, 9, 3, -1), ++calls;
    // extreme shrink and stretch along one axis: 18001 taps for one output pixel; one source pixel under every output pixel
    run(HG_RESAMPLE_LANCZOS, HG_FRAME_L, HG_FRAME_L, 3000, 1, 1, 1, 0, 200), ++calls;
    run(HG_RESAMPLE_LANCZOS, HG_FRAME_L, HG_FRAME_L, 3000, 2, 1, 5, 0, -1), ++calls;
    run(HG_RESAMPLE_BICUBIC, HG_FRAME_RGB, HG_FRAME_RGB, 1, 1, 3000, 2, 1, 99), ++calls;
    run(HG_RESAMPLE_HAMMING, HG_FRAME_BGRA, HG_FRAME_L, 2, 3000, 2, 1, 1, -1), ++calls;

    // the tables alone: every row's count inside the axis, coefficients past the count zero, sums near 2^22
    for (const auto& s : shapes)
        for (int f : filters) {
            hg::ResampleAxis ax;
            const char* why = hg::resample_axis(s[0], s[2], f, ax);
            CHECK(!why, "tables %d -> %d filter %d: %s", s[0], s[2], f, why ? why : "");
            for (int xx = 0; xx < ax.out && !why; ++xx) {
                const int xmin = ax.bounds[(size_t)xx * 2], xmax = ax.bounds[(size_t)xx * 2 + 1];
                CHECK(xmin >= 0 && xmax >= 1 && xmin + xmax <= ax.in && xmax <= ax.ksize, "tables %d -> %d filter %d: row %d reads [%d, %d)", s[0], s[2], f, xx, xmin, xmin + xmax);
                int64_t sum = 0;
                for (int x = 0; x < ax.ksize; ++x) {
                    sum += ax.k[(size_t)xx * ax.ksize + x];
                    if (x >= xmax) CHECK(ax.k[(size_t)xx * ax.ksize + x] == 0, "tables: a coefficient past the row's count");
                }
                CHECK(sum > (1 << 22) - ax.ksize && sum < (1 << 22) + ax.ksize, "tables %d -> %d filter %d: row %d sums to %lld", s[0], s[2], f, xx, (long long)sum);
            }
        }

    // refusals: each with a message, nothing written
    uint8_t a[64] = {0}, b[64];
    std::memset(b, 7, sizeof b);
    hg::ResampleAxis ax;
    CHECK(hg::resample_axis(0, 4, HG_RESAMPLE_BOX, ax) != nullptr, "in = 0 accepted");
    CHECK(hg::resample_axis(4, -1, HG_RESAMPLE_BOX, ax) != nullptr, "out < 0 accepted");
    CHECK(hg::resample_axis(4, 2, HG_RESAMPLE_NEAREST, ax) != nullptr, "NEAREST has no tables");
    CHECK(hg::resample_axis(4, 2, 6, ax) != nullptr, "filter 6 accepted");
    CHECK(hg::resample_axis(2000000000, 1, HG_RESAMPLE_LANCZOS, ax) != nullptr, "tables beyond the cap accepted");
    CHECK(hg::resample_axis(3, 1 << 23, HG_RESAMPLE_BOX, ax) != nullptr, "tables beyond the cap accepted");
    CHECK(hg::frame_resize_host(2, a, HG_FRAME_L, 4, 4, 3, HG_FRAME_L, b, 2, 2, 2) != nullptr, "ld < w accepted");
    CHECK(hg::frame_resize_host(2, a, HG_FRAME_RGB, 2, 2, 6, HG_FRAME_BGR, b, 2, 2, 6) != nullptr, "foreign out_format accepted");
    CHECK(hg::frame_resize_host(0, a, HG_FRAME_RGB, 2, 2, 6, HG_FRAME_RGB, b, 2, 2, 6) != nullptr, "NEAREST colour output accepted");
    CHECK(hg::frame_resize_host(2, nullptr, HG_FRAME_L, 4, 4, 4, HG_FRAME_L, b, 2, 2, 2) != nullptr, "null source accepted");
    CHECK(hg::frame_resize_host(2, a, HG_FRAME_L, 4, 4, 4, HG_FRAME_L, a + 8, 2, 2, 2) != nullptr, "overlap accepted");
    for (size_t i = 0; i < sizeof b; ++i) CHECK(b[i] == 7, "a refused call wrote");

    std::printf("resample_driver: %s (%d calls, %d failed checks)\n", g_bad ? "FAILED" : "ok", calls, g_bad);
    return g_bad ? 1 : 0;
}
