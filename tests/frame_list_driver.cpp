// Stand-alone driver of the host-only part of the frame-list pass (pyfaceanalysis_amd/csrc/hg_frame_list.hpp): seeded lists of frames
// through hg::list_layout, every invariant of the layout checked, and every refusal with the bad frame first, in the middle and last.
// Built with -fsanitize=address,undefined by tests/test_frame_list_sanitizers.py; prints "ok <lists> <refusals>" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "hg_frame_list.hpp"

static int fails = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAILED line %d: %s\n", __LINE__, #c);        \
            ++fails;                                             \
        }                                                        \
    } while (0)

int main() {
    std::mt19937 rng(20240611u);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    // a pool of level tables: some equal in content at different addresses (equal grids are found by content, not by pointer)
    std::vector<std::vector<hg_cascade_level>> pool;
    for (int t = 0; t < 12; ++t) {
        std::vector<hg_cascade_level> lv((size_t)rnd(1, 32));
        for (auto& v : lv) {
            v = hg_cascade_level{};
            v.nx = rnd(1, 40);
            v.ny = rnd(1, 30);
            v.patch_w = v.patch_h = 64.0 * (1 + (int)(&v - lv.data()));
        }
        pool.push_back(lv);
        if (t % 3 == 0) pool.push_back(lv);      // a copy
    }
    static unsigned char pixels[16];
    int lists = 0, refusals = 0;
    for (int it = 0; it < 400; ++it) {
        const int n = it < 4 ? (it == 0 ? 1 : it == 1 ? HG_MAX_STACK_FRAMES : rnd(2, 5)) : rnd(1, 40);
        std::vector<hg_cascade_frame> fr((size_t)n);
        const int sizes[4][2] = {{97, 131}, {320, 240}, {1000, 562}, {7, 5}};
        for (auto& f : fr) {
            const int s = rnd(0, 3), t = rnd(0, (int)pool.size() - 1);
            f = hg_cascade_frame{};
            f.frame_dev = pixels;
            f.frame_w = sizes[s][0];
            f.frame_h = sizes[s][1];
            f.ld = f.frame_w + rnd(0, 9);
            if (rnd(0, 2) == 0) {
                f.prescale_w = 50 + 10 * rnd(0, 2);
                f.prescale_h = 40;
            }
            f.levels = pool[(size_t)t].data();
            f.n_levels = (int)pool[(size_t)t].size();
        }
        hg::ListLayout L, L2;
        const std::string why = hg::list_layout(fr.data(), n, 1, &L);
        CHECK(why.empty());
        if (!why.empty()) continue;
        ++lists;
        CHECK(hg::list_layout(fr.data(), n, 1, &L2).empty() && L2.key == L.key && L.key != 0);
        CHECK((int)L.first.size() == n + 1 && L.first[0] == 0 && (int)L.grid.size() == n && (int)L.tab_row.size() == n);
        int64_t rows = 0;
        for (size_t g = 0; g < L.grid_frame.size(); ++g) {
            const int f = L.grid_frame[g];
            CHECK(L.grid[(size_t)f] == (int)g && L.tab_row[(size_t)f] == rows);
            rows += L.first[(size_t)f + 1] - L.first[(size_t)f];
        }
        CHECK(rows == L.tab_rows && L.tab_rows <= L.first[(size_t)n]);
        for (int f = 0; f < n; ++f) {
            int64_t n0 = 0;
            for (int v = 0; v < fr[(size_t)f].n_levels; ++v) n0 += (int64_t)fr[(size_t)f].levels[v].nx * fr[(size_t)f].levels[v].ny;
            CHECK(L.first[(size_t)f + 1] - L.first[(size_t)f] == n0 && n0 >= 1);
            const int o = L.grid_frame[(size_t)L.grid[(size_t)f]];
            CHECK(o <= f && L.tab_row[(size_t)f] == L.tab_row[(size_t)o] && L.gw[(size_t)o] == L.gw[(size_t)f] && L.gh[(size_t)o] == L.gh[(size_t)f]);
            CHECK(fr[(size_t)o].n_levels == fr[(size_t)f].n_levels &&
                  memcmp(fr[(size_t)o].levels, fr[(size_t)f].levels, (size_t)fr[(size_t)f].n_levels * sizeof(hg_cascade_level)) == 0);
            CHECK(L.tab_row[(size_t)f] + n0 <= L.tab_rows);
            for (int e = 0; e < f; ++e)      // two frames share table rows exactly when their grids are equal
                CHECK((L.grid[(size_t)e] == L.grid[(size_t)f]) == (L.tab_row[(size_t)e] == L.tab_row[(size_t)f]));
            CHECK(L.gw[(size_t)f] == (fr[(size_t)f].prescale_w > 0 ? fr[(size_t)f].prescale_w : fr[(size_t)f].frame_w));
        }
        if (n < 3 || it % 4) continue;
        // refusals: the bad frame first, in the middle, last; the layout handed in stays untouched
        hg_cascade_level huge{};
        huge.nx = 1 << 12;
        huge.ny = 1 << 13;
        hg_cascade_level zero{};
        const int at[3] = {0, n / 2, n - 1};
        for (int a = 0; a < 3; ++a)
            for (int kind = 0; kind < 9; ++kind) {
                std::vector<hg_cascade_frame> bad = fr;
                hg_cascade_frame& b = bad[(size_t)at[a]];
                switch (kind) {
                    case 0: b.frame_h = 0; break;
                    case 1: b.frame_w = -1; break;
                    case 2: b.ld = b.frame_w - 1; break;
                    case 3: b.frame_dev = nullptr; break;
                    case 4: b.levels = nullptr; break;
                    case 5: b.n_levels = rnd(0, 1) ? 0 : 33; break;
                    case 6: b.prescale_w = 50; b.prescale_h = 0; break;
                    case 7: b.levels = &huge; b.n_levels = 1; break;
                    default: b.levels = &zero; b.n_levels = 1; break;
                }
                hg::ListLayout K;
                K.tab_rows = -7;
                const std::string w = hg::list_layout(bad.data(), n, 1, &K);
                char name[32];
                snprintf(name, sizeof name, "frame %d ", at[a]);
                CHECK(!w.empty() && w.find(name) != std::string::npos && K.tab_rows == -7 && K.first.empty());
                ++refusals;
            }
    }
    hg::ListLayout K;
    CHECK(!hg::list_layout(nullptr, 3, 1, &K).empty());
    hg_cascade_frame one{};
    CHECK(!hg::list_layout(&one, 0, 1, &K).empty() && !hg::list_layout(&one, HG_MAX_STACK_FRAMES + 1, 1, &K).empty());
    // the total above the bound (2^31 / 64 = 2^25 - 1) although no frame is: 2^24 windows twice
    hg_cascade_level big{};
    big.nx = big.ny = 1 << 12;
    std::vector<hg_cascade_frame> three(3);
    for (auto& f : three) {
        f = hg_cascade_frame{};
        f.frame_dev = pixels;
        f.frame_w = f.frame_h = 4;
        f.ld = 4;
        f.levels = &big;
        f.n_levels = 1;
    }
    CHECK(hg::list_layout(three.data(), 1, 1, &K).empty() && K.first[1] == (1 << 24) && K.tab_rows == (1 << 24));
    CHECK(hg::list_layout(three.data(), 2, 1, &K).find("too many windows") != std::string::npos);
    CHECK(hg::list_layout(three.data(), 3, 1, &K).find("too many windows") != std::string::npos);
    // bytes per pixel: ld is in bytes
    CHECK(hg::list_layout(three.data(), 2, 3, &K).find("frame 0 ") != std::string::npos);
    // two lists of one frame that share the prescaled size and the level table but not the frame's own size (1280 x 720 and 1920 x 1080
    // behind a prescale to 1000 x 562): what is kept under the key holds the whole-frame box, so the keys differ; the same list: the same key
    hg_cascade_level lv{};
    lv.nx = 7;
    lv.ny = 5;
    hg_cascade_frame a{}, b{};
    a.frame_dev = b.frame_dev = pixels;
    a.frame_w = a.ld = 1280;
    a.frame_h = 720;
    b.frame_w = b.ld = 1920;
    b.frame_h = 1080;
    a.prescale_w = b.prescale_w = 1000;
    a.prescale_h = b.prescale_h = 562;
    a.levels = b.levels = &lv;
    a.n_levels = b.n_levels = 1;
    hg::ListLayout Ka, Kb, Ka2;
    CHECK(hg::list_layout(&a, 1, 1, &Ka).empty() && hg::list_layout(&b, 1, 1, &Kb).empty() && hg::list_layout(&a, 1, 1, &Ka2).empty());
    CHECK(Ka.key != Kb.key && Ka.key == Ka2.key && Ka.gw == Kb.gw && Ka.gh == Kb.gh && Ka.tab_rows == Kb.tab_rows);
    // a frame outside PIL's fixed-point range: refused only where rotated NEAREST windows are cut from it, by the size the grid is laid over
    for (int at = 0; at < 3; ++at) {
        hg_cascade_frame w3[3] = {a, a, a};
        w3[at].frame_w = w3[at].ld = 40000;
        w3[at].prescale_w = w3[at].prescale_h = 0;
        CHECK(hg::list_layout(w3, 3, 1, &K, false).empty());
        char name[32];
        snprintf(name, sizeof name, "frame %d ", at);
        CHECK(hg::list_layout(w3, 3, 1, &K, true).find(name) != std::string::npos);
        w3[at].prescale_w = 1000;
        w3[at].prescale_h = 18;
        CHECK(hg::list_layout(w3, 3, 1, &K, true).empty());
    }
    if (fails) return 1;
    printf("ok %d %d\n", lists, refusals);
    return 0;
}
