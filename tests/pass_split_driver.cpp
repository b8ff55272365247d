// Stand-alone driver of what the pooled passes do on the host with their survivors (pyfaceanalysis_amd/csrc/hg_frame_list.hpp):
// hg::split_by_first against restatements of the two functions it replaced, the layout of a pooled eye tail (hg::tail_place) against a
// direct restatement, and hg::tail_segments_refusal on every segment word out of range.  Seeded cases; built plain and with
// -fsanitize=address,undefined by tests/test_pass_split_host.py; prints "ok <cases> <refusals>" and returns 0.
#include <algorithm>
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

// the split of a STACK's survivors as it was: a survivor's frame is its index / n0
static void old_split_by_frame(int32_t* orig_index, int64_t n, int64_t n0, int n_frames, int32_t* frame_first) {
    int f = 0;
    frame_first[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int fi = (int)(orig_index[i] / n0);
        while (f < fi && f < n_frames) frame_first[++f] = (int32_t)i;
        orig_index[i] = (int32_t)(orig_index[i] - (int64_t)fi * n0);
    }
    while (f < n_frames) frame_first[++f] = (int32_t)n;
}

// the split of a LIST's survivors as it was: frame f holds the windows first[f] .. first[f + 1]
static void old_split_by_list(int32_t* orig_index, int64_t n, const std::vector<int32_t>& first, int n_frames, int32_t* frame_first) {
    int f = 0;
    frame_first[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        while (f + 1 < n_frames && orig_index[i] >= first[(size_t)f + 1]) frame_first[++f] = (int32_t)i;
        orig_index[i] -= first[(size_t)f];
    }
    while (f < n_frames) frame_first[++f] = (int32_t)n;
}

int main() {
    std::mt19937 rng(20241020u);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    int cases = 0, refusals = 0;
    for (int it = 0; it < 400; ++it) {
        // ---- the split ----------------------------------------------------------------------------------------------------
        const int nf = it % 10 == 0 ? 1 : rnd(2, 12);
        const bool stack = it % 2 == 0;      // equal grids: first[f] = f * n0, both old functions apply
        const int n0 = rnd(1, 60);
        std::vector<int32_t> first((size_t)nf + 1, 0);
        for (int f = 0; f < nf; ++f) first[(size_t)f + 1] = first[(size_t)f] + (stack ? n0 : rnd(1, 60));
        // which frames have survivors: none at all, none at the front / in the middle / at the end, or at random
        std::vector<int> has((size_t)nf);
        const int mode = it % 8;
        for (int f = 0; f < nf; ++f) {
            has[(size_t)f] = rnd(0, 2) != 0;
            if (mode == 1) has[(size_t)f] = 0;
            if (mode == 2 && f == 0) has[(size_t)f] = 0;
            if (mode == 3 && f == nf / 2) has[(size_t)f] = 0;
            if (mode == 4 && f == nf - 1) has[(size_t)f] = 0;
            if (mode == 5 && (f == 0 || f == nf - 1)) has[(size_t)f] = 0;
        }
        std::vector<int32_t> idx, frame_of;      // ascending original windows, every one inside its frame's windows
        for (int f = 0; f < nf; ++f) {
            if (!has[(size_t)f]) continue;
            const int w = first[(size_t)f + 1] - first[(size_t)f];
            std::vector<int32_t> all((size_t)w);
            for (int j = 0; j < w; ++j) all[(size_t)j] = first[(size_t)f] + j;
            std::shuffle(all.begin(), all.end(), rng);
            all.resize((size_t)rnd(1, w));
            if (rnd(0, 3) == 0) all[0] = first[(size_t)f];                    // the frame's first window
            if (rnd(0, 3) == 0) all.back() = first[(size_t)f + 1] - 1;        // ... and its last
            std::sort(all.begin(), all.end());
            all.erase(std::unique(all.begin(), all.end()), all.end());
            for (int32_t o : all) {
                idx.push_back(o);
                frame_of.push_back(f);
            }
        }
        const int64_t n = (int64_t)idx.size();
        std::vector<int32_t> a = idx, b = idx, fa((size_t)nf + 1, -7), fb((size_t)nf + 1, -7);
        hg::split_by_first(a.data(), n, first.data(), nf, fa.data());
        old_split_by_list(b.data(), n, first, nf, fb.data());
        CHECK(a == b && fa == fb);
        if (stack) {
            std::vector<int32_t> s = idx, fs((size_t)nf + 1, -7);
            old_split_by_frame(s.data(), n, n0, nf, fs.data());
            CHECK(a == s && fa == fs);
        }
        // the properties themselves: frame f's survivors are [fa[f], fa[f + 1]), each index the window within its own frame
        CHECK(fa[0] == 0 && fa[(size_t)nf] == n);
        for (int64_t i = 0; i < n; ++i) {
            const int f = frame_of[(size_t)i];
            CHECK(fa[(size_t)f] <= i && i < fa[(size_t)f + 1] && a[(size_t)i] == idx[(size_t)i] - first[(size_t)f]);
        }
        for (int f = 0; f < nf; ++f) CHECK(fa[(size_t)f] <= fa[(size_t)f + 1]);
        // ---- the layout of a pooled eye tail --------------------------------------------------------------------------------
        // frame f assembled nb[f] rows and kept kf[f] of them: 0, 1, or one more than it had (the first row appended twice)
        std::vector<int32_t> seg((size_t)2 * nf + 1, 0);
        int64_t rows_n = 0, kept = 0;
        for (int f = 0; f < nf; ++f) {
            const int nb = has[(size_t)f] ? rnd(0, 9) : 0, pick = rnd(0, 2);
            seg[(size_t)f] = (int32_t)rows_n;
            rows_n += nb;
            seg[(size_t)nf + 1 + f] = pick == 0 ? 0 : pick == 1 ? 1 : nb + 1;
            kept += seg[(size_t)nf + 1 + f];
        }
        seg[(size_t)nf] = (int32_t)rows_n;
        const int64_t n_tail = rows_n + rnd(0, 3);      // the survivors: at least as many as the assembled rows
        std::vector<double> purged((size_t)(n_tail + nf) * 10);
        for (size_t q = 0; q < purged.size(); ++q) purged[q] = (double)q + 0.25;
        int64_t got = -1;
        CHECK(hg::tail_segments_refusal(seg.data(), nf, n_tail, &got).empty() && got == kept);
        const bool with_before = it % 3 != 0;      // n_before_purge is optional
        std::vector<double> out((size_t)kept * 10 + 1, -1.0), want((size_t)kept * 10 + 1, -1.0);
        std::vector<int32_t> ff((size_t)nf + 1, -7), before((size_t)nf, -7);
        hg::tail_place(seg.data(), purged.data(), nf, out.data(), ff.data(), with_before ? before.data() : nullptr);
        int64_t at = 0;
        for (int f = 0; f < nf; ++f) {
            CHECK(ff[(size_t)f] == at);
            CHECK(before[(size_t)f] == (with_before ? seg[(size_t)f + 1] - seg[(size_t)f] : -7));
            for (int j = 0; j < seg[(size_t)nf + 1 + f]; ++j, ++at)
                for (int q = 0; q < 10; ++q) want[(size_t)at * 10 + q] = purged[(size_t)(seg[(size_t)f] + f + j) * 10 + q];
        }
        CHECK(ff[(size_t)nf] == kept && at == kept && out == want);      // (the guard element behind the rows is untouched)
        // ---- every segment word out of range is refused, naming the frame -----------------------------------------------------
        const int bf = rnd(0, nf - 1);
        char name[32];
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<int32_t> bad = seg;
            int64_t n_bad = n_tail;
            int named = bf;
            const int32_t nb = bad[(size_t)bf + 1] - bad[(size_t)bf];
            if (kind == 0) {      // a negative first row (the frames before it then hold a negative number of rows: the first bad frame is named)
                for (int f = 0; f <= bf; ++f) bad[(size_t)f] = -1 - (bf - f);
                named = 0;
            } else if (kind == 1) {      // a negative number of rows
                bad[(size_t)bf + 1] = bad[(size_t)bf] - 1;
            } else if (kind == 2) {      // rows beyond the survivors
                n_bad = bad[(size_t)bf + 1] - 1;
                if (n_bad < 0) continue;
                for (named = 0; bad[(size_t)named + 1] <= n_bad; ++named) {}
            } else if (kind == 3) {      // a negative kept count
                bad[(size_t)nf + 1 + bf] = -1;
            } else {      // more kept rows than the purge can write
                bad[(size_t)nf + 1 + bf] = nb + 2;
            }
            snprintf(name, sizeof name, "frame %d:", named);
            const std::string why = hg::tail_segments_refusal(bad.data(), nf, n_bad, &got);
            CHECK(!why.empty() && why.rfind(name, 0) == 0);
            ++refusals;
        }
        ++cases;
    }
    // no survivors at all, one frame and several
    for (int nf : {1, 5}) {
        std::vector<int32_t> first((size_t)nf + 1, 0), ff((size_t)nf + 1, -7);
        for (int f = 0; f < nf; ++f) first[(size_t)f + 1] = first[(size_t)f] + 9;
        hg::split_by_first(nullptr, 0, first.data(), nf, ff.data());
        for (int f = 0; f <= nf; ++f) CHECK(ff[(size_t)f] == 0);
        ++cases;
    }
    if (fails) return 1;
    printf("ok %d %d\n", cases, refusals);
    return 0;
}
