// The planner's summed-link tables without a device (host only; links hg_tree.cpp and hg_fused_plan.cpp and nothing of HIP).
//   pair_plan_driver FILE...        for every blob, with FusedOptions::hoist and ::pair on: per node of a hoisted stage its children in the
//                                   normal form (FNode::kids, "link"), then per stage of the plan what Planner::plan_pairs recorded:
//                                   shape, name, pair_kids, kb1tab_pre, and bias / bias_pre as bit patterns
//   pair_plan_driver --off FILE...  the plan with hoist OFF and pair on (tests/plan_digest.hpp): the recorded plans, unchanged
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hg_fused_plan.hpp"
#include "hg_fused_stages.hpp"
#include "plan_digest.hpp"

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> b;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

static void print_bits(const char* what, size_t si, const std::vector<float>& v) {
    printf("%s %zu:", what, si);
    for (float x : v) {
        unsigned u;
        memcpy(&u, &x, 4);
        printf(" %08x", u);
    }
    printf("\n");
}

static void print_ints(const char* what, size_t si, const std::vector<int32_t>& v) {
    printf("%s %zu:", what, si);
    for (int32_t x : v) printf(" %d", (int)x);
    printf("\n");
}

int main(int argc, char** argv) {
    using namespace hg::fused;
    const bool off = argc >= 2 && !strcmp(argv[1], "--off");
    FusedOptions opt = FusedOptions::from_env();
    opt.hoist = !off;
    opt.pair = true;
    for (int i = off ? 2 : 1; i < argc; ++i) {
        const auto b = slurp(argv[i]);
        const char* base = argv[i];
        for (const char* c = argv[i]; *c; ++c)
            if (*c == '/') base = c + 1;
        printf("== %s\n", base);
        try {
            const auto tree = hg::parse_blob(b.data(), b.size());
            std::string why;
            const auto plan = build_fused_plan(*tree, opt, &why);
            if (!plan) {
                printf("refused: %s\n", why.c_str());
                continue;
            }
            const FusedPlan& p = *plan;
            if (off) {
                for (auto& hs : p.stages)
                    if (!hs.pair_kids.empty() || !hs.kb1tab_pre.empty() || !hs.bias_pre.empty()) printf("pairs in a plan without hoisted links\n");
                plan_digest::print_plan(stdout, p.stages, p.col_base, p.col_of, p.sub_runs, p.tail_begin, p.tail_act_blocks, p.tail_e_blocks, p.fuse01, p.s0_transpose,
                                        p.max_nb, (long long)p.padded_flops, [&](int t) { return p.pick_sub_set(t); }, [&](int t) { return p.tail_start(t); });
                continue;
            }
            std::vector<FStage> fs;
            if (!build_stages(*tree, fs, why, opt)) {
                printf("refused: %s\n", why.c_str());
                continue;
            }
            for (int pi : hoist_first_affines(fs, opt))
                for (size_t j = 0; j < fs[pi].nodes.size(); ++j) {
                    printf("link %d %zu:", pi, j);
                    for (int k : fs[pi].nodes[j].kids) printf(" %d", k);
                    printf("\n");
                }
            for (size_t si = 0; si < p.stages.size(); ++si) {
                const HostStage& hs = p.stages[si];
                printf("stage %zu: sum_in %d n_nodes %d mt1 %d mt2 %d kb1 %d bias_floats %d paired %d\n", si, hs.sum_in ? 1 : 0, hs.n_nodes, hs.mt1, hs.mt2, hs.kb1,
                       hs.bias_floats, hs.pair_kids.empty() ? 0 : 1);
                printf("name %zu: %s\n", si, hs.name.c_str());
                if (hs.pair_kids.empty()) {
                    if (!hs.kb1tab_pre.empty() || !hs.bias_pre.empty()) printf("tables without pairs\n");
                    continue;
                }
                print_ints("kids", si, hs.pair_kids);
                print_ints("tab", si, hs.kb1tab_pre);
                print_bits("bias", si, hs.bias);
                print_bits("biaspre", si, hs.bias_pre);
            }
        } catch (const hg::Error& e) {
            printf("blob rejected: %s\n", e.what());
        }
    }
    return 0;
}
