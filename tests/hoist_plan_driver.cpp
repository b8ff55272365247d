// The hoist pass of the fused planner without a device (host only; links hg_tree.cpp and hg_fused_plan.cpp and nothing of HIP).
//   hoist_plan_driver FILE...          for every blob: the stages whose first affine was hoisted, then the plan build_fused_plan makes
//                                      with FusedOptions::hoist on (tests/plan_digest.hpp), or the reason it refuses
//   hoist_plan_driver --dump FILE      the normal form after hoist_first_affines, in full float64: per hoisted parent node its children
//                                      and bias vector, per child node the folded second affine
//   hoist_plan_driver --links FILE...  for every blob, per node of a hoisted stage: stage, node, columns of z, children in the order
//                                      their tiles are added
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

static int dump(const char* path) {
    using namespace hg::fused;
    const auto b = slurp(path);
    const auto tree = hg::parse_blob(b.data(), b.size());
    FusedOptions opt = FusedOptions::from_env();
    opt.hoist = true;
    std::vector<FStage> fs;
    std::string why;
    if (!build_stages(*tree, fs, why, opt)) {
        printf("refused: %s\n", why.c_str());
        return 0;
    }
    const std::vector<int> parents = hoist_first_affines(fs, opt);
    for (int pi : parents) {
        const FStage& pa = fs[pi];
        const FStage& ch = fs[pi - 1];
        for (size_t j = 0; j < pa.nodes.size(); ++j) {
            const FNode& n = pa.nodes[j];
            printf("parent %d %zu kids", pi, j);
            for (int k : n.kids) printf(" %d", k);
            printf(" bias");
            for (double v : n.sum_bias) printf(" %.17g", v);
            printf("\n");
        }
        for (size_t i = 0; i < ch.nodes.size(); ++i) {
            const Aff& a = ch.nodes[i].A2;
            double c = 0;      // what is left of the child's own constants: nothing
            for (double v : a.a) c = c > (v < 0 ? -v : v) ? c : (v < 0 ? -v : v);
            for (double v : a.b) c = c > (v < 0 ? -v : v) ? c : (v < 0 ? -v : v);
            printf("child %d %zu shape %d %d const %.17g W", pi - 1, i, a.in, a.out, c);
            for (double v : a.W) printf(" %.17g", v);
            printf("\n");
        }
    }
    return 0;
}

static int links(int argc, char** argv) {
    using namespace hg::fused;
    for (int i = 2; i < argc; ++i) {
        const auto b = slurp(argv[i]);
        const auto tree = hg::parse_blob(b.data(), b.size());
        FusedOptions opt = FusedOptions::from_env();
        opt.hoist = true;
        std::vector<FStage> fs;
        std::string why;
        printf("== %d\n", i - 2);
        if (!build_stages(*tree, fs, why, opt)) {
            printf("refused: %s\n", why.c_str());
            continue;
        }
        for (int pi : hoist_first_affines(fs, opt))
            for (size_t j = 0; j < fs[pi].nodes.size(); ++j) {
                const FNode& n = fs[pi].nodes[j];
                printf("parent %d %zu cols %zu kids", pi, j, n.sum_bias.size());
                for (int k : n.kids) printf(" %d", k);
                printf("\n");
            }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--dump")) return dump(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "--links")) return links(argc, argv);
    hg::fused::FusedOptions opt = hg::fused::FusedOptions::from_env();
    opt.hoist = true;
    for (int i = 1; i < argc; ++i) {
        const auto b = slurp(argv[i]);
        const char* base = argv[i];
        for (const char* c = argv[i]; *c; ++c)
            if (*c == '/') base = c + 1;
        printf("== %s\n", base);
        try {
            const auto tree = hg::parse_blob(b.data(), b.size());
            std::string why;
            const auto plan = hg::fused::build_fused_plan(*tree, opt, &why);
            if (!plan) {
                printf("refused: %s\n", why.c_str());
                continue;
            }
            const hg::fused::FusedPlan& p = *plan;
            printf("hoisted:");
            for (size_t s = 0; s < p.stages.size(); ++s)
                if (p.stages[s].sum_in) printf(" %zu", s);
            printf("\n");
            plan_digest::print_plan(stdout, p.stages, p.col_base, p.col_of, p.sub_runs, p.tail_begin, p.tail_act_blocks, p.tail_e_blocks, p.fuse01, p.s0_transpose,
                                    p.max_nb, (long long)p.padded_flops, [&](int t) { return p.pick_sub_set(t); }, [&](int t) { return p.tail_start(t); });
        } catch (const hg::Error& e) {
            printf("blob rejected: %s\n", e.what());
        }
    }
    return 0;
}
