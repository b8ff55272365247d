// The fused planner without a device (host only; links hg_tree.cpp and hg_fused_plan.cpp and nothing of HIP): for every blob file on
// the command line, the plan build_fused_plan makes of it under the HIGSFA_* switches of the environment, as text
// (tests/plan_digest.hpp), or the reason it refuses.
#include <cstdio>
#include <string>
#include <vector>

#include "hg_fused_plan.hpp"
#include "plan_digest.hpp"

int main(int argc, char** argv) {
    const hg::fused::FusedOptions opt = hg::fused::FusedOptions::from_env();
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<unsigned char> b;
        unsigned char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
        fclose(f);
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
            plan_digest::print_plan(stdout, p.stages, p.col_base, p.col_of, p.sub_runs, p.tail_begin, p.tail_act_blocks, p.tail_e_blocks, p.fuse01, p.s0_transpose,
                                    p.max_nb, (long long)p.padded_flops, [&](int t) { return p.pick_sub_set(t); }, [&](int t) { return p.tail_start(t); });
        } catch (const hg::Error& e) {
            printf("blob rejected: %s\n", e.what());
        }
    }
    return 0;
}
