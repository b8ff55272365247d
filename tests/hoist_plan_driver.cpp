// The hoist pass of the fused planner and the executor's call plan without a device (host only; links hg_tree.cpp, hg_fused_plan.cpp and
// hg_fused_call.cpp and nothing of HIP).
//   hoist_plan_driver FILE...          for every blob: the stages whose first affine was hoisted, then the plan build_fused_plan makes
//                                      with FusedOptions::hoist on (tests/plan_digest.hpp), or the reason it refuses
//   hoist_plan_driver --dump FILE      the normal form after hoist_first_affines, in full float64: per hoisted parent node its children
//                                      and bias vector, per child node the folded second affine
//   hoist_plan_driver --links FILE...  for every blob, per node of a hoisted stage: stage, node, columns of z, children in the order
//                                      their tiles are added
//   hoist_plan_driver --call TILES[,TILES...] [--occ K] [--no-vec4] FILE...
//                                      for every blob and tile count the call plan (hg_fused_call.hpp) of the plan the executor makes:
//                                      per step its route, first stage, stages covered, summed input, sub-tree set and grid, then
//                                      the step's HIGSFA_DEBUG line with tile_parts at K resident workgroups per CU (default 1)
//   hoist_plan_driver --rule parts GROUPS TILE_GROUPS OCC | --rule sweep TILES GROUPS | --rule sweepgrid TILES_MAX GROUPS_MAX
//                                      sweep_tile_parts; the waves x tiles of the ordinary sweep; the same for tiles 1 .. TILES_MAX (a line
//                                      each) x node groups 1 .. GROUPS_MAX
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hg_fused_call.hpp"
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

static const char* base_name(const char* path) {
    const char* base = path;
    for (const char* c = path; *c; ++c)
        if (*c == '/') base = c + 1;
    return base;
}

// --call: the executor's plan of every blob (hg::fused::executor_options) and, per tile count, what a call of float32 rows of the
// flow's own width launches
static int call(int argc, char** argv) {
    using namespace hg::fused;
    std::vector<int> tiles;
    for (const char* c = argv[2]; *c;) {
        tiles.push_back(atoi(c));
        while (*c && *c != ',') ++c;
        if (*c) ++c;
    }
    int occ = 1, i = 3;
    FrontInput fi;
    for (; i < argc && argv[i][0] == '-'; ++i) {
        if (!strcmp(argv[i], "--occ") && i + 1 < argc) occ = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--no-vec4")) fi.vec4_ok = false;
        else return 2;
    }
    std::vector<CallStep> steps;
    char line[512];
    for (; i < argc; ++i) {
        const auto b = slurp(argv[i]);
        printf("== %s\n", base_name(argv[i]));
        try {
            const auto tree = hg::parse_blob(b.data(), b.size());
            std::string why;
            const auto plan = build_fused_plan(*tree, executor_options(), &why);
            if (!plan) {
                printf("refused: %s\n", why.c_str());
                continue;
            }
            fi.ldx = tree->in_dim;
            printf("plan stages %zu fuse01 %d fold01 %d tail_begin %d\n", plan->stages.size(), (int)plan->fuse01, (int)plan->fold01, plan->tail_begin);
            for (int t : tiles) {
                plan_call(*plan, t, fi, steps);
                printf("call tiles %d steps %zu\n", t, steps.size());
                for (const CallStep& st : steps) {
                    const int parts = step_tile_parts(st, occ);
                    printf("step %s stage %d covered %d summed %d set %d blocks %lld | %s\n", route_name(st.route), st.stage, st.covered, (int)st.in_summed,
                           st.sub_run >= 0 ? plan->sub_runs[st.sub_run].set : -1, st.route == Route::Top ? 1ll : (long long)step_blocks(st, parts),
                           format_step(*plan, st, occ, parts, line, sizeof line));
                }
            }
        } catch (const hg::Error& e) {
            printf("failed: %s\n", e.what());
        }
    }
    return 0;
}

// --rule: one launch rule at given values
static int rule(int argc, char** argv) {
    using namespace hg::fused;
    if (argc == 6 && !strcmp(argv[2], "parts")) return printf("%d\n", sweep_tile_parts(atoi(argv[3]), atoi(argv[4]), atoi(argv[5]))) < 0;
    if (argc == 5 && !strcmp(argv[2], "sweep")) {
        const WavesTiles w = stage_sweep_shape(atoi(argv[3]), atoi(argv[4]));
        return printf("%dx%d\n", w.nw, w.T) < 0;
    }
    if (argc == 5 && !strcmp(argv[2], "sweepgrid")) {
        for (int t = 1; t <= atoi(argv[3]); ++t)
            for (int g = 1, gn = atoi(argv[4]); g <= gn; ++g) {
                const WavesTiles w = stage_sweep_shape(t, g);
                printf("%dx%d%c", w.nw, w.T, g == gn ? '\n' : ' ');
            }
        return 0;
    }
    return 2;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--dump")) return dump(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "--links")) return links(argc, argv);
    if (argc >= 4 && !strcmp(argv[1], "--call")) return call(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "--rule")) return rule(argc, argv);
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
