// The planner's packing of the folded link's one-row k-steps without a device (host only; links hg_tree.cpp and hg_fused_plan.cpp and nothing
// of HIP).
//   fold01_pack_plan_driver [--fold 0|1] [--pack 0|1] [--digest] [--nodes a,b,...] FILE...
// plans every blob with FusedOptions::hoist on, fold01 and fold01_pack as given (default 1 1) and the environment's other switches, and prints
//       == <file name>
//       fold01 <0|1> pack <0|1> s0_transpose <0|1> padded_flops <issued> given <as given>
//       note <FusedPlan::fold01_note>
//       pack_note <FusedPlan::fold01_pack_note>
//       name1 <stage 1's name>
//       issue <stage> <mfma16_tile> <mfma4_tile>                      stages 0 and 1
//   --digest: the plan as tests/plan_digest.hpp prints it, every line behind "D ", and one more line with the folded arrays' digests
//   a packed plan, per layer-1 node q of --nodes (default: all), un-permuted from the fragment order the kernels read:
//       F q child <32 x 32 floats>          fold_frag: row = 16 x function + z0 feature of the child, column = z1 feature (as fold01_plan_driver)
//       last q tile <64 floats>             fold_last as stored: lane (g, i) at position 16 g + i
//     and per layer-0 node c = 2 q, 2 q + 1, the packed first affine and the plan's own, rows = tile rows, columns = k slots 4 r + g:
//       a1 c <16 x 16 floats>   a1_plain c <16 x 16 floats>   b1 c <16 floats>   b1_plain c <16 floats>
//   -DPLAN_WITHOUT_PACK builds the driver against a planner that has no fold01_pack yet (--pack 0 only): how
//   tests/golden/fold01_pack_off_digests.json was recorded from the commit before the option.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "hg_fused_plan.hpp"
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

static void print_block_rows(const char* tag, int node, const float* blk) {      // [lane = 16 g + i][r] -> row i, column 4 r + g
    printf("%s %d", tag, node);
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 16; ++k) printf(" %.9g", blk[((k & 3) * 16 + i) * 4 + (k >> 2)]);
    printf("\n");
}

int main(int argc, char** argv) {
    using namespace hg::fused;
    FusedOptions opt = FusedOptions::from_env();
    opt.hoist = true;
    bool fold = true, pack = true, digest = false;
    std::set<int> only;
    int i = 1;
    for (; i < argc && argv[i][0] == '-'; ++i) {
        if (!strcmp(argv[i], "--fold") && i + 1 < argc) fold = atoi(argv[++i]) != 0;
        else if (!strcmp(argv[i], "--pack") && i + 1 < argc) pack = atoi(argv[++i]) != 0;
        else if (!strcmp(argv[i], "--digest")) digest = true;
        else if (!strcmp(argv[i], "--nodes") && i + 1 < argc) {
            for (char* t = strtok(argv[++i], ","); t; t = strtok(nullptr, ",")) only.insert(atoi(t));
        } else {
            fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    opt.fold01 = fold;
#ifndef PLAN_WITHOUT_PACK
    opt.fold01_pack = pack;
#else
    if (pack) {
        fprintf(stderr, "this build has no fold01_pack\n");
        return 2;
    }
#endif
    for (; i < argc; ++i) {
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
#ifndef PLAN_WITHOUT_PACK
            const bool packed = p.fold01_pack;
            const std::string pack_note = p.fold01_pack_note;
#else
            const bool packed = false;
            const std::string pack_note;
#endif
            printf("fold01 %d pack %d s0_transpose %d padded_flops %lld given %lld\n", p.fold01 ? 1 : 0, packed ? 1 : 0, p.s0_transpose ? 1 : 0,
                   (long long)p.padded_flops, (long long)p.padded_flops_given);
            printf("note %s\npack_note %s\n", p.fold01_note.c_str(), pack_note.c_str());
            printf("name1 %s\n", p.stages.size() > 1 ? p.stages[1].name.c_str() : "");
            for (size_t s = 0; s < 2 && s < p.stages.size(); ++s)
                printf("issue %zu %lld %lld\n", s, (long long)p.stages[s].mfma16_tile, (long long)p.stages[s].mfma4_tile);
            if (digest) {
                char* text = nullptr;
                size_t len = 0;
                FILE* m = open_memstream(&text, &len);
                plan_digest::print_plan(m, p.stages, p.col_base, p.col_of, p.sub_runs, p.tail_begin, p.tail_act_blocks, p.tail_e_blocks, p.fuse01, p.s0_transpose,
                                        p.max_nb, (long long)p.padded_flops, [&](int t) { return p.pick_sub_set(t); }, [&](int t) { return p.tail_start(t); });
                fprintf(m, "folded:");
                if (p.stages.size() > 1) {
                    plan_digest::arr(m, "fold_frag", p.stages[1].fold_frag);
                    plan_digest::arr(m, "fold_bias", p.stages[1].fold_bias);
                }
                fprintf(m, " fold01=%d given=%lld\n", (int)p.fold01, (long long)p.padded_flops_given);
                fclose(m);
                for (char* ln = strtok(text, "\n"); ln; ln = strtok(nullptr, "\n")) printf("D %s\n", ln);
                free(text);
            }
#ifndef PLAN_WITHOUT_PACK
            if (!packed) {
                if (p.stages.size() > 1 && (!p.stages[1].fold_last.empty() || !p.stages[0].fold_a1.empty() || !p.stages[0].fold_b1.empty())) {
                    printf("packed arrays on a plan that is not packed\n");
                    return 3;
                }
                continue;
            }
            const HostStage &s0 = p.stages[0], &st = p.stages[1];
            if (st.fold_frag.size() != (size_t)st.n_nodes * 8 * 256 || st.fold_last.size() != (size_t)st.n_nodes * 128 ||
                s0.fold_a1.size() != (size_t)s0.n_nodes * 256 || s0.fold_b1.size() != (size_t)s0.n_nodes * 16 || s0.n_nodes != 2 * st.n_nodes) {
                printf("bad array sizes\n");
                return 3;
            }
            for (int q = 0; q < st.n_nodes; ++q) {
                if (!only.empty() && !only.count(q)) continue;
                for (int sl = 0; sl < 2; ++sl) {
                    std::vector<float> F(32 * 32, 0.f);
                    for (int fi = 0; fi < 2; ++fi)
                        for (int mt = 0; mt < 2; ++mt) {
                            const float* blk = st.fold_frag.data() + ((((size_t)q * 2 + sl) * 2 + fi) * 2 + mt) * 256;
                            for (int lane = 0; lane < 64; ++lane) {
                                const int g = lane >> 4, l = lane & 15;
                                for (int r = 0; r < 4; ++r) {
                                    const float v = blk[lane * 4 + r];
                                    const int fz = 4 * r + g;
                                    if (mt == 0) {
                                        F[(size_t)(16 * fi + fz) * 32 + 4 * (l & 3) + (l >> 2)] = v;
                                    } else {
                                        const float first = blk[((lane & 48) | (lane & 3)) * 4 + r];
                                        if (memcmp(&v, &first, 4) != 0) {
                                            printf("4x4-form repeat differs: node %d child %d function %d lane %d\n", q, sl, fi, lane);
                                            return 3;
                                        }
                                        F[(size_t)(16 * fi + fz) * 32 + 16 + (l & 3)] = v;
                                    }
                                }
                            }
                        }
                    printf("F %d %d", q, sl);
                    for (float v : F) printf(" %.9g", v);
                    printf("\n");
                }
                for (int mt = 0; mt < 2; ++mt) {
                    printf("last %d %d", q, mt);
                    for (int lane = 0; lane < 64; ++lane) printf(" %.9g", st.fold_last[((size_t)q * 2 + mt) * 64 + lane]);
                    printf("\n");
                }
                for (int c = 2 * q; c < 2 * q + 2; ++c) {
                    print_block_rows("a1", c, s0.fold_a1.data() + (size_t)c * 256);
                    print_block_rows("a1_plain", c, s0.afrag.data() + (size_t)c * s0.node_blocks * 256);
                    printf("b1 %d", c);
                    for (int k = 0; k < 16; ++k) printf(" %.9g", s0.fold_b1[(size_t)c * 16 + k]);
                    printf("\nb1_plain %d", c);
                    for (int k = 0; k < 16; ++k) printf(" %.9g", s0.bias[(size_t)c * s0.bias_floats + k]);
                    printf("\n");
                }
            }
#endif
        } catch (const hg::Error& e) {
            printf("blob rejected: %s\n", e.what());
        }
    }
    return 0;
}
