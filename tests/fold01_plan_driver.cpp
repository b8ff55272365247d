// The planner's fold of the link 0 -> 1 without a device (host only; links hg_tree.cpp and hg_fused_plan.cpp and nothing of HIP).
//   fold01_plan_driver FILE...   for every blob, planned with FusedOptions::fold01 on (and the environment's other switches):
//       == <file name>
//       fold01 <0|1> fuse01 <0|1> padded_flops <issued> given <as given> note <FusedPlan::fold01_note>
//       name0 / name1 <stage names>
//       issue <stage> <mfma16_tile> <mfma4_tile>                      stages 0 and 1
//       chunks <node chunks of stage 0>
//     and where the link is folded, per layer-1 node q, un-permuted from the fragment order the kernels read:
//       bias q <32 floats>                  z1 feature o at position o (two tiles of 16)
//       F q child <32 x 32 floats>          row = 16 x function + z0 feature of the child, column = z1 feature
//     Tile 1 is stored in 4x4 form: of a lane group's 16 lanes four hold a row each and the other twelve repeat them; the driver checks
//     the repeats and fails (exit 3) where one differs.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hg_fused_plan.hpp"

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

int main(int argc, char** argv) {
    using namespace hg::fused;
    FusedOptions opt = FusedOptions::from_env();
    opt.hoist = true;
    opt.fold01 = true;
    for (int i = 1; i < argc; ++i) {
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
            printf("fold01 %d fuse01 %d padded_flops %lld given %lld note %s\n", p.fold01 ? 1 : 0, p.fuse01 ? 1 : 0, (long long)p.padded_flops,
                   (long long)p.padded_flops_given, p.fold01_note.c_str());
            for (size_t s = 0; s < 2 && s < p.stages.size(); ++s) printf("name%zu %s\n", s, p.stages[s].name.c_str());
            for (size_t s = 0; s < 2 && s < p.stages.size(); ++s)
                printf("issue %zu %lld %lld\n", s, (long long)p.stages[s].mfma16_tile, (long long)p.stages[s].mfma4_tile);
            printf("chunks %zu\n", p.stages[0].chunks.size());
            if (!p.fold01) continue;
            const HostStage& st = p.stages[1];
            if (st.fold_frag.size() != (size_t)st.n_nodes * 8 * 256 || st.fold_bias.size() != (size_t)st.n_nodes * 32) {
                printf("bad array sizes\n");
                return 3;
            }
            for (int q = 0; q < st.n_nodes; ++q) {
                printf("bias %d", q);
                for (int o = 0; o < 32; ++o) {      // feature 16 mt + 4 r + g sits at [mt][g][r]
                    const int mt = o / 16, r = (o % 16) / 4, g = o % 4;
                    printf(" %.9g", st.fold_bias[(size_t)q * 32 + mt * 16 + g * 4 + r]);
                }
                printf("\n");
                for (int sl = 0; sl < 2; ++sl) {
                    std::vector<float> F(32 * 32, 0.f);
                    for (int fi = 0; fi < 2; ++fi)
                        for (int mt = 0; mt < 2; ++mt) {
                            const float* blk = st.fold_frag.data() + ((((size_t)q * 2 + sl) * 2 + fi) * 2 + mt) * 256;
                            for (int lane = 0; lane < 64; ++lane) {
                                const int g = lane >> 4, i = lane & 15;
                                for (int r = 0; r < 4; ++r) {
                                    const float v = blk[lane * 4 + r];
                                    const int fz = 4 * r + g;
                                    if (mt == 0) {
                                        F[(size_t)(16 * fi + fz) * 32 + 4 * (i & 3) + (i >> 2)] = v;      // tile row i holds feature 4 (i % 4) + i / 4
                                    } else {      // 4x4 form: lane (g, i % 4) holds the tile's row 4 (i % 4), i.e. feature 16 + i % 4
                                        const float first = blk[((lane & 48) | (lane & 3)) * 4 + r];
                                        if (memcmp(&v, &first, 4) != 0) {
                                            printf("4x4-form repeat differs: node %d child %d function %d lane %d\n", q, sl, fi, lane);
                                            return 3;
                                        }
                                        F[(size_t)(16 * fi + fz) * 32 + 16 + (i & 3)] = v;
                                    }
                                }
                            }
                        }
                    printf("F %d %d", q, sl);
                    for (float v : F) printf(" %.9g", v);
                    printf("\n");
                }
            }
        } catch (const hg::Error& e) {
            printf("blob rejected: %s\n", e.what());
        }
    }
    return 0;
}
