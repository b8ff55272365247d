// A fused plan as text (tests/plan_digest_driver.cpp, tests/test_fused_plan_host.py): every scalar of every stage in full, every
// non-empty array as its length and an FNV-1a 64 digest, the plan's own fields, the sub-tree runs and the per-call choices at the batch sizes
// around their documented edges.  A template over the stage and run types, so the same routine prints any plan that keeps the
// field names.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace plan_digest {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    }
    template <class T> void val(const T& v) { bytes(&v, sizeof v); }      // only for types without padding
};

// arrays: name=length:digest; an empty array is left out of the line
template <class T> void arr(FILE* f, const char* name, const std::vector<T>& v) {      // T: int32_t or float
    if (v.empty()) return;
    Fnv d;
    for (const T& x : v) d.val(x);
    fprintf(f, " %s=%zu:%016llx", name, v.size(), (unsigned long long)d.h);
}

// DChunk / DRun field by field: the structs' padding words are never part of a digest
template <class C> void chunks(FILE* f, const std::vector<C>& v) {
    if (v.empty()) return;
    Fnv d;
    for (const C& c : v) { d.val(c.node_begin); d.val(c.node_count); d.val(c.run_begin); d.val(c.run_count); d.val(c.n_cols); d.val(c.piece_begin); d.val(c.n_pieces); }
    fprintf(f, " chunks=%zu:%016llx", v.size(), (unsigned long long)d.h);
}
template <class R> void runs(FILE* f, const std::vector<R>& v) {
    if (v.empty()) return;
    Fnv d;
    for (const R& r : v) { d.val(r.start); d.val(r.len); d.val(r.lds_off); }
    fprintf(f, " runs=%zu:%016llx", v.size(), (unsigned long long)d.h);
}

// the scalars of a stage, in the order print_stage writes their values (first line of every plan)
constexpr const char* kStageFields =
    "kind mt1 mt2 mto nb_out nb_in n_nodes kb1 nf node_blocks bias_floats nk_last p_max s_max rem4 pack_out pack_soa pack_in pk_kbi has_exp contig4 vec_ok "
    "direct_ok lds_stride max_chunk_nodes max_chunk_pieces neb has_clip clip_lo clip_hi from_x ig_has_lr ig_folded ig_nks mfma_per_tile mfma16_tile mfma4_tile "
    "ks1_tile ks2_tile nk2 funcs";

template <class Stage> void print_stage(FILE* f, int i, const Stage& s) {
    fprintf(f, "stage %d: %d %d %d %d %d %d %d %d %d %d %d %d %d %d", i, s.kind, s.mt1, s.mt2, s.mto, s.nb_out, s.nb_in, s.n_nodes, s.kb1, s.nf, s.node_blocks,
            s.bias_floats, s.nk_last, s.p_max, s.s_max);
    fprintf(f, " %d %d %d %d %d %d %d %d %d %d %d %d", (int)s.rem4, (int)s.pack_out, (int)s.pack_soa, s.pack_in, s.pk_kbi, (int)s.has_exp, (int)s.contig4, (int)s.vec_ok,
            (int)s.direct_ok, s.lds_stride, s.max_chunk_nodes, s.max_chunk_pieces);
    fprintf(f, " %d %d %.9g %.9g %d %d %d %d,%d,%d,%d", s.neb, (int)s.has_clip, (double)s.clip_lo, (double)s.clip_hi, (int)s.from_x, (int)s.ig_has_lr, (int)s.ig_folded,
            s.ig_nks[0], s.ig_nks[1], s.ig_nks[2], s.ig_nks[3]);
    fprintf(f, " %lld %lld %lld %lld %lld ", (long long)s.mfma_per_tile, (long long)s.mfma16_tile, (long long)s.mfma4_tile, (long long)s.ks1_tile, (long long)s.ks2_tile);
    for (size_t a = 0; a < sizeof s.nk2 / sizeof s.nk2[0]; ++a)
        for (size_t b = 0; b < sizeof s.nk2[0]; ++b) fprintf(f, "%d", (int)s.nk2[a][b]);
    fprintf(f, " [");
    for (const auto& fn : s.funcs) fprintf(f, "(%u,%u,%u,%.17g)", fn.kind, fn.sel, fn.k, fn.expo);
    fprintf(f, "]\nstage %d arrays:", i);
    arr(f, "afrag", s.afrag);
    arr(f, "bias", s.bias);
    arr(f, "kb1tab", s.kb1tab);
    chunks(f, s.chunks);
    runs(f, s.runs);
    arr(f, "piece_col", s.piece_col);
    arr(f, "koff", s.koff);
    arr(f, "kmean", s.kmean);
    arr(f, "kcol", s.kcol);
    arr(f, "gcol", s.gcol);
    arr(f, "etab", s.etab);
    arr(f, "pack_slot", s.pack_slot);
    fprintf(f, "\nstage %d name: %s\n", i, s.name.c_str());
}

constexpr int kTiles[] = {1, 2, 3, 8, 9, 32, 33, 45, 64, 65, 95, 96, 200};      // 16-row tiles: around the 44 / 130 / 512 / 728-row and 96-tile edges

template <class Stages, class Runs, class PickSet, class TailStart>
void print_plan(FILE* f, const Stages& stages, const std::vector<int32_t>& col_base, const std::vector<int32_t>& col_of, const Runs& sub_runs, int tail_begin,
                int tail_act_blocks, int tail_e_blocks, bool fuse01, bool s0_transpose, int max_nb, long long padded_flops, PickSet pick_sub_set,
                TailStart tail_start) {
    fprintf(f, "stage fields: %s\n", kStageFields);
    int i = 0;
    for (const auto& s : stages) print_stage(f, i++, s);
    fprintf(f, "plan:");
    arr(f, "col_base", col_base);
    arr(f, "col_of", col_of);
    fprintf(f, " tail_begin=%d tail_act_blocks=%d tail_e_blocks=%d fuse01=%d s0_transpose=%d max_nb=%d padded_flops=%lld\n", tail_begin, tail_act_blocks, tail_e_blocks,
            (int)fuse01, (int)s0_transpose, max_nb, padded_flops);
    i = 0;
    for (const auto& r : sub_runs) {
        fprintf(f, "sub-run %d: begin=%d len=%d n=%d act_blocks=%d e_blocks=%d set=%d", i++, r.begin, r.len, r.n, r.act_blocks, r.e_blocks, r.set);
        for (size_t k = 0; k < sizeof r.nodes / sizeof r.nodes[0]; ++k) {
            char name[16];
            snprintf(name, sizeof name, "nodes%zu", k);
            arr(f, name, r.nodes[k]);
            snprintf(name, sizeof name, "tab%zu", k);
            arr(f, name, r.tab[k]);
        }
        fprintf(f, "\n");
    }
    fprintf(f, "choices (tiles:sub_set,tail_start):");
    for (int t : kTiles) fprintf(f, " %d:%d,%d", t, pick_sub_set(t), tail_start(t));
    fprintf(f, "\n");
}

}  // namespace plan_digest
