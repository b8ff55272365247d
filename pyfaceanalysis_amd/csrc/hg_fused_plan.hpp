// The fused plan: what the planner (hg_fused_plan.cpp, host only) makes of a flow tree and the executor (hg_fused.hip) uploads
// and launches from.  Plain host data — no HIP runtime, no device code, no device buffers — and read-only once built.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "hg_common.hpp"

namespace hg {
namespace fused {

constexpr int kMaxMT = 4;            // up to 64 outputs per affine in the fused plan

// Every stage is padded to a UNIFORM node structure (same K-block count, tile counts and
// expansion list for all its nodes; missing pieces are zero weights), so all weight / bias
// addresses are arithmetic on the node index and the only per-node table is the list of source
// blocks of GEMM 1.
constexpr int kMaxFuncs = 4;

constexpr int kMaxTail = 3;          // most layers one top-of-hierarchy or sub-tree launch runs (k_tail, k_subtree)

struct DChunk {   // stage 0: a group of consecutive nodes whose input columns share one LDS tile
    int32_t node_begin, node_count, run_begin, run_count, n_cols, piece_begin, n_pieces, pad1;
};
struct DRun {
    int32_t start, len, lds_off, pad;
};

// Diagnostic switches (DESIGN.md "Diagnostic environment variables"), read ONCE when a plan is built — never on the
// execute path.  None changes results beyond rounding.
struct FusedOptions {
    bool no_rem4 = false, ig_nofold = false, debug = false;
    int stamp_stage = -1;
    // batches of up to this many 16-row tiles run the top layers as one persistent launch (0: never).  Measured on U11L-128
    // (tools/small_batch2.py): 5-10 % of a call up to N = 128, a loss from N = 340 (one workgroup per node and slice cannot
    // match the per-layer kernels' throughput), so the default stops at 8 tiles.
    bool no_pack = false;         // HIGSFA_NO_PACK: remainder tiles as whole blocks
    bool no_soa = false;          // HIGSFA_NO_SOA: packed remainder blocks always lane-major (plan_slot_major off)
    uint32_t wq_start = 0;        // HIGSFA_WQ_START: initial value of the tile-queue counters (tests: wrap-around)
    bool no_wgq = false;          // HIGSFA_NO_WGQ: k_stage01d with one tile queue per layer-1 node instead of one per chunk (2-3 % faster, +29 % HBM bytes)
    bool no_direct = false;       // HIGSFA_NO_DIRECT: front kernel always stages the input rows through LDS (k_stage01p)
    int tail_max = 3;             // HIGSFA_TAIL: most layers k_tail fuses at the top of the hierarchy (0: off — per-layer launches + k_unpack)
    bool no_fspec = false;        // HIGSFA_NO_FSPEC: front kernel without the compile-time (identity, abs-power) expansion
    int subtree_max_tiles = 64;   // HIGSFA_SUBTREE: batches of up to this many 16-row tiles may run layers below the top as sub-trees (k_subtree); 0: never
    int subtree_max_wgs = 256;    // HIGSFA_SUBTREE_WGS: ... while sub-trees x tiles stays within this many workgroups
    int splitm_max_nodes = 4;     // experiments: HIGSFA_SPLITM_MAX
    int splitm_max_wgs = 512;     // HIGSFA_SPLITM_WGS: largest k_stage_splitm grid for layers of more than splitm_max_nodes nodes
    int sum_lds_kib = 32;         // HIGSFA_SUM_LDS: KiB of second-affine fragments a k_stage_sum workgroup keeps in LDS (node group of a hoisted layer)
    bool hoist = false;           // fold each parent's first affine into its children's second affine where the link allows it (hoist_first_affines);
                                  // not an environment switch of the planner: the executor turns it on unless HIGSFA_NO_HOIST is set
    bool fold01 = false;          // fold layer 0's second affine into layer 1's first inside the front kernels (Planner::plan_fold01); like hoist,
                                  // the executor's switch: on unless HIGSFA_NO_FOLD01 is set
    bool fold01_pack = false;     // with fold01: the four one-row k-steps of the folded link (feature 12 of a 13-output layer 0, per child and function) packed
                                  // into ONE k-step (Planner::plan_fold01_pack); the executor's switch: on unless HIGSFA_NO_FOLD01_PACK is set
    bool pair = false;            // record, for hoisted stages whose parents all have two children, what the layer below needs to store
                                  // (bias + child 0) + child 1 once per parent (Planner::plan_pairs); rides on hoist, and like it
                                  // the executor's switch: on unless HIGSFA_NO_PAIR is set
    int pair_min_wgs = 512;       // HIGSFA_PAIR_WGS: a link is stored summed in a call while pair groups x tile groups of its producer reach this
    static FusedOptions from_env() {
        FusedOptions o;
        o.no_rem4 = getenv("HIGSFA_NO_REM4") != nullptr;
        o.ig_nofold = getenv("HIGSFA_IG_NOFOLD") != nullptr;
        o.debug = getenv("HIGSFA_DEBUG") != nullptr;
        if (const char* e = getenv("HIGSFA_STAMP")) o.stamp_stage = atoi(e);

        o.no_pack = getenv("HIGSFA_NO_PACK") != nullptr;
        o.no_soa = getenv("HIGSFA_NO_SOA") != nullptr;
        o.no_fspec = getenv("HIGSFA_NO_FSPEC") != nullptr;
        o.no_direct = getenv("HIGSFA_NO_DIRECT") != nullptr;
        o.no_wgq = getenv("HIGSFA_NO_WGQ") != nullptr;
        if (const char* e = getenv("HIGSFA_WQ_START")) o.wq_start = (uint32_t)strtoul(e, nullptr, 0);
        if (const char* e = getenv("HIGSFA_SPLITM_MAX")) o.splitm_max_nodes = atoi(e);
        if (const char* e = getenv("HIGSFA_SPLITM_WGS")) o.splitm_max_wgs = atoi(e);
        if (const char* e = getenv("HIGSFA_SUBTREE")) o.subtree_max_tiles = std::max(0, atoi(e));
        if (const char* e = getenv("HIGSFA_SUBTREE_WGS")) o.subtree_max_wgs = std::max(0, atoi(e));
        if (const char* e = getenv("HIGSFA_SUM_LDS")) o.sum_lds_kib = std::max(1, atoi(e));
        if (const char* e = getenv("HIGSFA_PAIR_WGS")) o.pair_min_wgs = std::max(0, atoi(e));
        if (const char* e = getenv("HIGSFA_TAIL")) o.tail_max = std::max(0, std::min(atoi(e), kMaxTail));
        return o;
    }
};

// layers [begin, begin + len) as n independent sub-trees in one launch (k_subtree, short batches; plan_subtree)
// Per layer of the run: [sub-tree][position] -> node of the layer, and (layers above the run's first) the K-block table with source blocks
// renumbered to the sub-tree's own activation buffer in LDS (position of the source node in the layer below x mto + tile).
// set: runs are planned in two alternative sets (plan_subtree); a call uses the runs of ONE set.
struct SubRun {
    int begin = 0, len = 0, n = 0, act_blocks = 0, e_blocks = 0, set = 0;
    std::vector<int32_t> nodes[kMaxTail], tab[kMaxTail];
};

struct HostStage {
    int mt1 = 1, mt2 = 1, mto = 1, nb_out = 0, nb_in = 0, n_nodes = 0, kb1 = 0, nf = 0;
    int node_blocks = 0, bias_floats = 0, nk_last = 4;
    int p_max = 0, s_max = 0;   // widest first / second affine of the layer (real outputs)
    bool rem4 = false;          // last tiles of both affines in 4x4 form (k_stage REM instantiations)
    bool pack_out = false;      // output: the remainder tiles of four sibling nodes share one block (StageParams::pack_base)
    bool pack_soa = false;      // ... stored slot-major (StageParams::pack_soa; plan_slot_major)
    int pack_in = 0x7fffffff;   // input: source blocks from this one on are slot-major packed blocks of the stage below (StageParams::pack_in)
    int pk_kbi = -1;            // ... and sit at this position of every node's K-block list
    std::vector<int32_t> pack_slot;
    bool has_exp = false, contig4 = false, vec_ok = false;
    std::vector<ExpFunc> funcs;
    uint8_t nk2[kMaxMT][kMaxFuncs] = {};
    std::vector<float> afrag, bias;
    std::vector<int32_t> kb1tab;  // int2 pairs
    // stage 0
    std::vector<DChunk> chunks;
    std::vector<DRun> runs;
    std::vector<int32_t> piece_col, koff;
    std::vector<float> kmean;
    std::vector<int32_t> kcol;     // k_stage01d: [node][g] first source column of the lane group's four (empty: not applicable)
    bool direct_ok = false;
    int lds_stride = 0, max_chunk_nodes = 0, max_chunk_pieces = 0;
    int kind = 0;            // 0: affine-expansion-affine layer, 1: row-major -> fragment gather, 2: iGSFA layer, 3: table-driven expansion
    int neb = 0;             // kind 3: K-blocks of the expanded input
    bool has_clip = false;
    float clip_lo = 0, clip_hi = 0;
    std::vector<int32_t> etab;
    bool from_x = false;     // reads the caller's row-major matrix
    bool ig_has_lr = false, ig_folded = false;
    int ig_nks[kMaxMT] = {};  // k-steps of each slow-feature tile
    std::vector<int32_t> gcol;
    int64_t mfma_per_tile = 0;
    int64_t mfma16_tile = 0, mfma4_tile = 0;      // instructions issued per batch tile, all nodes of the layer
    int64_t ks1_tile = 0, ks2_tile = 0;      // k-steps of the first / second affine summed over the layer's nodes (per batch tile): issue accounting
    std::string name;
    bool sum_in = false;     // hoisted link: no first affine; kb1tab lists the children's tiles child-major (entry i: z tile i % mt1; k-steps = 1 real, 0 padding)
    int n_kids = 0;          // ... children per node (kb1 / mt1)
    // The link 0 -> 1 folded (FusedPlan::fold01; stage 1 only).  Everything above stays as it is; the front kernels read these INSTEAD of
    // stage 0's second-affine and stage 1's first-affine fragments and of both biases between them:
    // fold_frag [node][child 0..1][function 0..1][tile: 0 = 16x16 form, 1 = 4x4 form][lane][4]: A fragments of F_c = A2_c A1[rows of c, :]
    // (k = z0 feature 4 r + lane group of child c, per function; rows = z1 features), fold_bias [node][2 x 16]: z1's ONE bias vector.
    std::vector<float> fold_frag, fold_bias;
    // ... with its four one-row k-steps packed (FusedPlan::fold01_pack; layer-0 nodes of 13 outputs: feature 12 sits alone in register 3).  The
    // k-steps of register 3 are gone from fold_frag (zeros) and ONE k-step carries their four k-rows, k = lane group: 0 = child 0's feature 12,
    // 1 = child 1's, 2 = |child 0's|^p, 3 = |child 1's|^p.
    // fold_last [node][tile: 0 = 16x16 form, 1 = 4x4 form][lane]: that k-step's A fragments (lane (g, i): row (child g % 2, function g / 2,
    // feature 12) of F_c at the tile's row i) — stage 1.
    // fold_a1 [node][lane][4], fold_b1 [node][16]: STAGE 0's first-affine block and first bias with feature 12 (tile row 3) repeated where the
    // packed k-step reads it — rows 3 and 11 of an even node, rows 7 and 15 of an odd node, whose row 3 is zero — so that the sum of the two
    // children's registers 3 holds (c0, c1, c0, c1) by lane group, each value plus an exact +0.0.  Those rows are padding in afrag / bias.
    std::vector<float> fold_last, fold_a1, fold_b1;
    // Summed link (FusedOptions::pair; hoisted stages whose nodes all have exactly two children).  The layer below may then store ONE tile set
    // per node of this stage, (bias + child 0's tiles) + child 1's tiles, in place of its own two (k_stage_sum_pair); this stage reads it as a
    // hoisted stage of one child per node whose first bias adds nothing.  Empty where the stage has no pairs.
    std::vector<int32_t> pair_kids;    // int2 per node: its two children in FNode::kids order (first read; neither ascending nor adjacent)
    std::vector<int32_t> kb1tab_pre;   // int2 [node][mt1] = {node * mt1 + mt, 1}, and the eight spare entries every table carries
    std::vector<float> bias_pre;       // `bias` with the first mt1 x 16 floats of every node = -0.0f: (-0.0f) + x is x, bit for bit, for every x
};

struct FusedPlan {
    FusedOptions opt;
    int out_dim = 0;
    bool s0_transpose = false, fuse01 = false;
    bool fold01 = false;                // the front kernels run the link 0 -> 1 folded (stages[1].fold_frag / fold_bias); implies fuse01
    std::string fold01_note;            // why, or why not (stage 1's line of hg_flow_describe); empty where FusedOptions::fold01 is off
    bool fold01_pack = false;           // ... with the four one-row k-steps packed into one (stages[1].fold_last, stages[0].fold_a1 / fold_b1); implies fold01
    std::string fold01_pack_note;       // why, or why not (appended to stage 1's line); empty where FusedOptions::fold01_pack is off
    std::vector<HostStage> stages;
    std::vector<int32_t> col_base, col_of;
    int tail_begin = -1;          // first stage of the top-of-hierarchy launch (k_tail); -1: none
    int tail_act_blocks = 0, tail_e_blocks = 0;
    std::vector<SubRun> sub_runs;       // k_subtree runs (short batches)
    int max_nb = 0;
    int64_t padded_flops = 0;           // FLOPs per row this plan issues (hoisted links included)
    int64_t fold01_flops = 0;           // ... what folding the link 0 -> 1 changed in it (<= 0)
    int64_t padded_flops_given = 0;     // ... the plan of the same flow with no link hoisted issues: what hg_info reports (== padded_flops where nothing was hoisted)

    // The per-call choices: pure functions of the plan and the batch's 16-row tiles.
    // Three fused layers pay off from ~1400 rows on (call times against N, profiles/r03_call_times.txt: 16 waves per workgroup walk
    // the three layers' latencies one after the other — 23 us however small the batch, against 6 us for a k_stage_splitm launch of
    // the 4-node layer plus 13 us for the two layers above it); below that the launch starts one layer later.  Same bits either way.
    // A sub-tree launch pays while all its workgroups (sub-trees x batch tiles, each pulling its sub-tree's weights through ONE compute
    // unit's L1) are resident at once, one per CU: measured on U11L-128 (profiles/r05_subtree_call_times.txt) 8 sub-trees gain up to 512
    // rows = 256 workgroups and lose from 728; 32 sub-trees gain up to 44 rows and lose from 130.
    bool sub_run_pays(const SubRun& r, int n_tiles) const;
    // the set of runs a call of n_tiles uses: more layers inside usable runs first, then more sub-trees in the smallest of them
    int pick_sub_set(int n_tiles) const;
    int tail_start(int n_tiles) const;
};

// nullptr (and a reason) when the flow does not have the regular structure the fused MFMA kernels need.
std::unique_ptr<const FusedPlan> build_fused_plan(const TNode& root, const FusedOptions& opt, std::string* why_not);

}  // namespace fused
}  // namespace hg
