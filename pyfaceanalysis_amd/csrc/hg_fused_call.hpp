// The call plan: what ONE call of n_tiles batch tiles launches from a fused plan — which stage runs on which route and in what
// shape.  Pure functions of (plan, tiles, the caller's rows, occupancy): host only like the plan itself (no HIP runtime, no device
// pointers), so a plain g++ driver reaches every rule (tests/hoist_plan_driver.cpp --call).  The executor (hg_fused.hip) carries the
// steps out: it fills the kernel parameters, maps a step's shape to its kernel (pick_* stay with the kernels), asks the occupancy
// and launches.  Nothing here is cached: a call plan is recomputed per call, into a step list its lane keeps.
#pragma once
#include <vector>

#include "hg_fused_plan.hpp"

namespace hg {
namespace fused {

// ---- constants the rules read (the kernels include them from here) ---------------------------------------------------------------
constexpr int kWeightLdsKiB = 64;       // target size of a node group's weights in LDS (k_stage)
constexpr int kProdLdsBytes = 52 * 1024;      // k_stage_prod: z images + product table + node group (three workgroups per CU)
constexpr int kPairLdsCapKiB = 144;     // k_stage_sum_pair: most KiB of fragments a pair group holds, whatever HIGSFA_SUM_LDS says
constexpr int kPairTiles = 1;           // batch tiles per wave of k_stage_sum_pair (two do not fit 128 registers)
// k_stage01p: two LDS tiles (one barrier per tile group) or one (two barriers, half the LDS).  With the packed
// tile layout (128 + 4 words per row) both fit three workgroups per CU and measure the same (152-154 us).
constexpr bool kDoubleBuffer01 = true;
// Tiles per pass of the instantiation pick_stage01p returns (LDS and the group count are sized with it): the
// compile-time-expansion form takes ONE tile per pass at four waves per SIMD (124 VGPRs; 146 us against 153 with two
// tiles at three waves), the generic form two tiles at three waves (168 VGPRs).
constexpr int stage01p_tiles(bool /*rem4*/, bool fspec) { return fspec ? 1 : 2; }

// The switches the executor plans under: the environment's, and the four that are the executor's own.
FusedOptions executor_options();

// (identity, |x|^p) expansion at compile time — the FS / FSPEC instantiations — unless HIGSFA_NO_FSPEC
bool fs_expansion(const HostStage& s, const FusedOptions& opt);

// ---- routes ------------------------------------------------------------------------------------------------------------------
// One value per thing a call can launch for a stage.  (The unpack pass follows from "no Top step ran".)
enum class Route : uint8_t {
    Gather,       // kind 1: the caller's rows -> fragment order (k_im2frag)
    Front01d,     // layers 0 and 1 in one launch, every wave on its own (k_stage01d)
    Front01p,     // ... LDS-staged (k_stage01p)
    Front0p,      // layer 0 alone, persistent (k_stage0p)
    Front0,       // layer 0 alone (k_stage0)
    IgSweep,      // iGSFA layer: k_igfold (folded) / k_igsfa
    IgSplit,      // the folded top of an iGSFA hierarchy in small workgroups (k_igfold_split)
    ProdSweep,    // table-driven expansion (k_stage_prod)
    Splitm,       // one node and T tiles per small workgroup (k_stage_splitm)
    Sweep,        // node groups in LDS swept over the batch (k_stage / k_stage_sum)
    SumPair,      // ... storing its link to the next stage summed per parent (k_stage_sum_pair)
    Subtree,      // a run of layers as independent sub-trees (k_subtree)
    Top,          // this stage and everything above it, into the caller's rows (k_tail)
};
const char* route_name(Route r);

// The three facts the front rule (and the row gather) reads from the caller's rows
struct FrontInput {
    bool vec4_ok = true;      // pointer and pitch allow 16-byte loads (4-byte for uint8); the stage's own vec_ok is the rule's
    int x_dtype = HG_F32;
    int64_t ldx = 0;
};

// What identifies the kernel instantiation and sizes the launch — everything but tile_parts, which needs the occupancy of the kernel
// the shape maps to.  Fields a route does not use stay zero.
struct CallShape {
    int nw = 0, T = 0;            // waves that take tiles x tiles per wave (front pair: T = tiles per pass)
    int per_group = 0;            // nodes (SumPair: pairs) per group
    int n_groups = 0;             // node groups: the launch's chunks (front: layer 0's chunks)
    int tile_groups = 0;
    int threads = 0;
    size_t lds = 0;               // dynamic LDS bytes
    int kbf = 0;                  // Sweep: K-blocks fetched a whole visit ahead
    bool fs = false;              // Sweep, IgSweep: compile-time expansion
    bool rem4 = false, fspec = false, direct = false, wgq = false, fold = false, pack = false, scalar = false;      // front
    bool vec4 = false;            // Gather, front: 16-byte loads of the caller's rows
    bool pair_chunks = false;     // Sweep: chunks 2c, 2c + 1 on one XCD (StageParams::pair_chunks)
    int kb1 = 0, n_kids = 0;      // Sweep, SumPair: the first affine as THIS call reads it (a summed input: one child per node)
    int queue_ctrs = 0;           // front pair: counters of its tile queue
    int64_t blocks = 0;           // the grid of a launch without tile_parts; the others: step_blocks()
};

struct CallStep {
    Route route = Route::Sweep;
    int stage = 0, covered = 1;   // first stage and how many the launch covers
    bool in_summed = false;       // reads ONE tile set per node: the stage below stored the link summed
    int sub_run = -1;             // Subtree: index into FusedPlan::sub_runs
    CallShape sh;
};

// The call's steps in order; `steps` is cleared first and keeps its capacity (a lane's list allocates once).
void plan_call(const FusedPlan& plan, int n_tiles, const FrontInput& fi, std::vector<CallStep>& steps);

// waves x tiles per workgroup of a node-group sweep: the first candidate that still gives every CU a workgroup (>= 256 over
// n_groups node groups); never fewer than 4 waves to copy a node's weights unless the batch is tiny
struct WavesTiles {
    int nw, T;
};
WavesTiles stage_sweep_shape(int n_tiles, int n_groups);      // k_stage: 8x2, 8x1, 4x2, 4x1 (k_stage_prod: 8x2, 4x2, 4x1 over single nodes)

// ---- the second phase: occupancy -> tile_parts -> grid ---------------------------------------------------------------------------
// Persistent sweep: each workgroup copies its node group's weights once and walks tile groups part, part + tile_parts, ...
// cost(parts) = rounds of resident workgroups (occ per CU; node groups padded to 8) x (weight copy + tile iterations per workgroup)
int sweep_tile_parts(int n_groups, int tile_groups, int occ);
// one resident round of workgroups over the chunks: min(groups, 256 occ / chunks), at least 1 (iGSFA, front pair, k_stage0p)
int spread_tile_parts(int groups, int chunks, int occ);
// by route (1 where the launch has no tile_parts)
int step_tile_parts(const CallStep& st, int occ);
// the grid; refuses a batch whose grid does not fit 31 bits where the launch can grow that far
int64_t step_blocks(const CallStep& st, int tile_parts);

// The step's HIGSFA_DEBUG line (no newline); returns buf.  The executor prints it, the plan driver prints the same text.
const char* format_step(const FusedPlan& plan, const CallStep& st, int occ, int tile_parts, char* buf, size_t cap);

}  // namespace fused
}  // namespace hg
