// The planner's normal form of a flow (internal to hg_fused_plan.cpp and to host-only drivers that test its passes): one FStage per
// network layer — the Switchboard in front of it as a column map, every node as [first affine][expansion][second affine] with
// adjacent affines folded in float64 — and the passes that run on that list before the Planner packs it.
#pragma once
#include <string>
#include <vector>

#include "hg_fused_plan.hpp"

namespace hg {
namespace fused {

struct Aff {  // y = (x - a) W + b
    int in = 0, out = 0;
    std::vector<double> a, W, b;
};

struct FNode {
    int in_off = 0, in_dim = 0, out_dim = 0;
    Aff A1, A2;
    bool has_exp = false;
    std::vector<ExpFunc> funcs;
    bool has_prod = false;              // cross-column products in the expansion -> k_stage_prod
    bool has_clip = false;              // CutoffNode between expansion and second affine
    double clip_lo = 0, clip_hi = 0;
    // iGSFA node: x0 = x - mean; s = sfa(expand(x0)) (scale folded in);
    // r = x0 - lr(s); q = pca(r); y = [s, q]
    bool is_ig = false, ig_has_lr = false;
    bool was_ig = false;                // an iGSFA node that fold_igsfa turned into an ordinary one
    int ig_k = 0;
    std::vector<double> ig_mean;
    Aff ig_sfa, ig_lr, ig_pca;
    // hoisted link (hoist_first_affines): this node's first affine was folded into its children's second affines.  z is the sum of
    // the children's output tiles plus sum_bias; A1 keeps its dimensions (in, out) and nothing else.
    std::vector<int> kids;              // nodes of the stage below, in the order this node's input first reads them
    std::vector<double> sum_bias;       // [A1.out]
};

struct FStage {
    std::vector<int32_t> conn;  // stage input column -> column of the previous frame (or of x)
    std::vector<FNode> nodes;
    int out_w = 0;
    bool sum_in = false;        // every node of the stage takes its z from its children's tiles (FNode::kids)
};

bool build_stages(const TNode& root, std::vector<FStage>& stages, std::string& why, const FusedOptions& opt);

// Folds each parent's first affine into its children's second affines wherever the link between two consecutive stages allows it
// (DESIGN.md §3.1 "Hoisted links"); returns the parents' stage indices.  Float64 throughout.
std::vector<int> hoist_first_affines(std::vector<FStage>& stages, const FusedOptions& opt);

}  // namespace fused
}  // namespace hg
