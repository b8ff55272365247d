// k_stage_sum: k_stage (hg_fused.hip) for a layer whose first affine was hoisted into the layer below (HostStage::sum_in,
// hoist_first_affines in hg_fused_plan.cpp).  The children already multiplied by the folded matrix, so a node visit is
//     z[mt] = ((bias[mt] + tile mt of child 0) + tile mt of child 1) + ...       (K-block-table order: child-major, entry i -> tile i % MT1)
// then the expansion and the second affine exactly as in k_stage (node_tail).  Every kernel family that runs such a layer
// (k_stage_splitm, the layer routine of k_tail / k_subtree) adds in this order, so a row has the same bits whichever one ran it.
//
// Same sweep as k_stage: a workgroup keeps the second-affine fragments of `nodes_per_group` nodes in LDS (32 KiB per 60 -> 60 node, half
// of what the layer needed with its first affine) and walks its share of the batch's tile groups.  The source blocks form one stream
// across children, nodes and tile groups: child 0's tiles of the NEXT visit are requested before the current node's second affine,
// whose MFMAs (no global loads of their own) cover the round trip; the further children follow as soon as child 0's registers are
// free again — MT1 x T blocks in flight at a time, which is what fits beside the second affine's accumulators.
#include <hip/hip_runtime.h>

#include "hg_fused_dev.hpp"

namespace hg {
namespace fused {

namespace {

template <int MT1, int MT2, int T, bool FS>
__global__ void __launch_bounds__(512, 4) k_stage_sum(StageParams P) {
    extern __shared__ __attribute__((aligned(16))) f32x4 smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, nw = nthr >> 6, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware decode, part-major within an XCD: as in k_stage
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
    const int cpx = (P.n_chunks + 7) >> 3;
    const int chunk = xcd + 8 * (kq % cpx), part = kq / cpx;
    if (chunk >= P.n_chunks) return;
    const int n_begin = chunk * P.nodes_per_wg;
    const int n_end = min(n_begin + P.nodes_per_wg, P.n_nodes);
    const int npg = P.nodes_per_group;
    float* sb = (float*)(smem + (size_t)npg * P.node_blocks * 64);
    int2* stab = (int2*)(sb + npg * P.bias_floats);
    const int n_kids = P.n_kids;

    for (int g0 = n_begin; g0 < n_end; g0 += npg) {
        const int gn = min(npg, n_end - g0);
        __syncthreads();
        {   // cooperative copy of the group's weights, 8 x 16 B in flight per thread
            const f32x4* src = P.afrag + (size_t)g0 * P.node_blocks * 64;
            const int nvec = gn * P.node_blocks * 64;
            int i = tid;
            for (; i + 7 * nthr < nvec; i += 8 * nthr) {
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = src[i + u * nthr];
#pragma unroll
                for (int u = 0; u < 8; ++u) smem[i + u * nthr] = v[u];
            }
            for (; i < nvec; i += nthr) smem[i] = src[i];
            const float* bsrc = P.bias + (size_t)g0 * P.bias_floats;
            for (int k = tid; k < gn * P.bias_floats; k += nthr) sb[k] = bsrc[k];
            const int2* tsrc = P.kb1tab + (size_t)g0 * P.kb1;
            for (int k = tid; k < gn * P.kb1; k += nthr) stab[k] = tsrc[k];
        }
        __syncthreads();
        int tile[T];
        uint32_t trow[T], trow_nx[T];   // first block of the tile's row in the input activation
#pragma unroll
        for (int t = 0; t < T; ++t) tile[t] = (part * nw + wave) * T + t;
        if (tile[0] >= P.n_tiles) continue;
#pragma unroll
        for (int t = 0; t < T; ++t) trow[t] = (uint32_t)(tile[t] < P.n_tiles ? tile[t] : tile[0]) * (uint32_t)P.nb_in;
        f32x4 bq[MT1][T];      // child 0's tiles of the visit about to start
#pragma unroll
        for (int mt = 0; mt < MT1; ++mt) {
            const int sb0 = __builtin_amdgcn_readfirstlane(stab[mt].x);
#pragma unroll
            for (int t = 0; t < T; ++t) bq[mt][t] = P.in[(size_t)(trow[t] + (uint32_t)sb0) * 64 + lane];
        }
        for (int grp = part; grp < P.tile_groups; grp += P.tile_parts) {
            const int tn0 = ((grp + P.tile_parts) * nw + wave) * T;
            const bool has_next = grp + P.tile_parts < P.tile_groups && tn0 < P.n_tiles;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int tn = tn0 + t;
                trow_nx[t] = has_next ? (uint32_t)(tn < P.n_tiles ? tn : tn0) * (uint32_t)P.nb_in : trow[t];
            }
            for (int ln = 0; ln < gn; ++ln) {
                const f32x4* wA2 = smem + (size_t)ln * P.node_blocks * 64 + lane;
                const float* b1 = sb + ln * P.bias_floats;
                const int2* kt = stab + ln * P.kb1;
                f32x4 z[MT1][T];
#pragma unroll
                for (int mt = 0; mt < MT1; ++mt) {
                    const f32x4 bb = *(const f32x4*)(b1 + mt * 16 + g * 4);
#pragma unroll
                    for (int t = 0; t < T; ++t) z[mt][t] = bb + bq[mt][t];
                }
                for (int c = 1; c < n_kids; ++c) {
                    if (__builtin_amdgcn_readfirstlane(kt[c * MT1].y) == 0) break;      // a node with fewer children: padding comes last
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) {
                        const int sbc = __builtin_amdgcn_readfirstlane(kt[c * MT1 + mt].x);
#pragma unroll
                        for (int t = 0; t < T; ++t) bq[mt][t] = P.in[(size_t)(trow[t] + (uint32_t)sbc) * 64 + lane];
                    }
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt)
#pragma unroll
                        for (int t = 0; t < T; ++t) z[mt][t] += bq[mt][t];
                }
                {   // next visit's first child: next node of this group on the same tiles, or the group's first node on the next tiles
                    const bool in_group = ln + 1 < gn;
                    const int2* ktn = in_group ? kt + P.kb1 : stab;
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) {
                        const int sbn = __builtin_amdgcn_readfirstlane(ktn[mt].x);
#pragma unroll
                        for (int t = 0; t < T; ++t) bq[mt][t] = P.in[(size_t)((in_group ? trow[t] : trow_nx[t]) + (uint32_t)sbn) * 64 + lane];
                    }
                }
                node_tail<MT1, MT2, T, false, FS, FS && T == 2>(P, wA2, b1 + MT1 * 16, g0 + ln, z, tile, lane);
            }
            if (!has_next) break;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                tile[t] = tn0 + t;
                trow[t] = trow_nx[t];
            }
        }
    }
}

template <int MT1, int MT2>
StageFn pick_t(int T) {
    if (T == 2) return k_stage_sum<MT1, MT2, 2, false>;
    return k_stage_sum<MT1, MT2, 1, false>;
}
template <int MT1>
StageFn pick_m2(int mt2, int T) {
    switch (mt2) {
        case 1: return pick_t<MT1, 1>(T);
        case 2: return pick_t<MT1, 2>(T);
        case 3: return pick_t<MT1, 3>(T);
        default: return pick_t<MT1, 4>(T);
    }
}

}  // namespace

// fs: the expansion is (identity, |x|^p), known at compile time — instantiated for the 60 -> 60 nodes of the preset networks' middle layers
StageFn pick_stage_sum(int mt1, int mt2, int T, bool fs) {
    if (fs && mt1 == 4 && mt2 == 4) return T == 2 ? (StageFn)k_stage_sum<4, 4, 2, true> : (StageFn)k_stage_sum<4, 4, 1, true>;
    switch (mt1) {
        case 1: return pick_m2<1>(mt2, T);
        case 2: return pick_m2<2>(mt2, T);
        case 3: return pick_m2<3>(mt2, T);
        default: return pick_m2<4>(mt2, T);
    }
}

}  // namespace fused
}  // namespace hg
