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

// ---- k_stage_sum_pair: the same layer storing ONE tile set per node of the layer above (summed link) ----
// Where the layer above is hoisted as well and each of its nodes has exactly two children (HostStage::pair_kids), that layer computes
// z = (bias_p + y of child 0) + y of child 1 from two stored tile sets.  Here one wave runs both children of a parent on its own batch tiles and
// stores that sum: half the bytes written, half read again, and no add left above.  Each y is the chain node_tail runs (the same MFMAs in the
// same order per accumulator, starting from the child's own second bias), the additions are the parent's, in its order, on the same floats
// (bias_p comes from the parent stage's own bias array): the same bits.  No workgroup depends on another.
// Shape: 4 x 4 tiles with the compile-time expansion, the preset networks' 60 -> 60 layers; everything else stays on k_stage_sum.
// A node group is a list of pairs; the two children's fragments are copied as two ranges (siblings are not adjacent nodes).

// z of one node from the prefetched tiles of its first child (bq) and those of its further children, as in k_stage_sum; bq leaves with the first
// child's tiles of the NEXT visit (table ktn, rows trow_n).
template <int T>
__device__ __forceinline__ void pair_z(const StageParams& P, const float* b1, const int2* kt, const int2* ktn, const uint32_t (&trow)[T],
                                       const uint32_t (&trow_n)[T], int n_kids, int lane, int g, f32x4 (&bq)[4][T], f32x4 (&z)[4][T]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const f32x4 bb = *(const f32x4*)(b1 + mt * 16 + g * 4);
#pragma unroll
        for (int t = 0; t < T; ++t) z[mt][t] = bb + bq[mt][t];
    }
    for (int c = 1; c < n_kids; ++c) {
        if (__builtin_amdgcn_readfirstlane(kt[c * 4].y) == 0) break;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int sbc = __builtin_amdgcn_readfirstlane(kt[c * 4 + mt].x);
#pragma unroll
            for (int t = 0; t < T; ++t) bq[mt][t] = P.in[(size_t)(trow[t] + (uint32_t)sbc) * 64 + lane];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int t = 0; t < T; ++t) z[mt][t] += bq[mt][t];
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int sbn = __builtin_amdgcn_readfirstlane(ktn[mt].x);
#pragma unroll
        for (int t = 0; t < T; ++t) bq[mt][t] = P.in[(size_t)(trow_n[t] + (uint32_t)sbn) * 64 + lane];
    }
}

// node_tail's compile-time-expansion second affine without its store: y = b2 + A2 (z, |z|^p).  T = 2: the m-tile-outer loop (LEAN);
// T = 1: k-step outer with the power block's fragments requested ahead of the power — the forms k_stage_sum<4, 4, T, true> runs.
template <int T, typename WP>
__device__ __forceinline__ void pair_affine2(const StageParams& P, WP wA2, const float* b2, int g, const f32x4 (&z)[4][T], f32x4 (&y)[4][T]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const f32x4 bb = *(const f32x4*)(b2 + mt * 16 + g * 4);
#pragma unroll
        for (int t = 0; t < T; ++t) y[mt][t] = bb;
    }
    const float ex1 = P.expo[1];
#pragma unroll
    for (int mt1 = 0; mt1 < 4; ++mt1) {
        const uint32_t nkp = P.nk2p[mt1];
        const int nk0 = nkp & 15, nk1 = (nkp >> 4) & 15;
        if constexpr (T == 2) {
            gemm_block<4, T>(wA2 + (mt1 * 2) * 4 * 64, z[mt1], y, nk0);
            f32x4 e[T];
#pragma unroll
            for (int t = 0; t < T; ++t) e[t] = pow_abs4(z[mt1][t], ex1);
            gemm_block<4, T>(wA2 + (mt1 * 2 + 1) * 4 * 64, e, y, nk1);
        } else {
            gemm_block<4, T, true>(wA2 + (mt1 * 2) * 4 * 64, z[mt1], y, nk0);
            f32x4 ap[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) ap[mt] = (wA2 + (mt1 * 2 + 1) * 4 * 64)[mt * 64];
            f32x4 e[T];
#pragma unroll
            for (int t = 0; t < T; ++t) e[t] = pow_abs4(z[mt1][t], ex1);
            gemm_block_regs<4, T>(ap, e, y, nk1);
        }
    }
}

template <int T>
__global__ void __launch_bounds__(512, 4) k_stage_sum_pair(StageParams P) {
    extern __shared__ __attribute__((aligned(16))) f32x4 smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, nw = nthr >> 6, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware decode, part-major within an XCD: as in k_stage (a chunk is a group of pairs)
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
    const int cpx = (P.n_chunks + 7) >> 3;
    const int chunk = xcd + 8 * (kq % cpx), part = kq / cpx;
    if (chunk >= P.n_chunks) return;
    const int ppg = P.nodes_per_group;      // pairs of a group; slot 2 j + k of the LDS image = child k of the group's pair j
    const int p_begin = chunk * ppg;
    const int gn = min(ppg, P.n_pairs - p_begin);
    const int nvn = P.node_blocks * 64, bf = P.bias_floats, kb1 = P.kb1;
    float* sb = (float*)(smem + (size_t)2 * ppg * nvn);
    float* spb = sb + 2 * ppg * bf;          // the parents' first bias: 4 x 16 floats per pair
    int2* stab = (int2*)(spb + ppg * 64);
    const int n_kids = P.n_kids;

    for (int s = 0; s < 2 * gn; ++s) {      // cooperative copy, node by node, 8 x 16 B in flight per thread
        const int2 pk = P.pair_kids[p_begin + (s >> 1)];
        const int node = __builtin_amdgcn_readfirstlane((s & 1) ? pk.y : pk.x);
        const f32x4* src = P.afrag + (size_t)node * nvn;
        f32x4* dst = smem + (size_t)s * nvn;
        int i = tid;
        for (; i + 7 * nthr < nvn; i += 8 * nthr) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[i + u * nthr];
#pragma unroll
            for (int u = 0; u < 8; ++u) dst[i + u * nthr] = v[u];
        }
        for (; i < nvn; i += nthr) dst[i] = src[i];
        const float* bsrc = P.bias + (size_t)node * bf;
        for (int k = tid; k < bf; k += nthr) sb[s * bf + k] = bsrc[k];
        const int2* tsrc = P.kb1tab + (size_t)node * kb1;
        for (int k = tid; k < kb1; k += nthr) stab[s * kb1 + k] = tsrc[k];
    }
    for (int k = tid; k < gn * 64; k += nthr) spb[k] = P.pair_bias[(size_t)(p_begin + (k >> 6)) * P.pair_bias_floats + (k & 63)];
    __syncthreads();

    int tile[T];
    uint32_t trow[T], trow_nx[T];   // first block of the tile's row in the input activation
#pragma unroll
    for (int t = 0; t < T; ++t) tile[t] = (part * nw + wave) * T + t;
    if (tile[0] >= P.n_tiles) return;
#pragma unroll
    for (int t = 0; t < T; ++t) trow[t] = (uint32_t)(tile[t] < P.n_tiles ? tile[t] : tile[0]) * (uint32_t)P.nb_in;
    f32x4 bq[4][T];      // the first child's tiles of the visit about to start
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
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
        for (int lp = 0; lp < gn; ++lp) {      // a visit: (parent, tile set)
            const int s0 = 2 * lp, s1 = 2 * lp + 1;
            f32x4 s[4][T];
            {   // child 0: s = bias_p + y0
                f32x4 z[4][T], y[4][T];
                pair_z<T>(P, sb + s0 * bf, stab + s0 * kb1, stab + s1 * kb1, trow, trow, n_kids, lane, g, bq, z);
                pair_affine2<T>(P, smem + (size_t)s0 * nvn + lane, sb + s0 * bf + 64, g, z, y);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const f32x4 bb = *(const f32x4*)(spb + lp * 64 + mt * 16 + g * 4);
#pragma unroll
                    for (int t = 0; t < T; ++t) s[mt][t] = bb + y[mt][t];
                }
            }
            {   // child 1: store s + y1 as the parent's tiles
                f32x4 z[4][T], y[4][T];
                const bool in_group = lp + 1 < gn;      // next visit: the group's next pair on the same tiles, or its first pair on the next tiles
                pair_z<T>(P, sb + s1 * bf, stab + s1 * kb1, in_group ? stab + (s1 + 1) * kb1 : stab, trow, in_group ? trow : trow_nx, n_kids, lane, g, bq, z);
                pair_affine2<T>(P, smem + (size_t)s1 * nvn + lane, sb + s1 * bf + 64, g, z, y);
                const int out_blk = (p_begin + lp) * 4;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int t = 0; t < T; ++t)
                        if (tile[t] < P.n_tiles) P.out[((size_t)tile[t] * P.nb_out + out_blk + mt) * 64 + lane] = s[mt][t] + y[mt][t];
            }
        }
        if (!has_next) break;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            tile[t] = tn0 + t;
            trow[t] = trow_nx[t];
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

StageFn pick_stage_sum_pair(int T) {
#ifdef HG_PAIR_T2      // (resource study only: two tiles per wave spill at 128 registers — DESIGN.md §6.10)
    if (T == 2) return (StageFn)k_stage_sum_pair<2>;
#endif
    return T == 1 ? (StageFn)k_stage_sum_pair<1> : nullptr;
}

}  // namespace fused
}  // namespace hg
