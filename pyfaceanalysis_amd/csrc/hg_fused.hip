// Fused executor: one kernel per network layer ("stage" = Switchboard gather + per-node
// [affine -> element-wise expansion -> affine]), fp32 MFMA (v_mfma_f32_16x16x4_f32), gfx950.
//
// Data layout ("fragment order").  A batch tile is 16 sub-images.  Every node output is cut
// into feature tiles of 16; one (batch tile, feature tile) pair is a 1 KiB block
//       block[lane 0..63][reg 0..3]   lane = 16*g + j   (j = sub-image in tile, g = 0..3)
// holding feature q = 4*reg + g of the tile for sub-image j.  This is exactly the C/D register
// image of v_mfma_f32_16x16x4_f32 (col = lane&15, row = 4*(lane>>4) + reg) under the row
// assignment row(q) = 4*(q&3) + (q>>2), so
//   * a producer stores each accumulator as one coalesced 16 B/lane (1 KiB/wave) write,
//   * a consumer loads a block with one 16 B/lane read and has FOUR k-steps of the MFMA B
//     operand in registers (k-step r: lane group g supplies feature 4r+g) — no shuffles, no LDS,
//   * inside a node the first affine's accumulators ARE the B operand of the second affine;
//     the expansion (|x|^0.8, ...) is applied to them in registers.
// The K order of every contraction is therefore permuted; the planner (hg_fused_plan.cpp, host only) permutes the weight
// matrices to match (A fragments, [k-block][m-tile][lane][4]) and folds Switchboards into the
// K-block lists, so a gather costs nothing at run time.  Stage 0 reads the caller's row-major
// sub-image matrix: coalesced row segments go through an LDS tile and the 4x4 (or any) receptive
// field is picked out of LDS by per-lane offsets.
//
// Reference semantics restated: SURVEY.md §8a rows a3-a7 (Switchboard, Layer, PCANode,
// GeneralExpansionNode, SFANode) behind the call FaceDetectUpdated.py:699.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <sstream>
#include <tuple>

#include "hg_fused_dev.hpp"

namespace hg {

namespace {

using namespace fused;

// Stages > 0.  A workgroup of NW waves owns NW*T batch tiles and walks a range of nodes; the
// weights of `nodes_per_group` nodes at a time are copied once into LDS and shared by all waves
// (A fragments by ds_read_b128); activation fragments come straight from HBM/L2 with one 16 B/lane
// coalesced load per K-block and tile, prefetched one K-block ahead.
// REM: the last tile of both affines holds <= 4 real rows and its A fragments are stored in 4x4 form
// (hg_fused_dev.hpp, "Remainder tiles").
// KBF > 0 (== P.kb1, checked at launch): all K-blocks of a node visit are fetched at once, one whole visit ahead — issued
// before the second half of the previous node, whose MFMAs (no global loads of their own) cover the L2 / HBM round trip.
// For small nodes (layer 2: four blocks of <= 4 k-steps) the one-block-ahead stream leaves each wave waiting ~1.5k cycles
// per block (in-kernel stamps: GEMM 1 took 6x its MFMA time); costs KBF * T * 4 registers.
#ifndef HG_A_PINGPONG
#define HG_A_PINGPONG 1      // (A/B switch: HIGSFA_CXXFLAGS=-DHG_A_PINGPONG=0)
#endif
#ifdef HIGSFA_DIAG
#define HG_HOT(blk) ((P.whatif & 1) ? ((blk) & 1) : (blk))      // timing experiment: all input blocks from the first two of the tile row
#else
#define HG_HOT(blk) (blk)
#endif
// PK >= 0 (only with KBF): K-block PK of every node is a slot-major packed block of the stage below (StageParams::pack_soa): its
// two slots are loaded with two 4-byte loads per lane at a position of the code that is fixed at compile time — a run-time test
// per K-block in the streaming loops below cost layers 3-7, which never see such a block, 5 % (profiles/r05_packed_stores.txt).
template <int MT1, int MT2, int T, bool STAMP = false, bool REM = false, int KBF = 0, bool FS = false, int PK = -1>
__global__ void __launch_bounds__(512, 4) k_stage(StageParams P) {
    extern __shared__ __attribute__((aligned(16))) f32x4 smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, nw = nthr >> 6, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps tile/row bookkeeping in SGPRs
    // XCD-aware decode: blocks b, b+8, ... share an XCD (and its L2); give each XCD whole node
    // chunks so a chunk's weights are fetched into one L2 only.
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
    // part-major within an XCD: the first workgroups dispatched — the oldest on their CUs, which the SIMD arbiter favours — are
    // part 0 of EVERY chunk, so every node's tiles are served by fast and slow workgroups alike (chunk-major: +0.4 % per step)
    const int cpx = (P.n_chunks + 7) >> 3;
    // pair_chunks: chunks 2c and 2c + 1 hold the four siblings of one lane-major packed output block; on ONE XCD, in the same part,
    // their partial-line stores meet in that XCD's L2 before the line is written back (otherwise in two L2s: never)
    const int jq = kq % cpx;
    const int chunk = P.pair_chunks ? (((xcd + 8 * (jq >> 1)) << 1) | (jq & 1)) : xcd + 8 * jq, part = kq / cpx;
    if (chunk >= P.n_chunks) return;
    const int n_begin = chunk * P.nodes_per_wg;
    const int n_end = min(n_begin + P.nodes_per_wg, P.n_nodes);
    const int npg = P.nodes_per_group;
    float* sb = (float*)(smem + (size_t)npg * P.node_blocks * 64);
    int2* stab = (int2*)(sb + npg * P.bias_floats);
    // (Round 5: the lane-group sums of the 4x4-form tiles through LDS — rem4_total_lds, which takes 1.9 us off the front kernel — make THIS kernel
    // slower, layer 2 91.8 -> 105.5 us: its LDS queue is full of A-fragment reads, and the reduction's reads wait behind them and its lgkmcnt(0)
    // for all of them.  The permlane form stays here.)

    unsigned long long t_copy = 0, t_g1 = 0, t_tail = 0, t_all0 = 0;
    int n_it = 0;
    unsigned long long rt0 = 0;
    if (STAMP) {
        t_all0 = stamp_now();
        rt0 = __builtin_amdgcn_s_memrealtime();
    }
    for (int g0 = n_begin; g0 < n_end; g0 += npg) {
        const int gn = min(npg, n_end - g0);
        unsigned long long tc0 = 0;
        if (STAMP) tc0 = stamp_now();
        __syncthreads();
        {   // cooperative copy of the group's weights, 8 x 16 B in flight per thread (an L2 round trip is
            // ~2k cycles here: the bytes in flight per CU set the copy rate)
            const f32x4* src = P.afrag + (size_t)g0 * P.node_blocks * 64;
#ifdef HIGSFA_DIAG
            // timing experiment (HIGSFA_WHATIF bit 2; wrong results): no weight copy at all — what hiding it could gain at most
            const int nvec = (P.whatif & 4) ? 0 : gn * P.node_blocks * 64;
#else
            const int nvec = gn * P.node_blocks * 64;
#endif
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
        // The workgroup keeps this node group's weights in LDS and sweeps its share of the batch:
        // tile groups part, part + tile_parts, ...  (no barrier inside: waves run free).  The
        // activation fragments form ONE prefetch stream across K-blocks, nodes and tile groups:
        // while block i is multiplied, block i+1 — possibly the first block of the next node or of
        // the next tile group — is already in flight, so no visit starts with an exposed load.
        if (STAMP) t_copy += stamp_now() - tc0;
        int tile[T];
        uint32_t trow[T], trow_nx[T];   // first block of the tile's row in the input activation
#pragma unroll
        for (int t = 0; t < T; ++t) tile[t] = (part * nw + wave) * T + t;
        if (tile[0] >= P.n_tiles) continue;
#pragma unroll
        for (int t = 0; t < T; ++t) trow[t] = (uint32_t)(tile[t] < P.n_tiles ? tile[t] : tile[0]) * (uint32_t)P.nb_in;
        // HG_VISIT_WAITS, packed remainder output: pack_slot[node] is read a visit ahead, in front of the visit's block requests — read in
        // node_tail it is a load waited for between two runs of stores
        // (a stage that does not pack has no such table: it reads a word of its K-block table instead, unconditionally — a load behind a
        // branch makes the compiler drain the counter where the two paths meet)
        constexpr bool SLOT = REM && HG_VISIT_WAITS != 0;
        const int32_t* const slots = P.pack_base > 0 ? P.pack_slot : (const int32_t*)P.kb1tab;
        const int slot_on = P.pack_base > 0 ? 1 : 0;
        int slot_q = 0;
        if constexpr (SLOT) {
            slot_q = slots[g0 * slot_on];
            asm volatile("" : "+v"(slot_q));
        }
        if constexpr (KBF > 0) {
            f32x4 bq[KBF][T];
#pragma unroll
            for (int kbi = 0; kbi < KBF; ++kbi) {
                const int2 e0 = stab[kbi];
                const int sb0 = HG_HOT(__builtin_amdgcn_readfirstlane(e0.x));
                if (kbi == PK) load_kblock_soa<T, true>(P, trow, sb0, __builtin_amdgcn_readfirstlane(e0.y), lane, bq[kbi]);
                else {
#pragma unroll
                    for (int t = 0; t < T; ++t) bq[kbi][t] = P.in[(size_t)(trow[t] + sb0) * 64 + lane];
                }
            }
            if constexpr (HG_VISIT_WAITS != 0) arrived(bq);
            for (int grp = part; grp < P.tile_groups; grp += P.tile_parts) {
                const int tn0 = ((grp + P.tile_parts) * nw + wave) * T;
                const bool has_next = grp + P.tile_parts < P.tile_groups && tn0 < P.n_tiles;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const int tn = tn0 + t;
                    trow_nx[t] = has_next ? (uint32_t)(tn < P.n_tiles ? tn : tn0) * (uint32_t)P.nb_in : trow[t];
                }
                for (int ln = 0; ln < gn; ++ln) {
                    const f32x4* wA1 = smem + (size_t)ln * P.node_blocks * 64 + lane;
                    const f32x4* wA2 = wA1 + KBF * MT1 * 64;
                    const float* b1 = sb + ln * P.bias_floats;
                    const int2* kt = stab + ln * KBF;
                    f32x4 z[MT1][T];
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) {
                        f32x4 bb = *(const f32x4*)(b1 + mt * 16 + g * 4);
#pragma unroll
                        for (int t = 0; t < T; ++t) z[mt][t] = bb;
                    }
                    f32x4 d4[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) d4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    unsigned long long ts0 = 0, ts1 = 0;
                    if (STAMP) ts0 = stamp_now();
#pragma unroll
                    for (int kbi = 0; kbi < KBF; ++kbi) {
                        const int nkr = __builtin_amdgcn_readfirstlane(kt[kbi].y), nk = nkr & 255, r0 = (nkr >> 8) & 255;
                        if constexpr (REM) gemm_block_rem<MT1, T>(wA1 + kbi * MT1 * 64, bq[kbi], z, d4, nk, r0);
                        else gemm_block<MT1, T, FS>(wA1 + kbi * MT1 * 64, bq[kbi], z, nk, r0);
                    }
                    if constexpr (REM) {
#pragma unroll
                        for (int t = 0; t < T; ++t) add_rem4(z[MT1 - 1][t], d4[t]);
                    }
                    const int slot = __builtin_amdgcn_readfirstlane(slot_q);
                    {   // next visit's blocks: next node of this group on the same tiles, or the group's first node on the next tiles
                        const bool in_group = ln + 1 < gn;
                        const int2* ktn = in_group ? kt + KBF : stab;
                        if constexpr (SLOT) slot_q = slots[(in_group ? g0 + ln + 1 : g0) * slot_on];
                        uint32_t rw[T];
#pragma unroll
                        for (int t = 0; t < T; ++t) rw[t] = in_group ? trow[t] : trow_nx[t];
#pragma unroll
                        for (int kbi = 0; kbi < KBF; ++kbi) {
                            const int2 en = ktn[kbi];
                            const int sbn = HG_HOT(__builtin_amdgcn_readfirstlane(en.x));
                            if (kbi == PK) load_kblock_soa<T, true>(P, rw, sbn, __builtin_amdgcn_readfirstlane(en.y), lane, bq[kbi]);
                            else {
#pragma unroll
                                for (int t = 0; t < T; ++t) bq[kbi][t] = P.in[(size_t)(rw[t] + sbn) * 64 + lane];
                            }
                        }
                    }
                    if (STAMP) ts1 = stamp_now();
                    node_tail<MT1, MT2, T, REM, FS, false, HG_VISIT_WAITS != 0>(P, wA2, b1 + MT1 * 16, g0 + ln, z, tile, lane, nullptr, slot);
                    if (STAMP) {
                        unsigned long long ts2 = stamp_now();
                        t_g1 += ts1 - ts0;
                        t_tail += ts2 - ts1;
                        ++n_it;
                    }
                }
                if (!has_next) break;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    tile[t] = tn0 + t;
                    trow[t] = trow_nx[t];
                }
            }
            continue;
        }
        f32x4 bf[T], bfn[T];
        int nk;
        {
            const int2 kb = stab[0];
            const int sb0 = HG_HOT(__builtin_amdgcn_readfirstlane(kb.x));
            nk = __builtin_amdgcn_readfirstlane(kb.y);
            if constexpr (REM) load_kblock<T>(P, trow, sb0, nk, lane, bf);
            else {
#pragma unroll
                for (int t = 0; t < T; ++t) bf[t] = P.in[(size_t)(trow[t] + sb0) * 64 + lane];
            }
        }
        if constexpr (HG_VISIT_WAITS != 0) arrived(bf);
        for (int grp = part; grp < P.tile_groups; grp += P.tile_parts) {
            // rows of the tile group after this one (or this one again when it is the last)
            const int tn0 = ((grp + P.tile_parts) * nw + wave) * T;
            const bool has_next = grp + P.tile_parts < P.tile_groups && tn0 < P.n_tiles;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int tn = tn0 + t;
                trow_nx[t] = has_next ? (uint32_t)(tn < P.n_tiles ? tn : tn0) * (uint32_t)P.nb_in : trow[t];
            }
            for (int ln = 0; ln < gn; ++ln) {
                const f32x4* wA1 = smem + (size_t)ln * P.node_blocks * 64 + lane;
                const f32x4* wA2 = wA1 + P.kb1 * MT1 * 64;
                const float* b1 = sb + ln * P.bias_floats;
                const int2* kt = stab + ln * P.kb1;
                f32x4 z[MT1][T];
#pragma unroll
                for (int mt = 0; mt < MT1; ++mt) {
                    f32x4 bb = *(const f32x4*)(b1 + mt * 16 + g * 4);
#pragma unroll
                    for (int t = 0; t < T; ++t) z[mt][t] = bb;
                }
                f32x4 d4[T];      // REM: 4x4-form accumulators of the last z tile
#pragma unroll
                for (int t = 0; t < T; ++t) d4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                unsigned long long ts0 = 0, ts1 = 0;
                if (STAMP) ts0 = stamp_now();
                if constexpr (FS && !REM && HG_A_PINGPONG) {
                    // A fragments of block kbi + 1 are read from LDS BEFORE block kbi is multiplied, into the other of two register
                    // sets (the loop body twice, so that no set is ever copied): the MFMAs of a block wait for no LDS read
                    // (-0.6 % per step, profiles/r04_ab_lds_prefetch.txt).  Reading the K-block table entry two blocks ahead as
                    // well, so that the input prefetch does not wait for its LDS read either, measured 0.4 % SLOWER: not kept.
                    f32x4 a0[MT1], a1[MT1];
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) a0[mt] = wA1[mt * 64];
                    auto kstep = [&](int kbi, const f32x4 (&ac)[MT1], f32x4 (&an)[MT1]) {
                        const bool in_node = kbi + 1 < P.kb1;
                        const bool in_group = in_node || ln + 1 < gn;
                        const int2 kbn = in_node ? kt[kbi + 1] : (ln + 1 < gn ? kt[P.kb1] : stab[0]);
                        const int sbn = HG_HOT(__builtin_amdgcn_readfirstlane(kbn.x));
                        const int nkn = __builtin_amdgcn_readfirstlane(kbn.y);
#pragma unroll
                        for (int t = 0; t < T; ++t) bfn[t] = P.in[(size_t)((in_group ? trow[t] : trow_nx[t]) + sbn) * 64 + lane];
                        if (in_node) {
#pragma unroll
                            for (int mt = 0; mt < MT1; ++mt) an[mt] = wA1[((kbi + 1) * MT1 + mt) * 64];
                        }
                        gemm_block_regs<MT1, T>(ac, bf, z, nk & 255, (nk >> 8) & 255);
#pragma unroll
                        for (int t = 0; t < T; ++t) bf[t] = bfn[t];
                        nk = nkn;
                    };
                    if constexpr (HG_VISIT_WAITS != 0) {
                        // the visit's first block on its own: it was requested before the previous visit's stores, the blocks in the loop
                        // after them — one wait in a shared loop header would have to cover both, and retire the stores
                        kstep(0, a0, a1);
                        for (int kbi = 1; kbi < P.kb1; kbi += 2) {
                            kstep(kbi, a1, a0);
                            if (kbi + 1 < P.kb1) kstep(kbi + 1, a0, a1);
                        }
                    } else
                    for (int kbi = 0; kbi < P.kb1; kbi += 2) {
                        kstep(kbi, a0, a1);
                        if (kbi + 1 < P.kb1) kstep(kbi + 1, a1, a0);
                    }
                } else {
                    auto kstep1 = [&](int kbi) {
                        const bool in_node = kbi + 1 < P.kb1;
                        const bool in_group = in_node || ln + 1 < gn;
                        const int2 kbn = in_node ? kt[kbi + 1] : (ln + 1 < gn ? kt[P.kb1] : stab[0]);
                        const int sbn = HG_HOT(__builtin_amdgcn_readfirstlane(kbn.x));
                        const int nkn = __builtin_amdgcn_readfirstlane(kbn.y);
                        if constexpr (REM) {      // (only remainder-tile stages can have slot-major packed input: plan_slot_major)
                            uint32_t rw[T];
#pragma unroll
                            for (int t = 0; t < T; ++t) rw[t] = in_group ? trow[t] : trow_nx[t];
                            load_kblock<T>(P, rw, sbn, nkn, lane, bfn);
                        } else {
#pragma unroll
                            for (int t = 0; t < T; ++t) bfn[t] = P.in[(size_t)((in_group ? trow[t] : trow_nx[t]) + sbn) * 64 + lane];
                        }
                        if constexpr (REM) gemm_block_rem<MT1, T>(wA1 + kbi * MT1 * 64, bf, z, d4, nk & 255, (nk >> 8) & 255);
                        else gemm_block<MT1, T, FS>(wA1 + kbi * MT1 * 64, bf, z, nk & 255, (nk >> 8) & 255);
#pragma unroll
                        for (int t = 0; t < T; ++t) bf[t] = bfn[t];
                        nk = nkn;
                    };
                    if constexpr (HG_VISIT_WAITS != 0) kstep1(0);      // on its own, as above
                    for (int kbi = HG_VISIT_WAITS ? 1 : 0; kbi < P.kb1; ++kbi) kstep1(kbi);
                }
                if constexpr (REM) {
#pragma unroll
                    for (int t = 0; t < T; ++t) add_rem4(z[MT1 - 1][t], d4[t]);
                }
                if (STAMP) ts1 = stamp_now();
                const int slot = __builtin_amdgcn_readfirstlane(slot_q);
                if constexpr (SLOT) slot_q = slots[(ln + 1 < gn ? g0 + ln + 1 : g0) * slot_on];
                node_tail<MT1, MT2, T, REM, FS, false, HG_VISIT_WAITS != 0>(P, wA2, b1 + MT1 * 16, g0 + ln, z, tile, lane, nullptr, slot);
                if (STAMP) {
                    unsigned long long ts2 = stamp_now();
                    t_g1 += ts1 - ts0;
                    t_tail += ts2 - ts1;
                    ++n_it;
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
    if (STAMP && lane == 0 && P.stamps) {
        unsigned long long* o = P.stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
        const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
        o[5] = rt1 - rt0;
        o[6] = rt0;
        o[7] = rt1;
        o[0] = t_copy;
        o[1] = t_g1;
        o[2] = t_tail;
        o[3] = stamp_now() - t_all0;
        o[4] = (unsigned long long)n_it;
    }
}

// Stages > 0 with FEW nodes (the top of the hierarchy: 16, 8, 4, 2, 1 nodes).  There are not enough
// (node, tile) pairs to fill 1024 SIMDs with whole nodes, and copying 64 KiB of weights into LDS
// per workgroup is all latency.  Here a workgroup of max(MT1, MT2) waves shares ONE node and T
// tiles; wave w computes m-tile w of GEMM 1 and later m-tile w of GEMM 2, so every weight block is
// read by exactly one wave (straight from L2, all loads of a phase issued up front), and the
// expanded z tiles are exchanged through 2*MT1*T KiB of LDS.
template <int T, bool REM = false>
__global__ void __launch_bounds__(256) k_stage_splitm(StageParams P, int mt1n, int mt2n) {
    extern __shared__ __attribute__((aligned(16))) f32x4 smem[];
    constexpr int KB = 8;   // K-blocks loaded per batch
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int node = blockIdx.x % P.n_nodes, grp = blockIdx.x / P.n_nodes;
    int tile[T];
#pragma unroll
    for (int t = 0; t < T; ++t) tile[t] = grp * T + t;
    uint32_t trow[T];
#pragma unroll
    for (int t = 0; t < T; ++t) trow[t] = (uint32_t)(tile[t] < P.n_tiles ? tile[t] : tile[0]) * (uint32_t)P.nb_in;
    const f32x4* wnode = P.afrag + (size_t)node * P.node_blocks * 64 + lane;
    const float* bnode = P.bias + (size_t)node * P.bias_floats + g * 4;
    const int2* kt = P.kb1tab + (size_t)node * P.kb1;
    const int nf = P.nf;
    // GEMM-2 weights of this wave's output tile do not depend on z: fetch them first
    f32x4 a2[KB];
    const int k2n = mt1n * nf;
    if (P.has_exp && w < mt2n) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < k2n) a2[k] = wnode[((size_t)(P.sum_in ? 0 : P.kb1 * mt1n) + (size_t)k * mt2n + w) * 64];
    }
    // Remainder tiles (P.a4x4: the stage's last tile of both affines is stored in 4x4 form, hg_fused_dev.hpp): the wave that owns
    // that tile multiplies with v_mfma_f32_4x4x1 into d4 and folds the four partial sums afterwards — the same products in the
    // same order as the k_stage REM instantiations
    const bool rem1 = REM && w == mt1n - 1, rem2 = REM && w == mt2n - 1;      // (REM instantiation <=> P.a4x4)
    f32x4 z[T], d4[T];
#pragma unroll
    for (int t = 0; t < T; ++t) d4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (w < mt1n) {
        const f32x4 bb = *(const f32x4*)(bnode + w * 16);
#pragma unroll
        for (int t = 0; t < T; ++t) z[t] = bb;
        if (P.sum_in) {
            // hoisted first affine (StageParams::sum_in): z tile w = ((bias + child 0's tile w) + child 1's) + ...; all blocks requested first
            int on[KB];
            f32x4 bf[KB][T];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const bool real = k < P.n_kids;
                const int2 e = kt[(real ? k : 0) * mt1n + w];
                on[k] = real ? e.y : 0;
#pragma unroll
                for (int t = 0; t < T; ++t) bf[k][t] = P.in[(size_t)(trow[t] + (uint32_t)e.x) * 64 + lane];
            }
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (on[k]) {
#pragma unroll
                    for (int t = 0; t < T; ++t) z[t] += bf[k][t];
                }
        } else
        for (int k0 = 0; k0 < P.kb1; k0 += KB) {
            // the whole batch of K-block entries first (scalar loads that do not wait for one another; the table has 8 spare
            // entries behind the last node), then every weight / input block of the batch, then the MFMAs
            int2 ent[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) ent[k] = kt[k0 + k];
            f32x4 a1[KB], bf[KB][T];
            int nks[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const bool real = k0 + k < P.kb1;
                nks[k] = real ? ent[k].y : 0;
                const int sb = real ? ent[k].x : ent[0].x, wk = real ? k0 + k : k0;      // (blocks beyond the node's: a harmless re-read, no MFMA)
                a1[k] = wnode[((size_t)wk * mt1n + w) * 64];
                load_kblock<T>(P, trow, sb, real ? ent[k].y : ent[0].y, lane, bf[k]);
            }
            if (REM && rem1) {
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const int nk = nks[k] & 255, r0 = (nks[k] >> 8) & 255;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r >= r0 && r < nk) {
#pragma unroll
                            for (int t = 0; t < T; ++t) d4[t] = MFMA4(a1[k][r], bf[k][t][r], d4[t]);
                        }
                }
            } else {
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const int nk = nks[k] & 255, r0 = (nks[k] >> 8) & 255;      // (r0 > 0: a lane-major packed remainder block)
                    if (nks[k] == 4) {      // a whole block: four k-steps, no branch between them
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int t = 0; t < T; ++t) z[t] = MFMA16(a1[k][r], bf[k][t][r], z[t]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (r >= r0 && r < nk) {
#pragma unroll
                                for (int t = 0; t < T; ++t) z[t] = MFMA16(a1[k][r], bf[k][t][r], z[t]);
                            }
                    }
                }
            }
        }
        if (rem1) {
#pragma unroll
            for (int t = 0; t < T; ++t) add_rem4(z[t], d4[t]);
        }
        if (!P.has_exp) {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (tile[t] < P.n_tiles) P.out[((size_t)tile[t] * P.nb_out + node * P.mto + w) * 64 + lane] = z[t];
            return;   // linear stage: no barrier follows on any path
        }
        for (int fi = 0; fi < nf; ++fi) {
            const int fk = (P.funcp >> (4 * fi)) & 15;
            const float ex = P.expo[fi];
#pragma unroll
            for (int t = 0; t < T; ++t) smem[((fi * mt1n + w) * T + t) * 64 + lane] = apply_func_uniform(fk, ex, z[t]);
        }
    } else if (!P.has_exp) {
        return;
    }
    __syncthreads();
    if (w >= mt2n) return;
#pragma unroll
    for (int t = 0; t < T; ++t) d4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 y[T];
    {
        const f32x4 bb = *(const f32x4*)(bnode + (mt1n + w) * 16);
#pragma unroll
        for (int t = 0; t < T; ++t) y[t] = bb;
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k >= k2n) continue;
        const int mt1 = k / nf, fi = k - mt1 * nf;
        const int nk = (P.nk2p[mt1] >> (4 * fi)) & 15;
        f32x4 e[T];
#pragma unroll
        for (int t = 0; t < T; ++t) e[t] = smem[((fi * mt1n + mt1) * T + t) * 64 + lane];
        if (REM && rem2) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < nk) {
#pragma unroll
                    for (int t = 0; t < T; ++t) d4[t] = MFMA4(a2[k][r], e[t][r], d4[t]);
                }
        } else if (nk == 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < T; ++t) y[t] = MFMA16(a2[k][r], e[t][r], y[t]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < nk) {
#pragma unroll
                    for (int t = 0; t < T; ++t) y[t] = MFMA16(a2[k][r], e[t][r], y[t]);
                }
        }
    }
    if (rem2) {
#pragma unroll
        for (int t = 0; t < T; ++t) add_rem4(y[t], d4[t]);
    }
    if (REM && P.pack_base > 0) {      // packed remainder tiles (StageParams::pack_base): full tiles as blocks, the remainder rows into the shared block
        if (rem2) {
            const int slot = __builtin_amdgcn_readfirstlane(P.pack_slot[node]);
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (tile[t] < P.n_tiles) *packed_slot_ptr(P, tile[t], slot, lane) = y[t][0];
        } else {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (tile[t] < P.n_tiles) P.out[((size_t)tile[t] * P.nb_out + node * (mt2n - 1) + w) * 64 + lane] = y[t];
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (tile[t] < P.n_tiles) P.out[((size_t)tile[t] * P.nb_out + node * P.mto + w) * 64 + lane] = y[t];
}

// Fragment order -> caller's row-major y (first y_cols columns).
template <typename YT>
__global__ void k_unpack(const float* __restrict__ act, int nb, const int32_t* __restrict__ col_base, YT* __restrict__ y,
                         int64_t ldy, int64_t n, int cols) {
    int64_t total = n * cols;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t row = idx / cols;
        int c = (int)(idx - row * cols);
        int64_t tile = row >> 4;
        int jj = (int)(row & 15);
        y[row * ldy + c] = (YT)act[tile * nb * 256 + col_base[c] + jj * 4];
    }
}

// ---- launch tables -----------------------------------------------------------------------------

template <int MT1, int MT2>
StageFn pick_stage_t(int T) {
    if (T == 2) return k_stage<MT1, MT2, 2>;
    return k_stage<MT1, MT2, 1>;
}
template <int MT1>
StageFn pick_stage_m2(int mt2, int T) {
    switch (mt2) {
        case 1: return pick_stage_t<MT1, 1>(T);
        case 2: return pick_stage_t<MT1, 2>(T);
        case 3: return pick_stage_t<MT1, 3>(T);
        default: return pick_stage_t<MT1, 4>(T);
    }
}
StageFn pick_stage(int mt1, int mt2, int T, bool rem = false, int kbf = 0, bool fs = false, int pk = -1) {
    if (pk >= 0) {      // slot-major packed input at K-block 1 of 3 (plan_slot_major admits exactly these shapes)
        if (pk == 1 && kbf == 3 && T == 2 && rem && mt1 == 3 && mt2 == 3) return fs ? (StageFn)k_stage<3, 3, 2, false, true, 3, true, 1> : (StageFn)k_stage<3, 3, 2, false, true, 3, false, 1>;
        if (pk == 1 && kbf == 3 && T == 2 && rem && mt1 == 2 && mt2 == 2) return (StageFn)k_stage<2, 2, 2, false, true, 3, false, 1>;
        return nullptr;
    }
    if (fs) {       // expansion (identity, |x|^p) at compile time: the shapes of the preset networks' middle layers
        if (kbf == 3 && T == 2 && rem && mt1 == 3 && mt2 == 3) return (StageFn)k_stage<3, 3, 2, false, true, 3, true>;
        if (kbf == 4 && T == 2 && !rem && mt1 == 3 && mt2 == 3) return (StageFn)k_stage<3, 3, 2, false, false, 4, true>;
        if (kbf == 0 && !rem && mt1 == 4 && mt2 == 4) return T == 2 ? (StageFn)k_stage<4, 4, 2, false, false, 0, true> : (StageFn)k_stage<4, 4, 1, false, false, 0, true>;
    }
    if (kbf == 4 && T == 2) {     // whole-visit prefetch (small nodes of four K-blocks; plan time checks kb1 == 4)
        if (rem && mt1 == 3 && mt2 == 3) return (StageFn)k_stage<3, 3, 2, false, true, 4>;
        if (rem && mt1 == 2 && mt2 == 2) return (StageFn)k_stage<2, 2, 2, false, true, 4>;
        if (!rem && mt1 == 3 && mt2 == 3) return (StageFn)k_stage<3, 3, 2, false, false, 4>;
        if (!rem && mt1 == 2 && mt2 == 2) return (StageFn)k_stage<2, 2, 2, false, false, 4>;
    }
    if (kbf == 3 && T == 2) {     // the same with the children's remainder tiles packed into one shared block
        if (rem && mt1 == 3 && mt2 == 3) return (StageFn)k_stage<3, 3, 2, false, true, 3>;
        if (rem && mt1 == 2 && mt2 == 2) return (StageFn)k_stage<2, 2, 2, false, true, 3>;
    }
    if (rem) {      // instantiated where the synthetic and test networks need it (plan time checks the same list)
        if (mt1 == 3 && mt2 == 3) return T == 2 ? (StageFn)k_stage<3, 3, 2, false, true> : (StageFn)k_stage<3, 3, 1, false, true>;
        if (mt1 == 2 && mt2 == 2) return T == 2 ? (StageFn)k_stage<2, 2, 2, false, true> : (StageFn)k_stage<2, 2, 1, false, true>;
    }
    switch (mt1) {
        case 1: return pick_stage_m2<1>(mt2, T);
        case 2: return pick_stage_m2<2>(mt2, T);
        case 3: return pick_stage_m2<3>(mt2, T);
        default: return pick_stage_m2<4>(mt2, T);
    }
}


// ---- the executor --------------------------------------------------------------------------------
// What a call launches — route and shape per stage — is the call plan's (hg_fused_call.hpp, host only); here its steps are carried out.

// Device mirrors of the plan's tables (hg_fused_plan.hpp): one StageDev per stage and one SubRunDev per sub-tree run, in the plan's
// order; filled by to_device(), freed by release().
struct StageDev {
    DevBuf afrag, bias, kb1tab, chunks, runs, piece, koff, kmean, kcol, gcol, etab, pack_slot;
    DevBuf fold_frag, fold_bias;      // stage 1 of a plan with the link 0 -> 1 folded
    DevBuf fold_last;                 // ... and its one-row k-steps packed (stage 0 of such a plan: fold_a1 / fold_b1 go up as afrag / bias)
    DevBuf pair_kids, kb1tab_pre, bias_pre;      // a hoisted stage whose nodes have two children each (HostStage::pair_kids)
};
struct SubRunDev {
    DevBuf nodes[kMaxTail], tab[kMaxTail];
};

// Counters of the dynamic tile queues (16 words apart); zeroed once, then only ever advanced.  One set per kernel that
// uses them (every launch advances all of ITS counters by the same amount).
struct WorkQueue {
    DevBuf ctr;
    uint32_t base = 0;
};

// What one call writes (Executor::set_lanes): two calls on two lanes share nothing they store to.
constexpr int kMaxLanes = 2;
struct Lane {
    DevBuf bufA, bufB;                    // activation workspace (fragment order), ping-pong
    int64_t cap_rows = 0;
    WorkQueue wq_front, wq_direct, wq_direct_wg;
    int32_t* err_host = nullptr;          // error word the polling kernels write (device_error_word)
    int32_t* err_dev = nullptr;
    std::vector<CallStep> steps;          // the call being enqueued (plan_call): sized by the first call, refilled by every one
};

class FusedExecutor : public Executor {
public:
    explicit FusedExecutor(std::unique_ptr<const FusedPlan> plan) : plan_(std::move(plan)) {}

    int plan_kind() const override { return HG_PLAN_FUSED; }
    int n_stages() const override { return (int)plan_->stages.size() + 1; }
    std::string stage_name(int i) const override {
        if (i == 1 && plan_->fuse01 && !plan_->opt.fold01)
            return plan_->stages[i].name + "  [link 0 -> 1 stays as it is: switched off (HIGSFA_NO_FOLD01)]";
        if (i == 1 && plan_->fold01 && !plan_->opt.fold01_pack)
            return plan_->stages[i].name + "  [the link's one-row k-steps stay as they are: switched off (HIGSFA_NO_FOLD01_PACK)]";
        if (i < (int)plan_->stages.size() && plan_->stages[i].sum_in && !plan_->opt.pair)
            return plan_->stages[i].name + "; unpaired: switched off (HIGSFA_NO_PAIR)";
        if (i < (int)plan_->stages.size()) return plan_->stages[i].name;
        return plan_->tail_begin >= 0 ? std::string("row-major y written by the top-of-hierarchy launch (no unpack pass)")
                                      : std::string("fused unpack (fragment order -> row-major y)");
    }
    std::string describe() const override {
        std::ostringstream os;
        os << "plan: FUSED (fragment-order activations, v_mfma_f32_16x16x4_f32)\n";
        for (int i = 0; i < n_stages(); ++i) os << "  [" << i << "] " << stage_name(i) << "\n";
        return os.str();
    }
    int64_t weight_bytes() const override {
        int64_t t = 0;
        for (auto& s : plan_->stages) t += (int64_t)(s.afrag.size() + s.bias.size()) * 4;
        return t;
    }
    int64_t padded_flops_per_row() const override { return plan_->padded_flops_given; }      // (the hoisted plan's own count: describe())
    int64_t workspace_bytes() const override {      // every lane's
        int64_t t = 0;
        for (int l = 0; l < n_lanes_; ++l) t += (int64_t)(lanes_[l].bufA.bytes + lanes_[l].bufB.bytes);
        return t;
    }

    void to_device() override {
        dev_.resize(plan_->stages.size());
        for (size_t si = 0; si < dev_.size(); ++si) {
            const HostStage& s = plan_->stages[si];
            StageDev& d = dev_[si];
            if (plan_->fold01 && si < 2) {
                // the link 0 -> 1 folded: no kernel reads stage 0's second-affine or stage 1's first-affine fragments any more; the
                // blocks that are read go up node by node (stage 0: A1 = block 0; stage 1: A2 = the blocks behind kb1 x mt1)
                const size_t first = si == 0 ? 0 : (size_t)s.kb1 * s.mt1, count = si == 0 ? (size_t)s.kb1 * s.mt1 : (size_t)s.node_blocks - first;
                std::vector<float> part((size_t)s.n_nodes * count * 256);
                for (int ni = 0; ni < s.n_nodes; ++ni)
                    std::copy_n(s.afrag.data() + ((size_t)ni * s.node_blocks + first) * 256, count * 256, part.data() + (size_t)ni * count * 256);
                // (packed one-row k-steps: stage 0's first affine is the variant with feature 12 repeated, HostStage::fold_a1 / fold_b1)
                const bool variant = plan_->fold01_pack && si == 0;
                if (variant) d.afrag.upload(s.fold_a1.data(), s.fold_a1.size() * 4);
                else d.afrag.upload(part.data(), part.size() * 4);
                if (si == 1) {
                    d.fold_frag.upload(s.fold_frag.data(), s.fold_frag.size() * 4);
                    d.fold_bias.upload(s.fold_bias.data(), s.fold_bias.size() * 4);
                    if (plan_->fold01_pack) d.fold_last.upload(s.fold_last.data(), s.fold_last.size() * 4);
                }
            } else {
                d.afrag.upload(s.afrag.data(), s.afrag.size() * 4);
            }
            if (plan_->fold01_pack && si == 0) d.bias.upload(s.fold_b1.data(), s.fold_b1.size() * 4);
            else d.bias.upload(s.bias.data(), s.bias.size() * 4);
            if (!s.kb1tab.empty()) d.kb1tab.upload(s.kb1tab.data(), s.kb1tab.size() * 4);
            if (!s.gcol.empty()) d.gcol.upload(s.gcol.data(), s.gcol.size() * 4);
            if (!s.etab.empty()) d.etab.upload(s.etab.data(), s.etab.size() * 4);
            if (!s.pack_slot.empty()) d.pack_slot.upload(s.pack_slot.data(), s.pack_slot.size() * 4);
            if (!s.pair_kids.empty()) {
                d.pair_kids.upload(s.pair_kids.data(), s.pair_kids.size() * 4);
                d.kb1tab_pre.upload(s.kb1tab_pre.data(), s.kb1tab_pre.size() * 4);
                d.bias_pre.upload(s.bias_pre.data(), s.bias_pre.size() * 4);
            }
            if (!s.chunks.empty()) {
                d.chunks.upload(s.chunks.data(), s.chunks.size() * sizeof(DChunk));
                d.runs.upload(s.runs.data(), s.runs.size() * sizeof(DRun));
                d.piece.upload(s.piece_col.data(), s.piece_col.size() * 4);
                d.koff.upload(s.koff.data(), s.koff.size() * 4);
                d.kmean.upload(s.kmean.data(), s.kmean.size() * 4);
                if (!s.kcol.empty()) d.kcol.upload(s.kcol.data(), s.kcol.size() * 4);
            }
        }
        sub_dev_.resize(plan_->sub_runs.size());
        for (size_t ri = 0; ri < sub_dev_.size(); ++ri) {
            const SubRun& r = plan_->sub_runs[ri];
            for (int k = 0; k < r.len; ++k) {
                sub_dev_[ri].nodes[k].upload(r.nodes[k].data(), r.nodes[k].size() * 4);
                if (k > 0) sub_dev_[ri].tab[k].upload(r.tab[k].data(), r.tab[k].size() * 4);
            }
        }
        d_col_base_.upload(plan_->col_base.data(), plan_->col_base.size() * 4);
        d_col_of_.upload(plan_->col_of.data(), plan_->col_of.size() * 4);
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            n_cus_ = prop.multiProcessorCount;
    }

    void reserve(int64_t rows) override {      // every lane
        for (int l = 0; l < n_lanes_; ++l) reserve_lane(lanes_[l], rows);
    }

    // Lanes (Executor::set_lanes): everything a call writes lives in a Lane; the plan and its device mirrors are shared and
    // only read once to_device() has run.  The lane of the call being enqueued is passed down to whatever touches its state.
    bool set_lanes(int n) override {
        if (n < 1 || n > kMaxLanes) return false;
        for (int l = n; l < n_lanes_; ++l) release_lane(lanes_[l]);
        for (int l = n_lanes_; l < n; ++l) reserve_lane(lanes_[l], lanes_[0].cap_rows);
        n_lanes_ = n;
        return true;
    }
    int lanes() const override { return n_lanes_; }

    void run(const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype, int64_t y_cols, int64_t ldy,
             hipStream_t st, hipEvent_t* ev) override {
        run_in(lanes_[0], x, x_dtype, n, ldx, y, y_dtype, y_cols, ldy, st, ev);
    }
    void run_lane(int lane, const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype, int64_t y_cols, int64_t ldy,
                  hipStream_t st) override {
        if (lane < 0 || lane >= n_lanes_) fail(HG_ERR_ARG, "lane %d outside 0..%d", lane, n_lanes_ - 1);
        run_in(lanes_[lane], x, x_dtype, n, ldx, y, y_dtype, y_cols, ldy, st, nullptr);
    }

    void run_in(Lane& L, const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype, int64_t y_cols, int64_t ldy,
                hipStream_t st, hipEvent_t* ev) {
        check_device_error();      // of an earlier call: the word is host memory the kernels write through
        if (dev_.size() != plan_->stages.size()) fail(HG_ERR_STATE, "fused: the plan is not on a device");
        if (n > L.cap_rows) {
            // the buffers about to be freed may still be read by this lane's last step, which ran on `st`.  The other lane's
            // buffers are not touched, but its step is drained as well: freeing device memory synchronises the whole device
            if (n_lanes_ > 1) HG_HIP(hipStreamSynchronize(st));
            reserve_lane(L, n);
        }
        // (Cutting a batch into row ranges on separate streams, plain or staggered, was measured and dropped: 0.69-0.84 ms
        // against 0.65 at N = 4096 — DESIGN.md §6.1.)
        run_range(L, x, x_dtype, n, ldx, y, y_dtype, y_cols, ldy, st, ev);
    }

    void run_range(Lane& L, const void* x, int x_dtype, int64_t n, int64_t ldx, void* y, int y_dtype, int64_t y_cols, int64_t ldy,
                   hipStream_t st, hipEvent_t* ev) {
        const int n_tiles = (int)((n + 15) / 16);
        FrontInput fi;
        fi.vec4_ok = rows_vec4(x, ldx, x_dtype);
        fi.x_dtype = x_dtype;
        fi.ldx = ldx;
        plan_call(*plan_, n_tiles, fi, L.steps);
        int e = 0;
        auto record = [&](int k) {      // k events after the last launch: one per stage it covered (the first carries its time)
            if (ev)
                for (int i = 0; i < k; ++i) HG_HIP(hipEventRecord(ev[e++], st));
        };
        record(1);
        f32x4* cur = (f32x4*)L.bufA.p;
        f32x4* nxt = (f32x4*)L.bufB.p;
        for (const CallStep& step : L.steps) {
            const int si = step.stage;
            if (step.route == Route::Top) {
                debug_line(step, 0, 1);
                launch_top(si, cur, n_tiles, y, y_dtype, y_cols, ldy, n, st);
                record(step.covered + 1);      // this stage, the ones above and the unpack pass it replaces
                HG_HIP(hipGetLastError());
                return;
            }
            if (step.route == Route::Subtree) {
                debug_line(step, 0, 1);
                launch_subtrees(plan_->sub_runs[step.sub_run], sub_dev_[step.sub_run], cur, nxt, n_tiles, st);
                std::swap(cur, nxt);
                record(step.covered);
                continue;
            }
            const HostStage& s = plan_->stages[si];
            const StageDev& d = dev_[si];
            StageParams P = stage_params(s, d, cur, nxt, n_tiles);
            switch (step.route) {
                case Route::Gather:      // row-major input -> fragment order
                    debug_line(step, 0, 1);
                    launch_im2frag(x, x_dtype, ldx, n, n_tiles, s.nb_out, (const int32_t*)d.gcol.p, nxt, step.sh.vec4 ? 1 : 0, (unsigned)step_blocks(step, 1), st);
                    break;
                case Route::IgSweep:
                case Route::IgSplit: launch_igsfa(step, s, P, st); break;
                case Route::Front01d:
                case Route::Front01p: launch_front_pair(L, step, s, d, P, x, x_dtype, ldx, n, n_tiles, cur, st); break;
                case Route::Front0p:
                case Route::Front0: launch_front(step, s, d, P, x, x_dtype, ldx, n, st); break;
                case Route::ProdSweep: launch_prod(step, s, d, P, st); break;
                case Route::Splitm: launch_splitm(step, s, P, st); break;
                default:
                    if (step.in_summed) {      // a hoisted stage of one child per node whose first bias adds nothing: (-0.0f) + x == x
                        P.kb1tab = (const int2*)d.kb1tab_pre.p;
                        P.bias = (const float*)d.bias_pre.p;
                        P.kb1 = step.sh.kb1;
                        P.n_kids = step.sh.n_kids;
                        P.nb_in = s.n_nodes * s.mt1;
                    }
                    if (step.route == Route::SumPair) launch_stage_pair(step, s, plan_->stages[si + 1], dev_[si + 1], P, st);
                    else launch_stage(step, s, P, st);
            }
            if (step.covered == 1) std::swap(cur, nxt);      // (fused front: layer 1 wrote `cur`, which stage 2 reads)
            record(step.covered);
        }
        launch_unpack(cur, n, y, y_dtype, y_cols, ldy, st);
        record(1);
        HG_HIP(hipGetLastError());
    }

    void release() override {
        for (Lane& L : lanes_) release_lane(L);
        n_lanes_ = 1;
        d_col_base_.free();
        d_col_of_.free();
        sub_dev_.clear();
        dev_.clear();
    }

private:
    void reserve_lane(Lane& L, int64_t rows) {
        int64_t tiles = (rows + 15) / 16;
        size_t need = (size_t)tiles * plan_->max_nb * 1024;
        L.bufA.alloc(need);
        L.bufB.alloc(need);
        L.cap_rows = std::max(L.cap_rows, tiles * 16);
        L.steps.reserve(plan_->stages.size());
    }
    void release_lane(Lane& L) {
        L.bufA.free();
        L.bufB.free();
        L.wq_front.ctr.free();
        L.wq_direct.ctr.free();
        L.wq_direct_wg.ctr.free();
        L.wq_front.base = L.wq_direct.base = L.wq_direct_wg.base = 0;
        if (L.err_host) (void)hipHostFree(L.err_host);
        L.err_host = nullptr;
        L.err_dev = nullptr;
        L.cap_rows = 0;
    }

    // resident workgroups per CU for (kernel, block size, LDS) — cached occupancy query
    int resident_blocks(StageFn fn, int threads, size_t lds) {
        set_lds_limit(fn, lds);
        auto key = std::make_tuple((const void*)fn, threads, lds);
        auto it = occ_.find(key);
        if (it != occ_.end()) return it->second;
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, threads, lds) != hipSuccess || nb < 1) nb = 1;
        occ_[key] = nb;
        return nb;
    }

    uint32_t* work_counters(WorkQueue& q, int n, hipStream_t st) {
        const size_t need = (size_t)n * 64;
        if (q.ctr.bytes < need) {
            q.ctr.alloc(std::max<size_t>(need, 64 * 1024));
            // counters and base start at the same value and only their difference matters; HIGSFA_WQ_START puts them just below
            // 2^32 so that a test can cross the wrap-around that a long-running process reaches after ~10^7 calls
            HG_HIP(hipMemsetD32Async((hipDeviceptr_t)q.ctr.p, (int)plan_->opt.wq_start, q.ctr.bytes / 4, st));
            q.base = plan_->opt.wq_start;
        }
        return (uint32_t*)q.ctr.p;
    }

    // Error word shared with the kernels that poll (k_chain, k_stage01d with the workgroup queue): pinned, device-mapped
    // host memory, so the host can look at it without synchronising.  A poll only runs out on a bug; the run that hit it
    // produced wrong features, and every later call on this flow fails loudly.
    int32_t* device_error_word(Lane& L) {
        if (!L.err_host) {
            HG_HIP(hipHostMalloc((void**)&L.err_host, 64, hipHostMallocMapped));
            *L.err_host = 0;
            HG_HIP(hipHostGetDevicePointer((void**)&L.err_dev, L.err_host, 0));
        }
        return L.err_dev;
    }
    void check_errors() override { check_device_error(); }
    void check_device_error() {      // every lane's word
        for (const Lane& L : lanes_)
            if (L.err_host && *(volatile int32_t*)L.err_host != 0)
                fail(HG_ERR_DEVICE, "fused: a bounded poll in a persistent kernel ran out (code %d); the features of that call are invalid", (int)*L.err_host);
    }

    void set_lds_limit(StageFn fn, size_t bytes) {
        if (bytes <= 64 * 1024) return;
        if (bytes > 160 * 1024) fail(HG_ERR_FORMAT, "fused: a node needs %zu bytes of LDS (> 160 KiB)", bytes);
        auto it = lds_set_.find((const void*)fn);
        if (it != lds_set_.end() && it->second >= bytes) return;
        HG_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024)));
        lds_set_[(const void*)fn] = 160 * 1024;
    }

    StageParams stage_params(const HostStage& hs, const StageDev& d, const f32x4* in, f32x4* out, int n_tiles) const {
        StageParams R{};
        R.afrag = (const f32x4*)d.afrag.p;
        R.bias = (const float*)d.bias.p;
        R.kb1tab = (const int2*)d.kb1tab.p;
        R.in = in;
        R.out = out;
        R.n_nodes = hs.n_nodes;
        R.kb1 = hs.kb1;
        R.nf = hs.nf;
        R.has_exp = hs.has_exp ? 1 : 0;
        R.node_blocks = hs.node_blocks;
        R.bias_floats = hs.bias_floats;
        R.n_tiles = n_tiles;
        R.nb_in = hs.nb_in;
        R.nb_out = hs.nb_out;
        R.mto = hs.mto;
        R.pack_base = hs.pack_out ? hs.n_nodes * (hs.mto - 1) : 0;
        R.pack_soa = hs.pack_soa ? 1 : 0;
        R.pack_in = hs.pack_in;
        R.pack_slot = (const int32_t*)d.pack_slot.p;
        R.a4x4 = hs.rem4 ? 1 : 0;
        R.sum_in = hs.sum_in ? 1 : 0;
        R.n_kids = hs.n_kids;
        if (plan_->fold01 && (&hs == &plan_->stages[0] || &hs == &plan_->stages[1])) {      // what to_device uploaded of these two stages
            const bool first = &hs == &plan_->stages[0];
            R.node_blocks = first ? hs.kb1 * hs.mt1 : hs.node_blocks - hs.kb1 * hs.mt1;
            R.fold_frag = (const f32x4*)d.fold_frag.p;
            R.fold_bias = (const float*)d.fold_bias.p;
            R.fold_last = (const float*)d.fold_last.p;
            if (plan_->fold01_pack && first) R.bias_floats = 16;      // HostStage::fold_b1: the first bias alone
        }
        for (int fi = 0; fi < hs.nf; ++fi) {
            R.funcp |= (uint32_t)hs.funcs[fi].kind << (4 * fi);
            R.expo[fi] = (float)hs.funcs[fi].expo;
            for (int mt1 = 0; mt1 < hs.mt1; ++mt1) R.nk2p[mt1] |= (uint32_t)hs.nk2[mt1][fi] << (4 * fi);
        }
        return R;
    }

    // the caller's rows allow 16-byte loads (4-byte for uint8): FrontInput::vec4_ok, for the row gather and the front kernels
    static bool rows_vec4(const void* x, int64_t ldx, int x_dtype) {
        const size_t esz = dtype_size(x_dtype), valign = x_dtype == HG_U8 ? 4 : 16;
        return ldx % 4 == 0 && ((uintptr_t)x % valign) == 0 && (ldx * esz) % valign == 0;
    }

    // The step's sweep parameters, from its shape and — the second phase of the call plan — the occupancy of the kernel the shape
    // mapped to.  Returns the grid.
    int64_t fill_sweep(const CallStep& step, StageFn fn, StageParams& P) {
        const CallShape& sh = step.sh;
        const int occ = resident_blocks(fn, sh.threads, sh.lds);
        P.nodes_per_group = sh.per_group;
        P.nodes_per_wg = sh.per_group;
        P.n_chunks = sh.n_groups;
        P.tile_groups = sh.tile_groups;
        P.tile_parts = step_tile_parts(step, occ);
        debug_line(step, occ, P.tile_parts);
        return step_blocks(step, P.tile_parts);
    }

    void debug_line(const CallStep& step, int occ, int tile_parts) const {
        if (!plan_->opt.debug) return;
        char buf[512];
        fprintf(stderr, "%s\n", format_step(*plan_, step, occ, tile_parts, buf, sizeof buf));
    }

    // the top of the hierarchy as one launch that ends in the caller's rows (hg_fused_tail.hip)
    void launch_top(int si, const f32x4* in, int n_tiles, void* y, int y_dtype, int64_t y_cols, int64_t ldy, int64_t n, hipStream_t st) {
        TailParams TP = tail_params(si, in, n_tiles, y, y_dtype, y_cols, ldy, n);
        // two tiles per workgroup only for narrow tops on long batches, and only while their doubled LDS image fits
        const int T = (n_tiles >= 512 && tail_waves(TP) <= 8 && tail_lds_bytes(TP, 2) <= (size_t)160 * 1024) ? 2 : 1;
#ifdef HIGSFA_DIAG
        const bool stamped = plan_->opt.stamp_stage == si;
        if (stamped) tail_stamps_begin(TP, (size_t)((n_tiles + T - 1) / T), st);
#endif
        launch_tail(TP, T, st);
#ifdef HIGSFA_DIAG
        if (stamped) tail_stamps_report("top-of-hierarchy launch", si, TP.n_stages, (size_t)((n_tiles + T - 1) / T), st);
#endif
    }

    // a short batch: the layers of a sub-tree run as independent sub-trees in one launch (hg_fused_tail.hip)
    void launch_subtrees(const SubRun& sr, const SubRunDev& sd, const f32x4* in, f32x4* out, int n_tiles, hipStream_t st) {
        TailParams TP = subtree_params(sr, sd, in, out, n_tiles);
#ifdef HIGSFA_DIAG
        const bool stamped = plan_->opt.stamp_stage == sr.begin;
        if (stamped) tail_stamps_begin(TP, (size_t)sr.n * n_tiles, st);
#endif
        launch_subtree(TP, st);
#ifdef HIGSFA_DIAG
        if (stamped) tail_stamps_report("sub-tree launch", sr.begin, TP.n_stages, (size_t)sr.n * n_tiles, st);
#endif
    }

    // iGSFA layer: the folded top of a hierarchy in small workgroups (k_igfold_split), else k_igfold (folded) / k_igsfa (unfolded)
    void launch_igsfa(const CallStep& step, const HostStage& s, StageParams& P, hipStream_t st) {
        const CallShape& sh = step.sh;
        if (step.route == Route::IgSplit) {
            P.ig_folded = 1;
            debug_line(step, 0, 1);
            launch_igfold_split(P, s.mt2, sh.T, (unsigned)step_blocks(step, 1), sh.threads, sh.lds, st);
            return;
        }
        StageFn fn = s.ig_folded ? pick_igfold(s.mt2, sh.T, sh.fs) : pick_igsfa(s.mt1, s.mt2, sh.T, s.kb1);
        const int64_t blocks = fill_sweep(step, fn, P);
        P.nodes_per_wg = sh.nw;      // (k_igsfa / k_igfold: the waves of a workgroup that take batch tiles)
        P.ig_has_lr = s.ig_has_lr ? 1 : 0;
        P.ig_folded = s.ig_folded ? 1 : 0;
        P.nk2p[0] = 0;
        for (int ms = 0; ms < s.mt1; ++ms) P.nk2p[0] |= (uint32_t)s.ig_nks[ms] << (4 * ms);
        hipLaunchKernelGGL(fn, (unsigned)blocks, sh.threads, sh.lds, st, P);
    }

    // what every first-layer kernel reads of the caller's rows and of stage 0's tables
    void front_params(const CallStep& step, const HostStage& s, const StageDev& d, StageParams& P, const void* x, int64_t ldx, int64_t n) const {
        P.chunks = (const DChunk*)d.chunks.p;
        P.runs = (const DRun*)d.runs.p;
        P.piece_col = (const int2*)d.piece.p;
        P.koff = (const int32_t*)d.koff.p;
        P.kmean = (const float*)d.kmean.p;
        P.kcol = (const int32_t*)d.kcol.p;
        P.x = x;
        P.ldx = ldx;
        P.n_rows = n;
        P.lds_stride = s.lds_stride;
        P.nk_last = s.nk_last;
        P.contig4 = s.contig4 ? 1 : 0;
        P.n_chunks = step.sh.n_groups;
        P.vec4 = step.sh.vec4 ? 1 : 0;
    }

    // layers 0 and 1 in one persistent kernel (k_stage01d / k_stage01p); layer 1 writes out1, where its own launch would
    void launch_front_pair(Lane& L, const CallStep& step, const HostStage& s, const StageDev& d, StageParams& P, const void* x, int x_dtype, int64_t ldx, int64_t n,
                           int n_tiles, f32x4* out1, hipStream_t st) {
        const CallShape& sh = step.sh;
        const bool direct = step.route == Route::Front01d;
        front_params(step, s, d, P, x, ldx, n);
        StageParams Q = stage_params(plan_->stages[1], dev_[1], nullptr, out1, n_tiles);
        if (sh.pack && (!Q.fold_last || P.bias_floats != 16)) fail(HG_ERR_STATE, "internal: a packed plan without its packed fragments on the device");
        StageFn2 fn = direct ? pick_stage01d(x_dtype, false, sh.wgq, sh.fold, sh.pack) : pick_stage01p(x_dtype, false, sh.rem4, sh.fspec, sh.fold, sh.scalar, sh.pack);
        if (!fn) fail(HG_ERR_STATE, "internal: no packed front kernel for this plan");      // never an unpacked kernel on packed fragments
        const int occ = resident_blocks((StageFn)fn, sh.threads, sh.lds);
        P.tile_parts = step_tile_parts(step, occ);
        debug_line(step, occ, P.tile_parts);
        const unsigned blocks = (unsigned)step_blocks(step, P.tile_parts);
#ifdef HIGSFA_DIAG
        if (plan_->opt.stamp_stage == 0 && x_dtype == HG_F32 && (direct || !sh.fold)) {      // (the folded k_stage01p has no stamped form)
            fn = direct ? pick_stage01d(HG_F32, true, sh.wgq, sh.fold, sh.pack) : pick_stage01p(HG_F32, true, sh.rem4, sh.fspec, sh.fold);
            stamps_begin(P, (int)blocks, 12, st);
        }
#endif
        P.err = device_error_word(L);
        {   // k_stage01p: one queue of tile groups per chunk; k_stage01d: one queue of tiles per layer-1 node (or per chunk)
            WorkQueue& wq = direct ? (sh.wgq ? L.wq_direct_wg : L.wq_direct) : L.wq_front;
            P.work_ctr = work_counters(wq, sh.queue_ctrs, st);
            P.work_base = wq.base;
            wq.base += (uint32_t)sh.tile_groups;      // what this launch adds to every counter (StageParams::work_ctr)
        }
#ifdef HIGSFA_DIAG
        if (const char* e = getenv("HIGSFA_WHATIF")) P.whatif = atoi(e);
#endif
        hipLaunchKernelGGL(fn, blocks, sh.threads, sh.lds, st, P, Q);
#ifdef HIGSFA_DIAG
        if (P.stamps) front_stamps_report(P.n_chunks, st);
#endif
    }

    // layer 0 alone: k_stage0p (persistent) or k_stage0
    void launch_front(const CallStep& step, const HostStage& s, const StageDev& d, StageParams& P, const void* x, int x_dtype, int64_t ldx, int64_t n, hipStream_t st) {
        const CallShape& sh = step.sh;
        front_params(step, s, d, P, x, ldx, n);
        const bool persistent = step.route == Route::Front0p;
        StageFn fn = persistent ? pick_stage0p(x_dtype) : pick_stage0(s.mt1, s.mt2, sh.T, x_dtype);
        const int occ = persistent ? resident_blocks(fn, sh.threads, sh.lds) : 0;      // (k_stage0: one workgroup per tile group and chunk)
        if (persistent) P.tile_parts = step_tile_parts(step, occ);
        const int64_t blocks = step_blocks(step, P.tile_parts);
        debug_line(step, occ, P.tile_parts);
        set_lds_limit(fn, sh.lds);
        hipLaunchKernelGGL(fn, (unsigned)blocks, sh.threads, sh.lds, st, P);
    }

    void launch_splitm(const CallStep& step, const HostStage& s, const StageParams& P, hipStream_t st) {
        const CallShape& sh = step.sh;
        const unsigned grid = (unsigned)step_blocks(step, 1);
        debug_line(step, 0, 1);
        if (sh.rem4) {
            if (sh.T == 2) hipLaunchKernelGGL((k_stage_splitm<2, true>), grid, sh.threads, sh.lds, st, P, s.mt1, s.mt2);
            else hipLaunchKernelGGL((k_stage_splitm<1, true>), grid, sh.threads, sh.lds, st, P, s.mt1, s.mt2);
        } else if (sh.T == 2)
            hipLaunchKernelGGL(k_stage_splitm<2>, grid, sh.threads, sh.lds, st, P, s.mt1, s.mt2);
        else
            hipLaunchKernelGGL(k_stage_splitm<1>, grid, sh.threads, sh.lds, st, P, s.mt1, s.mt2);
    }

    // an ordinary layer on k_stage: node groups whose weights sit in LDS, swept over the batch's tile groups
    void launch_stage(const CallStep& step, const HostStage& s, StageParams& P, hipStream_t st) {
        const CallShape& sh = step.sh;
        // slot-major packed input (plan_slot_major): the whole-visit-prefetch instantiation reads it at a fixed code position; any
        // other shape of this call (one tile per wave: small batches) takes the generic remainder-tile loop, which tests per block
        StageFn fn = s.pk_kbi >= 0 ? (sh.kbf == 3 ? pick_stage(s.mt1, s.mt2, sh.T, s.rem4, sh.kbf, sh.fs, s.pk_kbi) : nullptr) : pick_stage(s.mt1, s.mt2, sh.T, s.rem4, sh.kbf, sh.fs);
        if (!fn) fn = pick_stage(s.mt1, s.mt2, sh.T, s.rem4, 0, false);
        if (s.sum_in) fn = pick_stage_sum(s.mt1, s.mt2, sh.T, sh.fs);      // hoisted first affine: hg_fused_sum.hip
        const int64_t blocks = fill_sweep(step, fn, P);
        P.pair_chunks = sh.pair_chunks ? 1 : 0;
#ifdef HIGSFA_DIAG
        const int si = step.stage, T = sh.T, kbf = sh.kbf;
        const bool stamp_kbf3 = s.mt1 == 3 && s.mt2 == 3 && T == 2 && s.rem4 && kbf == 3;
        if (plan_->opt.stamp_stage == si && !s.sum_in && (stamp_kbf3 || (s.mt1 == s.mt2 && (s.mt1 == 4 || s.mt1 == 3) && T == 2 && !s.rem4 && kbf == 0))) {
            // diagnostic instantiation with s_memtime stamps (never used in timed runs)
            fn = stamp_kbf3 ? (StageFn)k_stage<3, 3, 2, true, true, 3> : s.mt1 == 4 ? (StageFn)k_stage<4, 4, 2, true> : (StageFn)k_stage<3, 3, 2, true>;
            stamps_begin(P, (int)blocks, 8, st);
        }
#endif
        set_lds_limit(fn, sh.lds);
#ifdef HIGSFA_DIAG
        if (const char* e = getenv("HIGSFA_WHATIF")) P.whatif = atoi(e);
#endif
        hipLaunchKernelGGL(fn, (unsigned)blocks, sh.threads, sh.lds, st, P);
#ifdef HIGSFA_DIAG
        if (P.stamps) stage_stamps_report(si, blocks, sh.nw, st);
#endif
    }

    // launch_stage for the producer of a summed link: one tile set stored per node of `parent`
    void launch_stage_pair(const CallStep& step, const HostStage& s, const HostStage& parent, const StageDev& pd, StageParams& P, hipStream_t st) {
        const CallShape& sh = step.sh;
        StageFn fn = pick_stage_sum_pair(sh.T);
        if (!fn) fail(HG_ERR_STATE, "internal: no pair kernel of %d tiles per wave", sh.T);
        P.pair_kids = (const int2*)pd.pair_kids.p;
        P.pair_bias = (const float*)pd.bias.p;      // the parent stage's own floats (not bias_pre)
        P.pair_bias_floats = parent.bias_floats;
        P.n_pairs = parent.n_nodes;
        P.nb_out = parent.n_nodes * s.mto;
        const int64_t blocks = fill_sweep(step, fn, P);
        hipLaunchKernelGGL(fn, (unsigned)blocks, sh.threads, sh.lds, st, P);
    }

    void launch_prod(const CallStep& step, const HostStage& s, const StageDev& d, StageParams& P, hipStream_t st) {
        StageFn fn = pick_prod(s.mt1, s.mt2, step.sh.T);
        const int64_t blocks = fill_sweep(step, fn, P);
        P.etab = (const int2*)d.etab.p;
        P.neb = s.neb;
        P.nk_last = s.nk_last;
        P.has_clip = s.has_clip ? 1 : 0;
        P.clip_lo = s.clip_lo;
        P.clip_hi = s.clip_hi;
        hipLaunchKernelGGL(fn, (unsigned)blocks, step.sh.threads, step.sh.lds, st, P);
    }

    // fragment order -> the caller's row-major y (where no top-of-hierarchy launch wrote it)
    void launch_unpack(const f32x4* in, int64_t n, void* y, int y_dtype, int64_t y_cols, int64_t ldy, hipStream_t st) {
        const HostStage& last = plan_->stages.back();
        unsigned grid = (unsigned)std::min<int64_t>((n * y_cols + 255) / 256, 4096);
        if (y_dtype == HG_F32)
            hipLaunchKernelGGL(k_unpack<float>, grid, 256, 0, st, (const float*)in, last.nb_out, (const int32_t*)d_col_base_.p,
                               (float*)y, ldy, n, (int)y_cols);
        else if (y_dtype == HG_F64)
            hipLaunchKernelGGL(k_unpack<double>, grid, 256, 0, st, (const float*)in, last.nb_out, (const int32_t*)d_col_base_.p,
                               (double*)y, ldy, n, (int)y_cols);
        else
            fail(HG_ERR_ARG, "output dtype must be f32 or f64");
    }

#ifdef HIGSFA_DIAG
    // k_tail / k_subtree with wall-clock stamps (hg_fused_tail.hip: TAIL_STAMP): where a wave's time goes, layer by layer
    void tail_stamps_begin(TailParams& TP, size_t blocks, hipStream_t st) {
        stamp_buf_.alloc(blocks * 16 * 16 * 8);
        HG_HIP(hipMemsetAsync(stamp_buf_.p, 0, stamp_buf_.bytes, st));
        TP.stamps = (unsigned long long*)stamp_buf_.p;
    }
    void tail_stamps_report(const char* what, int si, int n_layers, size_t blocks, hipStream_t st) {
        HG_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> h(blocks * 16 * 16);
        HG_HIP(hipMemcpy(h.data(), stamp_buf_.p, h.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull;
        for (size_t i = 0; i < h.size(); i += 16)
            if (h[i]) t0 = std::min(t0, h[i]);
        static const char* names[5] = {"loads in", "expanded", "barrier 1", "outputs stored", "barrier 2"};
        double sum[16] = {}, mx[16] = {}, cnt[16] = {};
        for (size_t i = 0; i < h.size(); i += 16)
            for (int k = 0; k < 16; ++k)
                if (h[i + k]) {
                    const double us = (double)(h[i + k] - t0) * 0.01;
                    sum[k] += us; cnt[k] += 1; mx[k] = std::max(mx[k], us);
                }
        fprintf(stderr, "[stamp stage %d] %s, %zu workgroups: us after the first wave's entry, mean (max) over the waves that took part\n", si, what, blocks);
        fprintf(stderr, "[stamp stage %d]   entry %.2f (%.2f)\n", si, cnt[0] ? sum[0] / cnt[0] : 0.0, mx[0]);
        for (int l = 0; l < n_layers; ++l) {
            fprintf(stderr, "[stamp stage %d]   layer %d:", si, l);
            for (int k = 0; k < 5; ++k) {
                const int q = 1 + 5 * l + k;
                fprintf(stderr, "  %s %.2f (%.2f; %.0f waves)", names[k], cnt[q] ? sum[q] / cnt[q] : 0.0, mx[q], cnt[q]);
            }
            fprintf(stderr, "\n");
        }
    }
    // stamped front-kernel / k_stage instantiations: `words` cycle and wall-clock stamps per wave, 8 waves per workgroup
    void stamps_begin(StageParams& P, int blocks, int words, hipStream_t st) {
        stamp_blocks_ = blocks;
        stamp_buf_.alloc((size_t)blocks * 8 * words * 8);
        HG_HIP(hipMemsetAsync(stamp_buf_.p, 0, stamp_buf_.bytes, st));
        P.stamps = (unsigned long long*)stamp_buf_.p;
    }
    void front_stamps_report(int n_chunks, hipStream_t st) {
        HG_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> h((size_t)stamp_blocks_ * 8 * 12);
        HG_HIP(hipMemcpy(h.data(), stamp_buf_.p, h.size() * 8, hipMemcpyDeviceToHost));
        double a[7] = {0, 0, 0, 0, 0, 0, 0}, nwv = 0;
        unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};     // wall clock (100 MHz): entry, loop start, end
        for (size_t i = 0; i < h.size(); i += 12)
            if (h[i + 4]) {
                for (int k = 0; k < 7; ++k) a[k] += h[i + k];
                nwv += 1;
                for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], h[i + 7 + k]); hi[k] = std::max(hi[k], h[i + 7 + k]); }
            }
        {
            double xs[8][4] = {}, ps[16][3] = {};
            for (size_t i = 0, w = 0; i < h.size(); i += 12, ++w)
                if (h[i + 4]) {
                    const int blk = (int)(w / 8), xc = blk % 8, pt = std::min(15, blk / n_chunks);
                    const double life = (h[i + 9] - h[i + 8]) * 0.01, clk = (double)h[i + 4] / (double)h[i + 5] * 100.0;
                    xs[xc][0] += 1; xs[xc][1] += life; xs[xc][2] = std::max(xs[xc][2], life); xs[xc][3] += clk;
                    ps[pt][0] += 1; ps[pt][1] += life; ps[pt][2] = std::max(ps[pt][2], life);
                }
            for (int k = 0; k < 8; ++k)
                if (xs[k][0] > 0) fprintf(stderr, "[stamp stage 0+1] xcd %d: waves %.0f loop us mean %.1f max %.1f clock %.0f MHz\n", k, xs[k][0], xs[k][1] / xs[k][0], xs[k][2], xs[k][3] / xs[k][0]);
            for (int k = 0; k < 16; ++k)
                if (ps[k][0] > 0) fprintf(stderr, "[stamp stage 0+1] part %d: waves %.0f loop us mean %.1f max %.1f\n", k, ps[k][0], ps[k][1] / ps[k][0], ps[k][2]);
        }
        fprintf(stderr, "[stamp stage 0+1] wall clock, us after the first wave's entry: entries until %.1f, loop starts %.1f..%.1f, ends %.1f..%.1f\n",
                (hi[0] - lo[0]) * 0.01, (lo[1] - lo[0]) * 0.01, (hi[1] - lo[0]) * 0.01, (lo[2] - lo[0]) * 0.01, (hi[2] - lo[0]) * 0.01);
        fprintf(stderr, "[stamp stage 0+1] waves %.0f clock %.0f MHz lifetime %.1f us, iterations %.1f; cycles per iteration: "
                        "lds-write+barrier %.0f, fetch issue %.0f, layer0 %.0f, layer1+store %.0f (sum %.0f)\n",
                nwv, a[4] / a[5] * 100.0, a[5] / nwv / 100.0, a[6] / nwv, a[0] / a[6], a[1] / a[6], a[2] / a[6], a[3] / a[6],
                (a[0] + a[1] + a[2] + a[3]) / a[6]);
    }
    void stage_stamps_report(int si, int64_t blocks, int nw, hipStream_t st) {
        HG_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> h((size_t)stamp_blocks_ * 8 * 8);
        HG_HIP(hipMemcpy(h.data(), stamp_buf_.p, h.size() * 8, hipMemcpyDeviceToHost));
        double c = 0, g1 = 0, tl = 0, all = 0, it = 0, nwv = 0, rt = 0;
        unsigned long long lo0 = ~0ull, hi0 = 0, lo1 = ~0ull, hi1 = 0;
        std::vector<unsigned long long> ends;
        for (size_t i = 0; i < h.size(); i += 8)
            if (h[i + 3]) {
                c += h[i]; g1 += h[i + 1]; tl += h[i + 2]; all += h[i + 3]; it += h[i + 4]; rt += h[i + 5]; nwv += 1;
                lo0 = std::min(lo0, h[i + 6]); hi0 = std::max(hi0, h[i + 6]); lo1 = std::min(lo1, h[i + 7]); hi1 = std::max(hi1, h[i + 7]);
                ends.push_back(h[i + 7]);
            }
        std::sort(ends.begin(), ends.end());
        if (!ends.empty())
            fprintf(stderr, "[stamp stage %d] wall clock, us after the first wave's start: starts until %.1f, ends %.1f (10%%) %.1f (50%%) %.1f (90%%) %.1f (last); grid %lld blocks x %d waves\n",
                    (int)si, (hi0 - lo0) * 0.01, (ends[ends.size() / 10] - lo0) * 0.01, (ends[ends.size() / 2] - lo0) * 0.01,
                    (ends[ends.size() * 9 / 10] - lo0) * 0.01, (hi1 - lo0) * 0.01, (long long)blocks, nw);
        fprintf(stderr, "[stamp stage %d] in-kernel clock %.0f MHz, wave lifetime %.1f us\n", (int)si, all / rt * 100.0, rt / nwv / 100.0);
        fprintf(stderr, "[stamp stage %d] waves %.0f  avg cycles/wave: total %.0f  copy+barrier %.0f  gemm1 %.0f  tail %.0f  node-iterations %.1f  (per iteration: gemm1 %.0f tail %.0f)\n",
                (int)si, nwv, all / nwv, c / nwv, g1 / nwv, tl / nwv, it / nwv, g1 / it, tl / it);
    }
#endif

    static void fill_tail_stage(TailStage& S, const HostStage& hs, const StageDev& d) {
        S.afrag = (const f32x4*)d.afrag.p;
        S.bias = (const float*)d.bias.p;
        S.kb1tab = (const int2*)d.kb1tab.p;
        S.n_nodes = hs.n_nodes;
        S.kb1 = hs.kb1;
        S.nf = hs.nf;
        S.has_exp = hs.has_exp ? 1 : 0;
        S.node_blocks = hs.node_blocks;
        S.bias_floats = hs.bias_floats;
        S.nb_out = hs.nb_out;
        S.mto = hs.mto;
        S.mt1 = hs.mt1;
        S.mt2 = hs.mt2;
        S.sum_in = hs.sum_in ? 1 : 0;
        S.n_kids = hs.n_kids;
        for (int fi = 0; fi < hs.nf; ++fi) {
            S.funcp |= (uint32_t)hs.funcs[fi].kind << (4 * fi);
            S.expo[fi] = (float)hs.funcs[fi].expo;
            for (int mt1 = 0; mt1 < hs.mt1; ++mt1) S.nk2p[mt1] |= (uint32_t)hs.nk2[mt1][fi] << (4 * fi);
        }
    }

    TailParams subtree_params(const SubRun& sr, const SubRunDev& sd, const f32x4* in, f32x4* out, int n_tiles) {
        const int sub_begin_ = sr.begin, sub_len_ = sr.len, sub_n_ = sr.n, sub_act_blocks_ = sr.act_blocks, sub_e_blocks_ = sr.e_blocks;
        TailParams TP{};
        TP.n_stages = sub_len_;
        for (int k = 0; k < sub_len_; ++k) {
            fill_tail_stage(TP.st[k], plan_->stages[sub_begin_ + k], dev_[sub_begin_ + k]);
            TP.st[k].n_nodes /= sub_n_;
            TP.sub_nodes[k] = (const int32_t*)sd.nodes[k].p;
            if (k > 0) TP.st[k].kb1tab = (const int2*)sd.tab[k].p;
        }
        TP.in = in;
        TP.out_frag = out;
        TP.n_sub = sub_n_;
        TP.nb_out_frag = plan_->stages[sub_begin_ + sub_len_ - 1].nb_out;
        TP.n_tiles = n_tiles;
        TP.nb_in = plan_->stages[sub_begin_].nb_in;
        TP.act_blocks = sub_act_blocks_;
        TP.e_blocks = sub_e_blocks_;
        return TP;
    }

    TailParams tail_params(int begin, const f32x4* in, int n_tiles, void* y, int y_dtype, int64_t y_cols, int64_t ldy, int64_t n) {
        TailParams TP{};
        const int ns = (int)plan_->stages.size();
        TP.n_stages = ns - begin;
        for (int k = 0; k < TP.n_stages; ++k) {
            fill_tail_stage(TP.st[k], plan_->stages[begin + k], dev_[begin + k]);
        }
        TP.in = in;
        TP.y = y;
        TP.col_of = (const int32_t*)d_col_of_.p;
        TP.ldy = ldy;
        TP.n_rows = n;
        TP.y_cols = (int32_t)y_cols;
        TP.y_f64 = y_dtype == HG_F64 ? 1 : 0;
        if (y_dtype != HG_F32 && y_dtype != HG_F64) fail(HG_ERR_ARG, "output dtype must be f32 or f64");
        TP.n_tiles = n_tiles;
        TP.nb_in = plan_->stages[begin].nb_in;
        TP.act_blocks = plan_->tail_act_blocks;
        TP.e_blocks = plan_->tail_e_blocks;
        return TP;
    }

    const std::unique_ptr<const FusedPlan> plan_;      // read-only: built by build_fused_plan, never written here
    std::vector<StageDev> dev_;                         // [stage] (to_device)
    std::vector<SubRunDev> sub_dev_;                    // [sub-tree run]
    DevBuf d_col_base_, d_col_of_;
    Lane lanes_[kMaxLanes];
    int n_lanes_ = 1;
#ifdef HIGSFA_DIAG
    DevBuf stamp_buf_;
    int stamp_blocks_ = 0;
#endif
    std::map<const void*, size_t> lds_set_;
    std::map<std::tuple<const void*, int, size_t>, int> occ_;
    int n_cus_ = 256;
};

}  // namespace

std::unique_ptr<Executor> make_fused_executor(const TNode& root, std::string* why_not) {
    auto plan = fused::build_fused_plan(root, fused::executor_options(), why_not);
    if (!plan) return nullptr;
    return std::make_unique<FusedExecutor>(std::move(plan));
}

}  // namespace hg
