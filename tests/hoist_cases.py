"""Flows for the hoisted-link tests (tests/test_hoist_plan_host.py on the CPU, tests/test_hoist_gpu.py on the device) and the
stand-alone driver that runs the planner's hoist pass without a device (tests/hoist_plan_driver.cpp).  Untrained: every weight is a
seeded draw (helpers.rand_pca / rand_sfa, or plan_cases.reseed where a digest or a float64 comparison depends on it)."""
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import helpers
from tests.plan_cases import CSRC, ROOT

FUNCS = [N.identity, N.unsigned_08expo]
FUZZ_SEED = 6      # a helpers.subtree_fuzz_net seed whose plan has a hoisted link (test_hoist_plan_host.py checks that it still has)


def _layer(rng, n, d_in, p, s):
    out = []
    for _ in range(n):
        ex = N.GeneralExpansionNode(FUNCS, p)
        out.append(N.FlowNode([helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, helpers.rand_sfa(rng, ex.output_dim, s)]))
    return N.Layer(out)


CHAIN_DIMS = [(13, 13), (20, 24), (24, 40), (40, 60), (60, 60), (60, 60), (60, 20)]


def chain_net(seed=0, dims=CHAIN_DIMS, side=32):
    """side x side input, 4x4 fields, then two-way merges down to one node.  With CHAIN_DIMS: link 0 -> 1 is not eligible (it leads
    into stage 1), links 1 -> 2 .. 5 -> 6 are (P of the parent == S of the child), with parents of 2, 3 and 4 tiles, chained, and a
    last layer whose 20 outputs fill a tile and a quarter."""
    rng = np.random.default_rng(4000 + seed)
    flow, c, w, h = [], 1, side, side
    for li, (p, s) in enumerate(dims):
        field = (4, 4) if li == 0 else ((2, 1) if (li % 2 == 1 and w > 1) or h == 1 else (1, 2))
        sb = N.Rectangular2dSwitchboard((w, h), field, field, c)
        flow += [sb, _layer(rng, sb.output_channels, sb.out_channel_dim, p, s)]
        w, h = sb.out_channels_xy
        c = s
    assert w * h == 1
    return flow


QUAD_DIMS = [(12, 24), (24, 30), (28, 36), (32, 40), (38, 10)]


def quad_net(seed=0):
    """64 x 32 input, 4x4 fields (128 nodes), three 2x2 merges (32, 8 and 2 nodes: four children per parent) and a pair merge.
    Links 1 -> 2, 2 -> 3 and 3 -> 4 are eligible; the parents of 28 and 32 columns are narrower than their children's 30 and 36."""
    rng = np.random.default_rng(4100 + seed)
    flow, c, w, h = [], 1, 64, 32
    for li, (p, s) in enumerate(QUAD_DIMS):
        field = (4, 4) if li == 0 else ((2, 2) if w > 1 and h > 1 else (2, 1))
        sb = N.Rectangular2dSwitchboard((w, h), field, field, c)
        flow += [sb, _layer(rng, sb.output_channels, sb.out_channel_dim, p, s)]
        w, h = sb.out_channels_xy
        c = s
    assert w * h == 1
    return flow


def small_net(seed=0):
    """The smallest net with a hoisted link and a permuting switchboard in front of the parents: 8 x 8 input, 16 + 4 nodes, then two
    parents that read their two children's columns through a PInvSwitchboard in a shuffled order."""
    rng = np.random.default_rng(4200 + seed)
    sb0 = N.Rectangular2dSwitchboard((8, 8), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((4, 4), (2, 2), (2, 2), 5)
    cols = []
    for pj in range(2):
        mine = np.arange(18 * pj, 18 * pj + 18)      # children 2 pj and 2 pj + 1, nine columns each
        cols.append(rng.permutation(mine))
    sb2 = N.PInvSwitchboard(36, np.concatenate(cols))
    return [sb0, _layer(rng, 16, 4, 4, 5), sb1, _layer(rng, 4, 20, 7, 9), sb2, _layer(rng, 2, 18, 6, 11)]


def _node(rng, d_in, p, s, funcs=None):
    ex = N.GeneralExpansionNode(funcs or FUNCS, p)
    return N.FlowNode([helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, helpers.rand_sfa(rng, ex.output_dim, s)])


def grouped_board(rng, widths, groups):
    """A PInvSwitchboard that hands the children (of `widths` columns each, laid side by side) to one parent per entry of `groups`.
    A parent reads all the columns of its children, shuffled, but so that it meets its children first in the order the group
    lists them — the order in which the planner records them (FNode::kids) and every kernel family adds their tiles."""
    col0 = np.concatenate([[0], np.cumsum(widths)])
    conn = []
    for grp in groups:
        seq = np.zeros(0, dtype=np.int64)
        for c in reversed(grp):      # one column of c in front, the others anywhere among what the later children already hold
            cols = col0[c] + rng.permutation(widths[c])
            merged = np.empty(seq.size + cols.size - 1, dtype=np.int64)
            mine = np.zeros(merged.size, dtype=bool)
            mine[rng.choice(merged.size, cols.size - 1, replace=False)] = True
            merged[mine], merged[~mine] = cols[1:], seq
            seq = np.concatenate([cols[:1], merged])
        conn.append(seq)
    return N.PInvSwitchboard(int(col0[-1]), np.concatenate(conn))


RAGGED_GROUPS = [[5], [9, 2, 14], [0, 15, 7, 3], [13, 1, 4, 6, 8, 10, 11, 12]]


def _ragged(rng, s1, p2, s2, p3, s3, p4, s4):
    sb0 = N.Rectangular2dSwitchboard((16, 8), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((8, 4), (2, 1), (2, 1), 6)
    sb2 = grouped_board(rng, [s1] * 16, RAGGED_GROUPS)
    l2 = N.Layer([_node(rng, s1 * len(g), p, s2) for g, p in zip(RAGGED_GROUPS, p2)])
    sb3 = N.Rectangular2dSwitchboard((4, 1), (2, 1), (2, 1), s2)
    sb4 = N.Rectangular2dSwitchboard((2, 1), (2, 1), (2, 1), s3)
    return [sb0, _layer(rng, 32, 4, 4, 6), sb1, _layer(rng, 16, 12, 8, s1), sb2, l2, sb3, _layer(rng, 2, 2 * s2, p3, s3),
            sb4, _layer(rng, 1, 2 * s3, p4, s4)]


def ragged_net(seed=0, p3=21):
    """Irregular hoisted links.  16 x 8 input, 32 nodes on 2x2 fields, 16 nodes on 2x1 merges (14 outputs each); a PInvSwitchboard
    hands those to FOUR parents of 1, 3, 4 and 8 children (RAGGED_GROUPS, read in that order, which is not ascending) and of 6, 12,
    14 and 10 columns: one z-tile, a K-block table padded to eight children.  Then two parents of p3 columns and one of 9.  With
    p3 = 21 stages 2, 3 and 4 are hoisted; with p3 = 18 or 20 the last tile of stage 3 holds 2 or 4 rows, the pass leaves that link
    alone and takes the ones below and above it."""
    return _ragged(np.random.default_rng(4400 + seed), 14, (6, 12, 14, 10), 24, p3, 9, 9, 5)


def ragged_wide_net(seed=0):
    """ragged_net's skeleton with parents of 6, 22, 40 and 33 columns over children of 44: the layer runs on three z-tiles, of which
    its parents fill 1, 2, 3 and 3 — the children of the narrow ones store zero tiles, and the parents add them.  Upper layers:
    two parents of 38 (of 40), one of 26 (of 30)."""
    return _ragged(np.random.default_rng(4500 + seed), 44, (6, 22, 40, 33), 40, 38, 30, 26, 12)


# (nodes, KiB of second-affine fragments per node) of the hoisted stages, bottom up: what HIGSFA_SUM_LDS is divided by to give
# k_stage_sum's node group (tests/test_hoist_plan_host.py pins them, tests/test_hoist_gpu.py::test_ragged_node_groups counts on them)
CHAIN_SUM_STAGES = [(16, 12), (8, 24), (4, 32), (2, 32), (1, 16)]
QUAD_SUM_STAGES = [(8, 8), (2, 12), (1, 6)]
RAGGED_SUM_STAGES = [(4, 4), (2, 4), (1, 2)]

ORDER_PROBE_SCALE = 2.0 ** 18


def order_probe_net(seed=0):
    """A net on which the ORDER of a hoisted parent's additions decides the result, so that the device shows it without recorded bits.
    Twelve input columns, six nodes on pairs of them, three nodes on pairs of those: C (node 0), A (node 1) and B (node 2).  A and
    B have the same weights, and so have the nodes below them; on rows whose columns 8..11 repeat columns 4..7
    (order_probe_rows) their outputs are the same bits.  One parent reads A's columns, then B's, then C's (first read: 1, 2, 0), with
    first-affine rows 2^18 R for A, -2^18 R for B, and no node of the net has a mean or a bias, so the parent's bias vector is zero:
        z = ((0 + t_A) + t_B) + t_C = t_C exactly, t_B = -t_A being 2^18 times C's size;
    in ascending order ((0 + t_C) + t_A) + t_B leaves t_C rounded to an ulp of t_A, 2^-6 of its size.  (The unhoisted plan, which
    multiplies x_A, x_B and x_C into one accumulator, has no such guarantee: this net is for the hoisted plans alone.)"""
    rng = np.random.default_rng(4700 + seed)

    def node(d_in, p, s, w1=None):
        w1 = rng.normal(size=(d_in, p)) / np.sqrt(d_in) if w1 is None else w1
        ex = N.GeneralExpansionNode(FUNCS, p)
        w2 = rng.normal(size=(ex.output_dim, s)) / np.sqrt(ex.output_dim)
        return N.FlowNode([N.PCANode(np.zeros(d_in), w1), ex, N.SFANode(np.zeros(ex.output_dim), w2)])

    def twin(nd):
        return N.FlowNode([N.PCANode(nd.flow[0].avg[0].copy(), nd.flow[0].v.copy()), N.GeneralExpansionNode(FUNCS, nd.flow[0].output_dim),
                           N.SFANode(nd.flow[2].avg[0].copy(), nd.flow[2].sf.copy())])

    l0 = [node(2, 2, 6) for _ in range(4)]
    l0 += [twin(l0[2]), twin(l0[3])]
    l1 = [node(12, 4, 6), node(12, 4, 6)]
    l1.append(twin(l1[1]))
    r = rng.normal(size=(6, 5)) / np.sqrt(18)
    w1 = np.concatenate([ORDER_PROBE_SCALE * r, -ORDER_PROBE_SCALE * r, rng.normal(size=(6, 5)) / np.sqrt(18)])
    sb2 = N.PInvSwitchboard(18, np.concatenate([np.arange(6, 12), np.arange(12, 18), np.arange(0, 6)]))
    return [N.Rectangular2dSwitchboard((12, 1), (2, 1), (2, 1), 1), N.Layer(l0), N.Rectangular2dSwitchboard((6, 1), (2, 1), (2, 1), 6), N.Layer(l1),
            sb2, N.Layer([node(18, 5, 7, w1)])]


def order_probe_rows(n, seed=0):
    x = np.random.default_rng(4750 + seed).normal(size=(n, 12)).astype(np.float32)
    x[:, 8:12] = x[:, 4:8]
    return x


HOIST_FUZZ_SEEDS = tuple(range(12))
HOIST_FUZZ_TAKEN = (0, 1, 2, 4, 6, 7, 8, 9, 10, 11)      # the seeds whose plan has a hoisted link (pinned by test_hoist_plan_host.py)


def hoist_fuzz_net(seed):
    """Random hierarchies without overlap, made for the hoist pass: above a layer of 2x2 fields every layer's children are dealt to
    parents in uneven groups of 1..8 through a PInvSwitchboard, in a random order of first read and with shuffled columns.  A
    parent is no wider than the narrowest of its children with probability 0.8 (one wider parent turns its layer's link off, so
    nets mix taken and refused links); widths whose last tile holds 1..4 rows are left to chance.  Children are 5..60 columns
    wide, expansions are one to three element-wise functions of helpers.fuzz_net's pool, at most five layers."""
    rng = np.random.default_rng(4600 + seed)
    pool = [N.identity, N.unsigned_08expo, N.signed_08expo, N.unsigned_expo(float(rng.uniform(0.5, 1.5))),
            N.signed_expo(float(rng.uniform(0.6, 1.2)))]

    def funcs():
        return [pool[int(i)] for i in rng.choice(len(pool), int(rng.integers(1, 4)), replace=False)]

    w, h = [(8, 8), (8, 4), (6, 6), (8, 6), (4, 4)][int(rng.integers(0, 5))]
    n = w * h
    sb = N.Rectangular2dSwitchboard((2 * w, 2 * h), (2, 2), (2, 2), 1)
    s = int(rng.integers(5, 13))
    fl = funcs()
    flow = [sb, N.Layer([_node(rng, 4, int(rng.integers(2, 5)), s, fl) for _ in range(n)])]
    widths = [s] * n
    for depth in range(1, 5):
        n = len(widths)
        tiles = (max(widths) + 15) // 16
        top = 3 if depth == 1 else min(8, 20 // tiles)     # a node's first-affine fragments (unhoisted) fit a workgroup's LDS
        order, groups = [int(v) for v in rng.permutation(n)], []
        while order:
            k = min(len(order), int(rng.integers(1, top + 1)))
            groups.append(order[:k])
            order = order[k:]
        s0 = int(rng.integers(5, 61))
        fl = funcs()
        nodes = []
        for grp in groups:
            narrow, d_in = min(widths[c] for c in grp), sum(widths[c] for c in grp)
            if rng.random() < 0.8:
                p = int(rng.integers(max(2, narrow - 12), narrow + 1))
            else:
                p = int(rng.integers(narrow + 1, min(narrow + 12, 60) + 1))
            nodes.append(_node(rng, d_in, min(p, d_in), max(5, s0 - int(rng.integers(0, 4))), fl))
        flow += [grouped_board(rng, widths, groups), N.Layer(nodes)]
        widths = [nd.output_dim for nd in nodes]
        if len(widths) == 1:
            break
    return flow


def igsfa_after_ordinary(seed=0):
    """An ordinary layer pair with an eligible link, but with iGSFA nodes on the parent side: not hoisted."""
    rng = np.random.default_rng(4300 + seed)
    sb0 = N.Rectangular2dSwitchboard((8, 8), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((4, 4), (2, 2), (2, 2), 6)
    sb2 = N.Rectangular2dSwitchboard((2, 2), (2, 1), (2, 1), 9)

    def ig(d_in, k, q):
        ex = N.GeneralExpansionNode(FUNCS, d_in)
        pca = helpers.rand_pca(rng, d_in, q)
        pca.avg = np.zeros_like(pca.avg)
        return N.iGSFANode(rng.normal(size=d_in), ex, helpers.rand_sfa(rng, ex.output_dim, k, N.GSFANode), rng.uniform(0.5, 2.0, size=k),
                           N.LinearRegressionNode(rng.normal(size=(k + 1, d_in)) / np.sqrt(k + 1)), pca, k)

    return [sb0, _layer(rng, 16, 4, 4, 6), sb1, _layer(rng, 4, 24, 8, 9), sb2, N.Layer([ig(18, 3, 4) for _ in range(2)])]


def build_driver(exe, extra_flags=()):
    """tests/hoist_plan_driver.cpp with plain g++ against hg_tree.cpp and the host-only plan unit (hg_fused_plan.cpp, hg_fused_call.cpp)
    only.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "hoist_plan_driver.cpp"), os.path.join(CSRC, "hg_tree.cpp"),
           os.path.join(CSRC, "hg_fused_plan.cpp"), os.path.join(CSRC, "hg_fused_call.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
