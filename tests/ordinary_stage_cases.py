"""Nets, batch sizes and expected launches of the ordinary-stage tests (tests/test_ordinary_stages_plan_host.py on the CPU,
tests/test_ordinary_stages_gpu.py on the device): k_stage at every instantiation of pick_stage, k_stage_splitm at every run-time
(mt1n, mt2n), both T and both REM forms, and the first-layer kernels k_stage0 / k_stage0p (csrc/hg_fused.hip), each at the batch sizes
where the call plan (csrc/hg_fused_call.cpp) changes route or shape.  Untrained: every weight is a seeded draw (helpers.rand_pca /
rand_sfa); no device code here.

What each (net, switches, rows) must launch is written out as literal tables (WANT_*): the host test holds plan_call to them through
the planner's stand-alone driver, the GPU test holds the debug lines of the device's launches to the same tables.  The tables were
written down when the nets were sized (with that driver, each family against the facts its nets were designed for:
test_the_tables_hold_the_design_of_each_family) and are data since: nothing here recomputes them with the rule under test.
If a generator or a rule drifts, decide which is wrong."""
import re

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import helpers
from tests.stage_shape_cases import covered_stages      # the stages the debug lines of one call name (every launch writes one)

SWEEP_ONLY = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0"}      # as tests/test_hoist_gpu.py
DEFAULT = {}

FS = [N.identity, N.unsigned_08expo]           # the form k_stage has a compile-time expansion for ("fs 1")
GENERAL = [N.identity, N.signed_expo(0.9)]     # the run-time expansion ("fs 0")
PAIRS = tuple((a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4))

# rows -> 16-row tiles 1, 2, 5, 13, 27, 51, 109, 163: a lone partly filled tile, odd tile counts (a T = 2 wave whose second tile is absent)
ROWS = (1, 17, 70, 195, 425, 805, 1738, 2600)
N_REF = ROWS[-1]


def tiles(rows):
    return (rows + 15) // 16


def inputs(d, seed, rows=N_REF):
    return np.random.default_rng(seed).normal(size=(rows, d)).astype(np.float32)


def _node(rng, d_in, p, s, funcs):
    seq = [helpers.rand_pca(rng, d_in, p, N.WhiteningNode)]
    if funcs is not None:      # None: a linear node, no expansion and no second affine
        ex = N.GeneralExpansionNode(funcs, p)
        seq += [ex, helpers.rand_sfa(rng, ex.output_dim, s)]
    return N.FlowNode(seq)


def _layer(rng, n, d_in, p, s, funcs):
    return N.Layer([_node(rng, d_in, p, s, funcs) for _ in range(n)])


def _bottom(rng, side, s=8):
    """Layer 0 of every two- and three-layer net here: (side / 2)^2 nodes on 2 x 2 fields, 4 -> 4 -> s with the identity alone as
    expansion — one function, so the front pair kernels never take layers 0 and 1 together (can_fuse01 asks for two) and the layer
    under test always has a launch of its own."""
    sb = N.Rectangular2dSwitchboard((side, side), (2, 2), (2, 2), 1)
    return [sb, _layer(rng, sb.output_channels, 4, 4, s, [N.identity])], sb.out_channels_xy


def ragged_dims(mt1, mt2):
    return 16 * mt1 - 3, 16 * mt2 - 5      # the last tile of each affine is ragged


def rem_dims(mt):
    return 16 * (mt - 1) + 3, 16 * (mt - 1) + 2      # the last tile of both affines holds 3 and 2 rows: the 4x4 remainder form


# ------------------------------------------------------------------------------------------------------------ family 1: ord11 .. ord44
def ord_net(mt1, mt2, funcs=FS, side=64, seed=0):
    """Two stages on a side x side input.  Layer 1, the layer under test: (side / 4)^2 nodes on 2 x 2 merges of 8-channel children
    (32 inputs, four K-blocks), p = 16 mt1 - 3, s = 16 mt2 - 5.  Every net of one side has the same input width."""
    rng = np.random.default_rng(8000 + 16 * mt1 + mt2 + (100 if funcs is GENERAL else 0) + side + 1000 * seed)
    flow, (w, h) = _bottom(rng, side)
    sb = N.Rectangular2dSwitchboard((w, h), (2, 2), (2, 2), 8)
    p, s = ragged_dims(mt1, mt2)
    return flow + [sb, _layer(rng, sb.output_channels, 32, p, s, funcs)]


# -------------------------------------------------------------------------------------------------- family 2: remainder tiles, prefetch, pk
REM_MERGES = {"A": ((2, 2), 144), "B": ((3, 1), 192), "C": ((2, 1), 288)}      # kind -> merge of layer 1, its nodes; K-blocks 4, 3, 2


def rem_net(kind, mt, funcs=FS, seed=0):
    """48 x 48 input, 576 layer-0 nodes; layer 1 with remainder tiles (rem_dims) on 2 x 2 ("A"), 3 x 1 ("B") or 2 x 1 ("C") merges:
    144, 192 or 288 nodes of four, three or two K-blocks.  (A and B are the whole-visit prefetch forms kbf 4 and kbf 3 at T = 2; C,
    of neither block count, is what reaches the plain remainder form at T = 2.)"""
    rng = np.random.default_rng(8200 + 10 * mt + "ABC".index(kind) + (100 if funcs is GENERAL else 0) + 1000 * seed)
    flow, (w, h) = _bottom(rng, 48)
    merge, n = REM_MERGES[kind]
    sb = N.Rectangular2dSwitchboard((w, h), merge, merge, 8)
    p, s = rem_dims(mt)
    assert sb.output_channels == n
    return flow + [sb, _layer(rng, n, sb.out_channel_dim, p, s, funcs)]


def pk_net(mt, funcs=FS, seed=0):
    """A third layer with packed input.  Layer 1 is rem_net("C", 2)'s: 288 nodes of 18 columns, whose two remainder rows are packed four
    nodes to a block.  Layer 2: 144 nodes on (2, 1) merges, each reading two children — a full tile each and their remainder rows
    from ONE packed block between them: three K-blocks, the packed one at position 1 (plan_slot_major).  Layer 2 has remainder
    tiles itself, mt tiles wide."""
    rng = np.random.default_rng(8300 + mt + (100 if funcs is GENERAL else 0) + 1000 * seed)
    flow, (w, h) = _bottom(rng, 48)
    sb1 = N.Rectangular2dSwitchboard((w, h), (2, 1), (2, 1), 8)
    p1, s1 = rem_dims(2)
    sb2 = N.Rectangular2dSwitchboard(sb1.out_channels_xy, (2, 1), (2, 1), s1)
    p2, s2 = rem_dims(mt)
    assert (sb1.output_channels, sb2.output_channels) == (288, 144)
    return flow + [sb1, _layer(rng, 288, 16, p1, s1, FS), sb2, _layer(rng, 144, 2 * s1, p2, s2, funcs)]


# ------------------------------------------------------------------------------------------------------ family 3: k_stage_splitm's extras
KB_MERGES = {8: (2, 4), 9: (3, 3), 16: (4, 4)}      # K-blocks of a node -> merge over the 12 x 12 grid of 16-channel children
KB_NODES = {8: 18, 9: 16, 16: 9, 17: 9}


def kb_net(kb1, seed=0):
    """24 x 24 input, 144 layer-0 nodes of 16 outputs (a K-block each); layer 1 reads kb1 of them per node: around k_stage_splitm's
    K-block batch of 8 — one full batch, a second batch of one block, two full batches, and (17: nine nodes that read children
    15 j .. 15 j + 16 through a PInvSwitchboard, neighbours sharing two; eight nodes or fewer would be the top-of-hierarchy
    launch's) a third batch of one."""
    rng = np.random.default_rng(8400 + kb1 + 1000 * seed)
    flow, (w, h) = _bottom(rng, 24, s=16)
    if kb1 in KB_MERGES:
        sb = N.Rectangular2dSwitchboard((w, h), KB_MERGES[kb1], KB_MERGES[kb1], 16)
        n = sb.output_channels
    else:
        n = 9
        sb = N.PInvSwitchboard(144 * 16, np.concatenate([np.arange(16 * 15 * j, 16 * (15 * j + kb1)) for j in range(n)]))
    assert n == KB_NODES[kb1]
    return flow + [sb, _layer(rng, n, 16 * kb1, 29, 27, FS)]


NF4 = [N.identity, N.unsigned_08expo, N.signed_08expo, N.unsigned_expo(1.2)]
NF3 = NF4[:3]


def nf_net(mt1, funcs, seed=0):
    """ord_net's 64-node twin with an expansion of len(funcs) functions: k_stage_splitm keeps mt1 x nf A fragments of the second affine
    in eight registers, so mt1 x nf <= 8 is its line."""
    rng = np.random.default_rng(8500 + 10 * mt1 + len(funcs) + 1000 * seed)
    flow, (w, h) = _bottom(rng, 32)
    sb = N.Rectangular2dSwitchboard((w, h), (2, 2), (2, 2), 8)
    return flow + [sb, _layer(rng, 64, 32, 16 * mt1 - 3, 27, funcs)]


def linear_net(seed=0):
    """ord_net's 64-node twin with layer 1 linear (one affine of 29 columns, no expansion): k_stage_splitm stores z and returns before
    its barrier on every path."""
    rng = np.random.default_rng(8600 + 1000 * seed)
    flow, (w, h) = _bottom(rng, 32)
    sb = N.Rectangular2dSwitchboard((w, h), (2, 2), (2, 2), 8)
    return flow + [sb, _layer(rng, 64, 32, 29, 0, None)]


# ------------------------------------------------------------------------------------------------------ family 4: the first-layer kernels
def front_net(mt1, mt2, seed=0):
    """One layer: 16 nodes on 4 x 4 fields of a 16 x 16 input (one K-block), p = 16 mt1 - 3, s = 16 mt2 - 5."""
    rng = np.random.default_rng(8700 + 16 * mt1 + mt2 + 1000 * seed)
    sb = N.Rectangular2dSwitchboard((16, 16), (4, 4), (4, 4), 1)
    p, s = ragged_dims(mt1, mt2)
    return [sb, _layer(rng, 16, 16, p, s, FS)]


# ------------------------------------------------------------------------------------------------------------------------- the list
NO_REM4 = {"HIGSFA_NO_REM4": "1"}
NO_SOA = {"HIGSFA_NO_SOA": "1"}
NO_PACK = {"HIGSFA_NO_PACK": "1"}
ROWS_SPLITM = (1, 17, 33, 49)                  # family 1 under the default switches: one tile, two, three (T = 2 with an absent second tile)
ROWS_ORD_D = ROWS_SPLITM + (70, 2600)       # and across the line to the sweep: 4 x 1 at 5 tiles, 8 x 2 at 163
ROWS_SMALL = (1, 17, 70, 195, 425)         # 64-node layers: k_stage_splitm up to 13 tiles, the sweep at 27
ROWS_REM = (1, 17, 33, 49, 70, 195)            # remainder-tile layers under the default switches: 1, 2, 3, 5 and 13 tiles
ROWS_KB = (1, 17, 520, 1030)               # 1, 2, 33 and 65 tiles: T = 2 needs 2 x 256 / nodes tiles


def nets():
    """{name: (family, constructor, switches the handle is planned under, batch sizes)}.  A name ends in ":d" where the handle is
    planned under the default switches (k_stage_splitm takes small batches); every other handle is planned under SWEEP_ONLY."""
    out = {}
    for a, b in PAIRS:
        out["ord%d%d" % (a, b)] = (1, (lambda a=a, b=b: ord_net(a, b)), SWEEP_ONLY, ROWS)
    for a in (3, 4):
        out["ordgen%d%d" % (a, a)] = (1, (lambda a=a: ord_net(a, a, GENERAL)), SWEEP_ONLY, ROWS)
    for kind in "AB":
        for mt in (2, 3):
            for tag, funcs in (("", FS), ("+gen", GENERAL)):
                for tag2, env in (("", {}), ("+norem4", NO_REM4)):
                    out["rem%s%d%s%s" % (kind, mt, tag, tag2)] = (2, (lambda kind=kind, mt=mt, funcs=funcs: rem_net(kind, mt, funcs)), dict(SWEEP_ONLY, **env), ROWS)
    for mt in (2, 3):
        out["remC%d" % mt] = (2, (lambda mt=mt: rem_net("C", mt)), SWEEP_ONLY, ROWS)
    for mt in (2, 3):
        for tag, funcs in (("", FS), ("+gen", GENERAL)):
            for tag2, env in (("", {}), ("+nosoa", NO_SOA), ("+nopack", NO_PACK)):
                out["pk%d%s%s" % (mt, tag, tag2)] = (2, (lambda mt=mt, funcs=funcs: pk_net(mt, funcs)), dict(SWEEP_ONLY, **env), ROWS)
    for a, b in PAIRS:
        out["ord%d%d:d" % (a, b)] = (3, (lambda a=a, b=b: ord_net(a, b)), DEFAULT, ROWS_ORD_D)
    for a, b in ((1, 1), (2, 3), (3, 2), (4, 4)):
        out["twin%d%d:d" % (a, b)] = (3, (lambda a=a, b=b: ord_net(a, b, side=32)), DEFAULT, ROWS_SMALL)
    for kind in "ABC":
        for mt in (2, 3):
            out["rem%s%d:d" % (kind, mt)] = (3, (lambda kind=kind, mt=mt: rem_net(kind, mt)), DEFAULT, ROWS_REM)
    for kb in (8, 9, 16, 17):
        out["kb%d:d" % kb] = (3, (lambda kb=kb: kb_net(kb)), DEFAULT, ROWS_KB)
    out["nf24:d"] = (3, (lambda: nf_net(2, NF4)), DEFAULT, ROWS_SMALL)
    out["nf33:d"] = (3, (lambda: nf_net(3, NF3)), DEFAULT, ROWS_SMALL)
    out["linear:d"] = (3, linear_net, DEFAULT, ROWS_SMALL)
    return out


# -------------------------------------------------------------------------------------------------- what a call must launch, by design
# The node-group sweep's (waves, tiles per wave, tile groups, tile parts) by node groups and batch tiles, tile parts at one resident
# workgroup per CU (the stand-alone driver's --occ 1; on the device they follow the occupancy the runtime reports, so the GPU test
# reads them from the line and holds them to tile_parts at the line's own occupancy).  Literal: the first of 8x2, 8x1, 4x1 with
# waves x tiles <= batch tiles and tile groups x node groups >= 256, else 4x1 halved down to the batch — written out, not computed here.
SWEEP_SHAPES = {
    7: {27: (4, 1, 7, 7)},
    8: {27: (4, 1, 7, 7), 65: (4, 1, 17, 17)},
    9: {65: (4, 1, 17, 9)},
    22: {27: (4, 1, 7, 7)},
    26: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 7), 51: (4, 1, 13, 7), 109: (8, 1, 14, 7), 163: (8, 2, 11, 6)},
    32: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 7), 51: (4, 1, 13, 7), 109: (8, 1, 14, 7), 163: (8, 2, 11, 6)},
    36: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 4), 51: (4, 1, 13, 5), 109: (8, 1, 14, 5), 163: (8, 2, 11, 6)},
    43: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 4), 51: (8, 1, 7, 4), 109: (8, 2, 7, 4), 163: (8, 2, 11, 4)},
    48: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 4), 51: (8, 1, 7, 4), 109: (8, 2, 7, 4), 163: (8, 2, 11, 4)},
    52: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 4), 51: (8, 1, 7, 4), 109: (8, 2, 7, 4), 163: (8, 2, 11, 4)},
    58: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 3: (2, 1, 2, 2), 4: (4, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (4, 1, 7, 4), 51: (8, 1, 7, 4), 109: (8, 2, 7, 4), 163: (8, 2, 11, 4)},
    64: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 4), 27: (8, 1, 4, 4), 51: (8, 2, 4, 4), 109: (8, 2, 7, 4), 163: (8, 2, 11, 4)},
    72: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 2), 27: (8, 1, 4, 2), 51: (8, 2, 4, 2), 109: (8, 2, 7, 7), 163: (8, 2, 11, 3)},
    86: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 2), 27: (8, 1, 4, 2), 51: (8, 2, 4, 2), 109: (8, 2, 7, 7), 163: (8, 2, 11, 11)},
    96: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (4, 1, 4, 2), 27: (8, 1, 4, 2), 51: (8, 2, 4, 2), 109: (8, 2, 7, 7), 163: (8, 2, 11, 2)},
    128: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 2), 13: (8, 1, 2, 2), 27: (8, 2, 2, 2), 51: (8, 2, 4, 2), 109: (8, 2, 7, 2), 163: (8, 2, 11, 2)},
    144: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 3: (2, 1, 2, 1), 4: (4, 1, 1, 1), 5: (4, 1, 2, 1), 13: (8, 1, 2, 1), 27: (8, 2, 2, 1), 51: (8, 2, 4, 4), 109: (8, 2, 7, 7), 163: (8, 2, 11, 3)},
    256: {1: (1, 1, 1, 1), 2: (2, 1, 1, 1), 5: (4, 1, 2, 1), 13: (8, 1, 2, 1), 27: (8, 2, 2, 1), 51: (8, 2, 4, 1), 109: (8, 2, 7, 1), 163: (8, 2, 11, 1)},
}

# Per net, the stages under test (every stage above the first-layer kernel).  For the node-group sweep: K-blocks, nodes per group,
# node groups, compile-time expansion, remainder tiles, the packed K-block, and kbf2, the whole-visit prefetch at T = 2 (at T = 1 it
# is always 0).  For k_stage_splitm: its waves and REM form (rem4m), and `routes`, "tiles:route" per batch size of the net —
# splitm1 / splitm2 are k_stage_splitm at T = 1 / 2.  A net without `routes` runs the sweep at every size.
STAGES = {
    'ord11': [dict(stage=1, nodes=256, mt=(1, 1), kb1=4, npg=10, ng=26, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord12': [dict(stage=1, nodes=256, mt=(1, 2), kb1=4, npg=8, ng=32, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord13': [dict(stage=1, nodes=256, mt=(1, 3), kb1=4, npg=6, ng=43, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord14': [dict(stage=1, nodes=256, mt=(1, 4), kb1=4, npg=5, ng=52, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord21': [dict(stage=1, nodes=256, mt=(2, 1), kb1=4, npg=5, ng=52, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord22': [dict(stage=1, nodes=256, mt=(2, 2), kb1=4, npg=4, ng=64, fs=1, rem4=0, pk=-1, kbf2=4)],
    'ord23': [dict(stage=1, nodes=256, mt=(2, 3), kb1=4, npg=3, ng=86, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord24': [dict(stage=1, nodes=256, mt=(2, 4), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord31': [dict(stage=1, nodes=256, mt=(3, 1), kb1=4, npg=3, ng=86, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord32': [dict(stage=1, nodes=256, mt=(3, 2), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord33': [dict(stage=1, nodes=256, mt=(3, 3), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=4)],
    'ord34': [dict(stage=1, nodes=256, mt=(3, 4), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord41': [dict(stage=1, nodes=256, mt=(4, 1), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord42': [dict(stage=1, nodes=256, mt=(4, 2), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord43': [dict(stage=1, nodes=256, mt=(4, 3), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ord44': [dict(stage=1, nodes=256, mt=(4, 4), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0)],
    'ordgen33': [dict(stage=1, nodes=256, mt=(3, 3), kb1=4, npg=2, ng=128, fs=0, rem4=0, pk=-1, kbf2=4)],
    'ordgen44': [dict(stage=1, nodes=256, mt=(4, 4), kb1=4, npg=1, ng=256, fs=0, rem4=0, pk=-1, kbf2=0)],
    'remA2': [dict(stage=1, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=1, rem4=1, pk=-1, kbf2=4)],
    'remA2+norem4': [dict(stage=1, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=1, rem4=0, pk=-1, kbf2=4)],
    'remA2+gen': [dict(stage=1, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=0, rem4=1, pk=-1, kbf2=4)],
    'remA2+gen+norem4': [dict(stage=1, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=0, rem4=0, pk=-1, kbf2=4)],
    'remA3': [dict(stage=1, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=1, rem4=1, pk=-1, kbf2=4)],
    'remA3+norem4': [dict(stage=1, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=1, rem4=0, pk=-1, kbf2=4)],
    'remA3+gen': [dict(stage=1, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=0, rem4=1, pk=-1, kbf2=4)],
    'remA3+gen+norem4': [dict(stage=1, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=0, rem4=0, pk=-1, kbf2=4)],
    'remB2': [dict(stage=1, nodes=192, mt=(2, 2), kb1=3, npg=4, ng=48, fs=1, rem4=1, pk=-1, kbf2=3)],
    'remB2+norem4': [dict(stage=1, nodes=192, mt=(2, 2), kb1=3, npg=4, ng=48, fs=1, rem4=0, pk=-1, kbf2=0)],
    'remB2+gen': [dict(stage=1, nodes=192, mt=(2, 2), kb1=3, npg=4, ng=48, fs=0, rem4=1, pk=-1, kbf2=3)],
    'remB2+gen+norem4': [dict(stage=1, nodes=192, mt=(2, 2), kb1=3, npg=4, ng=48, fs=0, rem4=0, pk=-1, kbf2=0)],
    'remB3': [dict(stage=1, nodes=192, mt=(3, 3), kb1=3, npg=2, ng=96, fs=1, rem4=1, pk=-1, kbf2=3)],
    'remB3+norem4': [dict(stage=1, nodes=192, mt=(3, 3), kb1=3, npg=2, ng=96, fs=1, rem4=0, pk=-1, kbf2=0)],
    'remB3+gen': [dict(stage=1, nodes=192, mt=(3, 3), kb1=3, npg=2, ng=96, fs=0, rem4=1, pk=-1, kbf2=3)],
    'remB3+gen+norem4': [dict(stage=1, nodes=192, mt=(3, 3), kb1=3, npg=2, ng=96, fs=0, rem4=0, pk=-1, kbf2=0)],
    'remC2': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0)],
    'remC3': [dict(stage=1, nodes=288, mt=(3, 3), kb1=2, npg=2, ng=144, fs=1, rem4=1, pk=-1, kbf2=0)],
    'pk2': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=3, npg=4, ng=36, fs=1, rem4=1, pk=1, kbf2=3)],
    'pk2+nosoa': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=3, npg=4, ng=36, fs=1, rem4=1, pk=-1, kbf2=3)],
    'pk2+nopack': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=1, rem4=1, pk=-1, kbf2=4)],
    'pk2+gen': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=3, npg=4, ng=36, fs=0, rem4=1, pk=1, kbf2=3)],
    'pk2+gen+nosoa': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=3, npg=4, ng=36, fs=0, rem4=1, pk=-1, kbf2=3)],
    'pk2+gen+nopack': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=0, rem4=1, pk=-1, kbf2=4)],
    'pk3': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=3, npg=2, ng=72, fs=1, rem4=1, pk=1, kbf2=3)],
    'pk3+nosoa': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=3, npg=2, ng=72, fs=1, rem4=1, pk=-1, kbf2=3)],
    'pk3+nopack': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=1, rem4=1, pk=-1, kbf2=4)],
    'pk3+gen': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=3, npg=2, ng=72, fs=0, rem4=1, pk=1, kbf2=3)],
    'pk3+gen+nosoa': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=3, npg=2, ng=72, fs=0, rem4=1, pk=-1, kbf2=3)],
    'pk3+gen+nopack': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=0),
        dict(stage=2, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=0, rem4=1, pk=-1, kbf2=4)],
    'ord11:d': [dict(stage=1, nodes=256, mt=(1, 1), kb1=4, npg=10, ng=26, fs=1, rem4=0, pk=-1, kbf2=0, waves=1, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord12:d': [dict(stage=1, nodes=256, mt=(1, 2), kb1=4, npg=8, ng=32, fs=1, rem4=0, pk=-1, kbf2=0, waves=2, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord13:d': [dict(stage=1, nodes=256, mt=(1, 3), kb1=4, npg=6, ng=43, fs=1, rem4=0, pk=-1, kbf2=0, waves=3, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord14:d': [dict(stage=1, nodes=256, mt=(1, 4), kb1=4, npg=5, ng=52, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord21:d': [dict(stage=1, nodes=256, mt=(2, 1), kb1=4, npg=5, ng=52, fs=1, rem4=0, pk=-1, kbf2=0, waves=2, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord22:d': [dict(stage=1, nodes=256, mt=(2, 2), kb1=4, npg=4, ng=64, fs=1, rem4=0, pk=-1, kbf2=4, waves=2, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord23:d': [dict(stage=1, nodes=256, mt=(2, 3), kb1=4, npg=3, ng=86, fs=1, rem4=0, pk=-1, kbf2=0, waves=3, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord24:d': [dict(stage=1, nodes=256, mt=(2, 4), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord31:d': [dict(stage=1, nodes=256, mt=(3, 1), kb1=4, npg=3, ng=86, fs=1, rem4=0, pk=-1, kbf2=0, waves=3, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord32:d': [dict(stage=1, nodes=256, mt=(3, 2), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0, waves=3, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord33:d': [dict(stage=1, nodes=256, mt=(3, 3), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=4, waves=3, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord34:d': [dict(stage=1, nodes=256, mt=(3, 4), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord41:d': [dict(stage=1, nodes=256, mt=(4, 1), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord42:d': [dict(stage=1, nodes=256, mt=(4, 2), kb1=4, npg=2, ng=128, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord43:d': [dict(stage=1, nodes=256, mt=(4, 3), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'ord44:d': [dict(stage=1, nodes=256, mt=(4, 4), kb1=4, npg=1, ng=256, fs=1, rem4=0, pk=-1, kbf2=0, waves=4, rem4m=0, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 163:sweep')],
    'twin11:d': [dict(stage=1, nodes=64, mt=(1, 1), kb1=4, npg=10, ng=7, fs=1, rem4=0, pk=-1, kbf2=None, waves=1, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
    'twin23:d': [dict(stage=1, nodes=64, mt=(2, 3), kb1=4, npg=3, ng=22, fs=1, rem4=0, pk=-1, kbf2=None, waves=3, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
    'twin32:d': [dict(stage=1, nodes=64, mt=(3, 2), kb1=4, npg=2, ng=32, fs=1, rem4=0, pk=-1, kbf2=None, waves=3, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
    'twin44:d': [dict(stage=1, nodes=64, mt=(4, 4), kb1=4, npg=1, ng=64, fs=1, rem4=0, pk=-1, kbf2=None, waves=4, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
    'remA2:d': [dict(stage=1, nodes=144, mt=(2, 2), kb1=4, npg=4, ng=36, fs=1, rem4=1, pk=-1, kbf2=None, waves=2, rem4m=1, routes='1:splitm1 2:splitm1 3:splitm2 4:splitm2 5:splitm2 13:sweep')],
    'remA3:d': [dict(stage=1, nodes=144, mt=(3, 3), kb1=4, npg=2, ng=72, fs=1, rem4=1, pk=-1, kbf2=None, waves=3, rem4m=1, routes='1:splitm1 2:splitm1 3:splitm2 4:splitm2 5:splitm2 13:sweep')],
    'remB2:d': [dict(stage=1, nodes=192, mt=(2, 2), kb1=3, npg=4, ng=48, fs=1, rem4=1, pk=-1, kbf2=None, waves=2, rem4m=1, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 13:sweep')],
    'remB3:d': [dict(stage=1, nodes=192, mt=(3, 3), kb1=3, npg=2, ng=96, fs=1, rem4=1, pk=-1, kbf2=None, waves=3, rem4m=1, routes='1:splitm1 2:splitm2 3:splitm2 4:splitm2 5:sweep 13:sweep')],
    'remC2:d': [dict(stage=1, nodes=288, mt=(2, 2), kb1=2, npg=5, ng=58, fs=1, rem4=1, pk=-1, kbf2=None, waves=2, rem4m=1, routes='1:splitm2 2:splitm2 3:sweep 4:sweep 5:sweep 13:sweep')],
    'remC3:d': [dict(stage=1, nodes=288, mt=(3, 3), kb1=2, npg=2, ng=144, fs=1, rem4=1, pk=-1, kbf2=None, waves=3, rem4m=1, routes='1:splitm2 2:splitm2 3:sweep 4:sweep 5:sweep 13:sweep')],
    'kb8:d': [dict(stage=1, nodes=18, mt=(2, 2), kb1=8, npg=2, ng=9, fs=1, rem4=0, pk=-1, kbf2=None, waves=2, rem4m=0, routes='1:splitm1 2:splitm1 33:splitm2 65:sweep')],
    'kb9:d': [dict(stage=1, nodes=16, mt=(2, 2), kb1=9, npg=2, ng=8, fs=1, rem4=0, pk=-1, kbf2=None, waves=2, rem4m=0, routes='1:splitm1 2:splitm1 33:splitm2 65:sweep')],
    'kb16:d': [dict(stage=1, nodes=9, mt=(2, 2), waves=2, rem4m=0, routes='1:splitm1 2:splitm1 33:splitm1 65:splitm2')],
    'kb17:d': [dict(stage=1, nodes=9, mt=(2, 2), waves=2, rem4m=0, routes='1:splitm1 2:splitm1 33:splitm1 65:splitm2')],
    'nf24:d': [dict(stage=1, nodes=64, mt=(2, 2), kb1=4, npg=2, ng=32, fs=0, rem4=0, pk=-1, kbf2=None, waves=2, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
    'nf33:d': [dict(stage=1, nodes=64, mt=(3, 2), kb1=4, npg=2, ng=32, fs=0, rem4=0, pk=-1, kbf2=None)],
    'linear:d': [dict(stage=1, nodes=64, mt=(2, 1), kb1=4, npg=8, ng=8, fs=0, rem4=0, pk=-1, kbf2=None, waves=2, rem4m=0, routes='1:splitm1 2:splitm1 5:splitm1 13:splitm2 27:sweep')],
}


SWEEP_LINE = (r"\[sweep stage (\d+)\] nodes (\d+) mt1 (\d+) mt2 (\d+) kb1 (\d+) shape (\d+)x(\d+) npg (\d+) node_groups (\d+) tile_groups (\d+) parts (\d+) "
              r"occ (\d+) lds (\d+) kbf (\d+) fs (\d+) rem4 (\d+) pk (-?\d+) hoisted (\d+) summed_in (\d+) pair_chunks (\d+)")
SPLITM_LINE = r"\[splitm stage (\d+)\] nodes (\d+) mt1 (\d+) mt2 (\d+) rem4 (\d+) tiles (\d+) waves (\d+) lds (\d+) blocks (\d+)"
FRONT0_LINE = (r"\[front0\] persistent (\d) tiles (\d+) vec4 (\d) occ (\d+) threads (\d+) lds (\d+) chunks (\d+) tile_groups (\d+) tile_parts (\d+) "
               r"blocks (\d+)")


def launches(text):
    """The launches that the lines of `text` name (a device's stderr under HIGSFA_DEBUG, or the driver's step lines), in order: a
    dict per sweep, split-m and first-layer line.  Any other line that names a stage of an ordinary route must not go unread."""
    out = []
    for ln in text.splitlines():
        m = re.search(SWEEP_LINE, ln)
        if m:
            v = [int(g) for g in m.groups()]
            out.append(dict(route="sweep", stage=v[0], nodes=v[1], mt=(v[2], v[3]), kb1=v[4], shape=(v[5], v[6]), npg=v[7], ng=v[8], tile_groups=v[9],
                            parts=v[10], occ=v[11], kbf=v[13], fs=v[14], rem4=v[15], pk=v[16], hoisted=v[17], summed_in=v[18], pair_chunks=v[19]))
            continue
        m = re.search(SPLITM_LINE, ln)
        if m:
            v = [int(g) for g in m.groups()]
            out.append(dict(route="splitm", stage=v[0], nodes=v[1], mt=(v[2], v[3]), rem4=v[4], T=v[5], waves=v[6], blocks=v[8]))
            continue
        m = re.search(FRONT0_LINE, ln)
        if m:
            v = [int(g) for g in m.groups()]
            out.append(dict(route="front0", stage=0, persistent=v[0], T=v[1], vec4=v[2], tile_groups=v[7]))
            continue
        assert "[sweep stage" not in ln and "[splitm stage" not in ln and "[front0]" not in ln, ln
    return out


def want(name, rows):
    """What the sweep and split-m lines of ONE call of `rows` rows of the net must say, stage by stage, from the tables above."""
    t = tiles(rows)
    out = []
    for s in STAGES[name]:
        route = dict(e.split(":") for e in s["routes"].split())[str(t)] if "routes" in s else "sweep"
        if route == "sweep":
            nw, T, tg, parts = SWEEP_SHAPES[s["ng"]][t]
            out.append(dict(route="sweep", stage=s["stage"], nodes=s["nodes"], mt=s["mt"], kb1=s["kb1"], shape=(nw, T), npg=s["npg"], ng=s["ng"], tile_groups=tg,
                            parts=parts, kbf=s["kbf2"] if T == 2 else 0, fs=s["fs"], rem4=s["rem4"], pk=s["pk"], hoisted=0, summed_in=0, pair_chunks=0))
        else:
            T = int(route[-1])
            out.append(dict(route="splitm", stage=s["stage"], nodes=s["nodes"], mt=s["mt"], rem4=s["rem4m"], T=T, waves=s["waves"],
                            blocks=s["nodes"] * ((t + T - 1) // T)))
    return out


def held(got, wanted, parts=True):
    """The launches `got` are the launches `wanted`, field by field (`parts`: tile parts too, where the occupancy is the driver's one
    workgroup per CU; at any occupancy they are tile_parts of the line's own figures)."""
    assert all(g["parts"] == tile_parts(g["ng"], g["tile_groups"], g["occ"]) for g in got if g["route"] == "sweep"), got
    skip = ("occ",) if parts else ("occ", "parts")
    return [{k: v for k, v in g.items() if k not in skip} for g in got] == [{k: v for k, v in w.items() if k not in skip} for w in wanted]


def instantiation(l):
    """The kernel a sweep or split-m line stands for: pick_stage's table (csrc/hg_fused.hip; launch_stage passes the line's fields) and
    launch_splitm's, restated.  k_stage<MT1, MT2, T, REM, KBF, FS, PK> as a tuple, k_stage_splitm<T, REM> with its run-time tile counts."""
    if l["route"] == "splitm":
        return ("k_stage_splitm", l["T"], bool(l["rem4"]), l["mt"])
    (a, b), T, rem, kbf, fs, pk = l["mt"], l["shape"][1], bool(l["rem4"]), l["kbf"], bool(l["fs"]), l["pk"]
    sq = a == b and a in (2, 3)
    if pk >= 0:
        if kbf == 3 and pk == 1 and T == 2 and rem and sq:
            return ("k_stage", a, b, 2, True, 3, fs and a == 3, 1)
        return ("k_stage", a, b, T, rem and sq, 0, False, -1)      # launch_stage falls back to the streaming form, which decodes every packed block
    if fs:
        if kbf == 3 and T == 2 and rem and (a, b) == (3, 3):
            return ("k_stage", 3, 3, 2, True, 3, True, -1)
        if kbf == 4 and T == 2 and not rem and (a, b) == (3, 3):
            return ("k_stage", 3, 3, 2, False, 4, True, -1)
        if kbf == 0 and not rem and (a, b) == (4, 4):
            return ("k_stage", 4, 4, T, False, 0, True, -1)
    if kbf == 4 and T == 2 and sq:
        return ("k_stage", a, b, 2, rem, 4, False, -1)
    if kbf == 3 and T == 2 and rem and sq:
        return ("k_stage", a, b, 2, True, 3, False, -1)
    if rem and sq:
        return ("k_stage", a, b, T, True, 0, False, -1)
    return ("k_stage", a, b, T, False, 0, False, -1)


def pick_stage_instantiations():
    """Every k_stage instantiation pick_stage can return, written out from its source: 32 plain, 4 remainder-tile, 2 + 4 whole-visit
    prefetch of three and four K-blocks, 4 with the expansion at compile time, 3 with a packed K-block."""
    out = {("k_stage", a, b, t, False, 0, False, -1) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4) for t in (1, 2)}
    out |= {("k_stage", m, m, t, True, 0, False, -1) for m in (2, 3) for t in (1, 2)}
    out |= {("k_stage", m, m, 2, True, 3, False, -1) for m in (2, 3)}
    out |= {("k_stage", m, m, 2, rem, 4, False, -1) for m in (2, 3) for rem in (False, True)}
    out |= {("k_stage", 3, 3, 2, True, 3, True, -1), ("k_stage", 3, 3, 2, False, 4, True, -1), ("k_stage", 4, 4, 1, False, 0, True, -1),
            ("k_stage", 4, 4, 2, False, 0, True, -1)}
    out |= {("k_stage", 3, 3, 2, True, 3, True, 1), ("k_stage", 3, 3, 2, True, 3, False, 1), ("k_stage", 2, 2, 2, True, 3, False, 1)}
    assert len(out) == 49
    return out


def sweep_shape(n_tiles, n_groups):
    """stage_sweep_shape restated: the first of 8x2, 8x1, 4x2, 4x1 with waves x tiles <= batch tiles and tile groups x node groups >=
    256, else 4x1; the waves halved while the workgroup holds more tiles than the batch."""
    nw, t = 4, 1
    for a, b in ((8, 2), (8, 1), (4, 2), (4, 1)):
        if a * b <= n_tiles and -(-n_tiles // (a * b)) * n_groups >= 256:
            nw, t = a, b
            break
    while nw * t > max(n_tiles, 1) and nw > 1:
        nw >>= 1
    return nw, t


def tile_parts(n_groups, tile_groups, occ):
    """sweep_tile_parts restated: the smallest number of parts of the least cost, cost(parts) = rounds x (0.35 + tile groups per part),
    rounds = ceil(node groups padded to 8 x parts / (256 CUs x occ resident workgroups))."""
    g8 = (n_groups + 7) // 8 * 8
    best, parts = None, 1
    for pp in range(1, tile_groups + 1):
        cost = -(-g8 * pp // (256 * occ)) * (0.35 + -(-tile_groups // pp))
        if best is None or cost < best - 1e-9:
            best, parts = cost, pp
    return parts


# family 4: what the "[front0]" line must say by tile widths.  Four tiles per workgroup from four batch tiles on where mt1 x mt2 <= 4,
# else one; the persistent kernel k_stage0p at (1, 1) alone (and only with 16-byte loads)
FRONT_ROWS = (48, 64, 80, 70)      # 3, 4 and 5 tiles, and 5 with a ragged last one
FRONT_T4 = ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (3, 1), (4, 1))
FRONT_DTYPES = ("uint8", "float32", "float64")


def front_want(pair, rows, vec4=True):
    t = tiles(rows)
    T = 4 if t >= 4 and pair in FRONT_T4 else 1
    return dict(route="front0", stage=0, persistent=int(T == 4 and pair == (1, 1) and vec4), T=T, vec4=int(vec4), tile_groups=(t + T - 1) // T)
