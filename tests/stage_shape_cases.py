"""Nets and batch sizes for the product and iGSFA stage tests (tests/test_stage_shapes_plan_host.py on the CPU,
tests/test_stage_shapes_gpu.py on the device): every tile width k_stage_prod, k_igsfa and k_igfold are instantiated for, at the
batch sizes where launch_prod / launch_igsfa (csrc/hg_fused.hip) change the launch shape.  Untrained: every weight is a seeded draw
(helpers.rand_pca / rand_sfa); no device code here.

What each net is sized for is written down as data (PROD_WANT, IG_UNFOLDED, IG_FOLDED, ...): the host test holds the planner to it,
the GPU test holds the debug lines of the launches to the shapes derived from it.  If a generator drifts, change the net, not these."""
import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import helpers

# rows -> 16-row tiles 1, 2, 5, 13, 27, 51, 109: a lone partly filled tile, odd tile counts, and (sweep_shape's rule: the first
# candidate nw x T with nw * T <= tiles and ceil(tiles / (nw * T)) * groups >= 256) every shape of a 64-node layer
ROWS = (1, 17, 70, 195, 425, 805, 1738)
N_REF = ROWS[-1]


def tiles(rows):
    return (rows + 15) // 16


def inputs(nodes, seed, rows=N_REF):
    return np.random.default_rng(seed).normal(size=(rows, nodes[0].input_dim)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- product stages
PROD_FUNCS = [N.identity, N.sel_exp(6, N.QT), N.pair_prodsadj_ex(1, "offset"), N.unsigned_08expo]
PROD_PAIRS = tuple((a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4))


def prod_dims(mt1, mt2):
    return 16 * mt1 - 3, 16 * mt2 - 5      # the last tile of each affine is ragged


def prod_neb(p):
    """16-column blocks of product columns of a node of width p under PROD_FUNCS: QT of the first 6, then x_i x_{i+1}."""
    return (21 + (p - 1) + 15) // 16


def _prod_node(rng, d_in, p, s, head=None, clip=4.0):
    ex = N.GeneralExpansionNode(PROD_FUNCS, p)
    seq = [helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, N.CutoffNode(ex.output_dim, -clip, clip),      # the clip keeps the untrained products bounded
           helpers.rand_sfa(rng, ex.output_dim, s)]
    if head:
        seq.append(N.HeadNode(s, head))
    return N.FlowNode(seq)


def prod_layer_net(mt1, mt2, n_nodes=64, seed=0):
    """One product layer of 64 nodes on a 16 x 16 input with 2 x 2 fields; p = 16 mt1 - 3 and s = 16 mt2 - 5, so the pair products
    x_i x_{i+1} read every feature up to p - 1 (etab byte offsets up to feature 60) and the per-wave z image in LDS is mt1 tiles."""
    assert n_nodes == 64
    rng = np.random.default_rng(6000 + 16 * mt1 + mt2 + 100 * seed)
    p, s = prod_dims(mt1, mt2)
    sb = N.Rectangular2dSwitchboard((16, 16), (2, 2), (2, 2), 1)
    return [sb, N.Layer([_prod_node(rng, 4, p, s) for _ in range(sb.output_channels)])]


def prod_shape(n_tiles, n_nodes):
    """launch_prod's (waves, tiles per wave), restated from sweep_shape: candidates 8x2, 4x2, 4x1 over single nodes, default 4x1,
    shrunk to the batch."""
    nw, t = 4, 1
    for a, b in ((8, 2), (4, 2), (4, 1)):
        if a * b <= n_tiles and -(-n_tiles // (a * b)) * n_nodes >= 256:
            nw, t = a, b
            break
    while nw * t > max(n_tiles, 1) and nw > 1:
        nw >>= 1
    return nw, t


# rows -> shape of a 64-node product layer: the shrunk default twice, the default, 4x1 chosen, 4x2 and 8x2 with an odd tile count
PROD_SHAPES_64 = {1: (1, 1), 17: (2, 1), 70: (4, 1), 195: (4, 1), 425: (4, 2), 805: (8, 2), 1738: (8, 2)}

PROD_UNEVEN_P = (12, 20)      # alternating widths of layer 0: one and two z-tiles, 11 and 19 pair products


def prod_uneven_net(seed=0):
    """A two-layer product hierarchy.  Layer 0: 64 nodes on a 32 x 8 input whose widths alternate between 12 and 20 — the narrow
    nodes' second affine is scattered into the 20-wide node's column table (columns they lack get zero rows).  Its nodes take
    9.3 KiB of LDS each, so launch_prod's node group is 2, 3 or 4 with the shape: 3 (at 4 x 2, 425 rows) leaves a last group of one.
    Layer 1: 6 nodes on overlapping fields (6 x 4 children at stride 2: 24 K-blocks per node, every child but the outer ones read by
    three parents), 14 outputs cut to 11 by a HeadNode."""
    rng = np.random.default_rng(6100 + seed)
    sb0 = N.Rectangular2dSwitchboard((32, 8), (2, 2), (2, 2), 1)
    l0 = N.Layer([_prod_node(rng, 4, PROD_UNEVEN_P[k % 2], 9) for k in range(sb0.output_channels)])
    sb1 = N.Rectangular2dSwitchboard((16, 4), (6, 4), (2, 4), 9)
    l1 = N.Layer([_prod_node(rng, sb1.out_channel_dim, 13, 14, head=11) for _ in range(sb1.output_channels)])
    assert (sb0.output_channels, sb1.output_channels) == (64, 6)
    return [sb0, l0, sb1, l1]


# --------------------------------------------------------------------------------------------------------------------- iGSFA stages
IG_FUNCS = [N.identity, N.unsigned_08expo]      # the form k_igfold has a compile-time expansion for
IG_FUNCS_SIGNED = [N.identity, N.signed_expo(0.9)]


def _ig_node(rng, rng_v, d_in, k, q, funcs, with_lr=True, lr_input="scaled", scaling="per_column"):
    """helpers.fuzz_igsfa_net's node, with the widths given."""
    ex = N.GeneralExpansionNode(funcs, d_in)
    sfa = helpers.rand_sfa(rng, ex.output_dim, k, N.GSFANode)
    lr = N.LinearRegressionNode(rng.normal(size=(k + 1, d_in)) / np.sqrt(k + 1))
    pca = helpers.rand_pca(rng, d_in, q)
    pca.avg = np.zeros_like(pca.avg)                   # the residual is centred by construction
    magn = rng.uniform(0.5, 2.0, size=k)
    mat = None
    if scaling == "matrix":        # like the R of a QR decomposition: triangular, well conditioned
        mat = np.triu(rng_v.normal(size=(k, k)) * 0.3, 1) + np.diag(rng_v.uniform(0.5, 2.0, size=k))
    return N.iGSFANode(rng.normal(size=d_in), ex, sfa, None if mat is not None else magn, lr, pca, k,
                       reconstruct_with_sfa=with_lr, lr_input=lr_input, scaling=scaling, scaling_matrix=mat)


def _ig_layer(rng, rng_v, n, d_in, k, q, funcs, **kw):
    return N.Layer([_ig_node(rng, rng_v, d_in, k, q, funcs, **kw) for _ in range(n)])


# Unfolded nets (planned under HIGSFA_IG_NOFOLD=1: the three-GEMM k_igsfa<MS, MO, T, KBM>).  Per net: the field side of layer 0
# (64 nodes on an 8 x 8 grid of fields), (k, q) of layer 0, the merge of layer 1 and its (k, q), the node variant; then what the
# planner must make of it per layer: (nodes, MS, MO, kb1).  MS = ceil(k / 16) slow tiles, MO = ceil((k + q) / 16) output tiles, kb1 =
# input blocks (layer 0: ceil(field^2 / 16) after the gather; layer 1: children x their MO); KBM = kb1 rounded up to 2, 4, 6 or 8.
IG_UNFOLDED = {
    "a": dict(field=4, kq0=(5, 6), merge=(2, 2), kq1=(20, 10), funcs=IG_FUNCS, kw=dict(),
              want=[(64, 1, 1, 1), (16, 2, 2, 4)]),
    "b": dict(field=6, kq0=(10, 17), merge=(2, 1), kq1=(20, 25), funcs=IG_FUNCS, kw=dict(with_lr=False),
              want=[(64, 1, 2, 3), (32, 2, 3, 4)]),
    "c": dict(field=9, kq0=(12, 30), merge=(1, 2), kq1=(20, 40), funcs=IG_FUNCS_SIGNED, kw=dict(scaling="matrix"),      # 64 nodes of 6 blocks: 12 x 2
              want=[(64, 1, 3, 6), (32, 2, 4, 6)]),
    "d": dict(field=10, kq0=(14, 45), merge=(2, 1), kq1=(40, 8), funcs=IG_FUNCS, kw=dict(lr_input="unscaled"),
              want=[(64, 1, 4, 7), (32, 3, 3, 8)]),
    "e": dict(field=8, kq0=(40, 20), merge=(1, 2), kq1=(50, 12), funcs=[N.identity], kw=dict(with_lr=False, scaling="matrix"),
              want=[(64, 3, 4, 4), (32, 4, 4, 8)]),
}
IG_PAIRS = ((1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4))      # pick_igsfa's instantiations
NOFOLD = {"HIGSFA_IG_NOFOLD": "1"}


def ig_unfolded_net(name, seed=0):
    c = IG_UNFOLDED[name]
    rng, rng_v = np.random.default_rng(6200 + ord(name) + 100 * seed), np.random.default_rng(6300 + ord(name) + 100 * seed)
    f = c["field"]
    sb0 = N.Rectangular2dSwitchboard((8 * f, 8 * f), (f, f), (f, f), 1)
    (k0, q0), (k1, q1) = c["kq0"], c["kq1"]
    l0 = _ig_layer(rng, rng_v, 64, f * f, k0, q0, c["funcs"], **c["kw"])
    sb1 = N.Rectangular2dSwitchboard((8, 8), c["merge"], c["merge"], k0 + q0)
    l1 = _ig_layer(rng, rng_v, sb1.output_channels, sb1.out_channel_dim, k1, q1, c["funcs"], **c["kw"])
    return [sb0, l0, sb1, l1]


def ig_shape(n_tiles, n_nodes, kb1, folded):
    """launch_igsfa's (waves that take tiles, tiles per wave) and whether it is the fallback, restated: 12x2 (unfolded, kb1 5 or 6),
    8x2, 4x2 where ceil(tiles / (nw * T)) * nodes >= 256, else 4x2 / 2x2 / 1x2 / 1x1 by the tile count alone."""
    for a, b in ((12, 2), (8, 2), (4, 2)):
        if a == 12 and (folded or kb1 not in (5, 6)):
            continue
        if a * b <= max(n_tiles, 1) and -(-n_tiles // (a * b)) * n_nodes >= 256:
            return a, b, False
    return (4 if n_tiles >= 8 else 2 if n_tiles >= 4 else 1), (2 if n_tiles >= 2 else 1), True


# Folded nets (a node of 65 .. 128 inputs whose expansion holds the identity: one GEMM, k_igfold<MO, T>, or k_igfold_split for a
# layer of at most 8 nodes).  Layer 0: 256 nodes with 9 x 9 fields at stride 1 on a 24 x 24 input (6 blocks each), its k + q spanning
# MO = 1 .. 4 over the variants; the merges above keep every node at 65 .. 128 inputs down to a top of 8 or 4 nodes.
# Per variant: (k, q) of layer 0, then (merge, (k, q)) per layer above, the expansion; want: (nodes, MO, kb1) per layer.
IG_FOLDED = {
    1: dict(kq0=(6, 10), up=[((2, 4), (8, 12)), ((2, 2), (10, 3))], funcs=IG_FUNCS, kw=dict(),
            want=[(256, 1, 6), (32, 2, 8), (8, 1, 8)]),
    2: dict(kq0=(9, 11), up=[((2, 2), (8, 12)), ((2, 2), (8, 12)), ((2, 2), (20, 10))], funcs=IG_FUNCS_SIGNED, kw=dict(scaling="matrix"),
            want=[(256, 2, 6), (64, 2, 8), (16, 2, 8), (4, 2, 8)]),
    3: dict(kq0=(14, 26), up=[((2, 1), (8, 12)), ((2, 2), (8, 12)), ((2, 2), (30, 10))], funcs=IG_FUNCS, kw=dict(with_lr=False),
            want=[(256, 3, 6), (128, 2, 6), (32, 2, 8), (8, 3, 8)]),
    4: dict(kq0=(20, 40), up=[((1, 2), (8, 12)), ((2, 2), (8, 12)), ((2, 2), (40, 24))], funcs=IG_FUNCS_SIGNED, kw=dict(lr_input="unscaled"),
            want=[(256, 4, 6), (128, 2, 8), (32, 2, 8), (8, 4, 8)]),
}


def ig_folded_net(mo, seed=0):
    c = IG_FOLDED[mo]
    rng, rng_v = np.random.default_rng(6400 + mo + 100 * seed), np.random.default_rng(6500 + mo + 100 * seed)
    sb = N.Rectangular2dSwitchboard((24, 24), (9, 9), (1, 1), 1)
    k, q = c["kq0"]
    flow = [sb, _ig_layer(rng, rng_v, 256, 81, k, q, c["funcs"], **c["kw"])]
    w, h, ch = 16, 16, k + q
    for merge, (k, q) in c["up"]:
        sb = N.Rectangular2dSwitchboard((w, h), merge, merge, ch)
        assert 64 < sb.out_channel_dim <= 128, sb.out_channel_dim
        flow += [sb, _ig_layer(rng, rng_v, sb.output_channels, sb.out_channel_dim, k, q, c["funcs"], **c["kw"])]
        (w, h), ch = sb.out_channels_xy, k + q
    return flow


SPLIT_LINE_ROWS = (32768, 32784)      # 2048 and 2049 tiles: 8 nodes x tiles <= 16384 runs k_igfold_split, above it k_igfold


def ig_split_line_net(seed=0):
    """A folded first layer of 8 nodes on 128 input columns (72-column fields at stride 8, 5 blocks each, 24 outputs)."""
    rng, rng_v = np.random.default_rng(6600 + seed), np.random.default_rng(6700 + seed)
    sb = N.Rectangular2dSwitchboard((128, 1), (72, 1), (8, 1), 1)
    assert sb.output_channels == 8
    return [sb, _ig_layer(rng, rng_v, 8, 72, 10, 14, IG_FUNCS)]


# ------------------------------------------------------------------------------------------------------------------------- mixed
def _plain_layer(rng, n, d_in, p, s):
    out = []
    for _ in range(n):
        ex = N.GeneralExpansionNode(IG_FUNCS, p)
        out.append(N.FlowNode([helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, helpers.rand_sfa(rng, ex.output_dim, s)]))
    return N.Layer(out)


MIXED_KINDS = [0, 3, 2, 0]      # HostStage::kind per stage: ordinary (front kernel), product, iGSFA, ordinary


def mixed_net(seed=0):
    """Ordinary layer 0 on the caller's rows (no gather stage) -> product layer -> folded iGSFA layer -> ordinary top: 64, 16, 4
    and 1 nodes on a 16 x 16 input.  The product layer reads an ordinary layer's tiles, the iGSFA layer (72 inputs: 4 children of two
    tiles, 8 blocks) a product layer's, the top an iGSFA layer's."""
    rng, rng_v = np.random.default_rng(6800 + seed), np.random.default_rng(6900 + seed)
    sb0 = N.Rectangular2dSwitchboard((16, 16), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((8, 8), (2, 2), (2, 2), 8)
    sb2 = N.Rectangular2dSwitchboard((4, 4), (2, 2), (2, 2), 18)
    sb3 = N.Rectangular2dSwitchboard((2, 2), (2, 2), (2, 2), 24)
    l1 = N.Layer([_prod_node(rng, 32, 14, 18) for _ in range(16)])
    return [sb0, _plain_layer(rng, 64, 4, 4, 8), sb1, l1, sb2, _ig_layer(rng, rng_v, 4, 72, 10, 14, IG_FUNCS), sb3, _plain_layer(rng, 1, 96, 20, 17)]


# ------------------------------------------------------------------------------------------------- what a call must launch, by design
def stage_table(name):
    """Per product / iGSFA stage of the net's full plan, from the data above (pinned by the host test): dicts with the stage index,
    kind, node count and what decides the shape."""
    if name.startswith("prod") and name != "prod_uneven":
        mt1, mt2 = int(name[4]), int(name[5])
        return [dict(kind="prod", stage=1, nodes=64, mt1=mt1, mt2=mt2)]
    if name == "prod_uneven":
        return [dict(kind="prod", stage=1, nodes=64, mt1=2, mt2=1), dict(kind="prod", stage=2, nodes=6, mt1=1, mt2=1)]
    if name.startswith("ig_"):
        return [dict(kind="igsfa", stage=i + 1, nodes=n, ms=ms, mo=mo, kb1=kb, folded=False) for i, (n, ms, mo, kb) in enumerate(IG_UNFOLDED[name[3:]]["want"])]
    if name.startswith("igfold"):
        return [dict(kind="igsfa", stage=i + 1, nodes=n, ms=mo, mo=mo, kb1=kb, folded=True) for i, (n, mo, kb) in enumerate(IG_FOLDED[int(name[6:])]["want"])]
    assert name == "mixed"
    return [dict(kind="prod", stage=1, nodes=16, mt1=1, mt2=2), dict(kind="igsfa", stage=2, nodes=4, ms=2, mo=2, kb1=8, folded=True)]


def expected_launches(name, rows):
    """What the product and iGSFA debug lines of one full call must say: (kind, stage, nodes, shape) per launch, and whether an iGSFA
    shape is the fallback.  A folded layer of at most 8 nodes runs k_igfold_split up to 16384 (node, tile) pairs: no such line.  From
    prod_shape / ig_shape, the restated rules: the host test holds the library's own rule to it, the GPU test its launches."""
    t = tiles(rows)
    out = []
    for s in stage_table(name):
        if s["kind"] == "prod":
            out.append(dict(kind="prod", stage=s["stage"], nodes=s["nodes"], shape=prod_shape(t, s["nodes"]), widths=(s["mt1"], s["mt2"])))
        elif not (s["folded"] and s["nodes"] <= 8 and s["nodes"] * t <= 16384):
            nw, tt, fallback = ig_shape(t, s["nodes"], s["kb1"], s["folded"])
            out.append(dict(kind="igsfa", stage=s["stage"], nodes=s["nodes"], shape=(nw, tt), fallback=fallback, widths=(s["ms"], s["mo"]),
                            kb1=s["kb1"], folded=s["folded"]))
    return out


PROD_LINE = r"\[prod stage (\d+)\] nodes (\d+) mt1 (\d+) mt2 (\d+) neb (\d+) shape (\d+)x(\d+) npg (\d+) node_groups (\d+) tile_groups (\d+) parts (\d+)"
IG_LINE = r"\[igsfa stage (\d+)\] nodes (\d+) kb1 (\d+) shape (\d+)x(\d+) occ (\d+) lds (\d+) tile_groups (\d+) parts (\d+)"
# one HIGSFA_DEBUG line per launch of a call; the stages it covers: "[front]" layers 0 and 1, "[front0]" layer 0, "... stage i]" stage i
# and, where the line says "layers k", the k - 1 above it
STEP_LINE = r"\[(front0?|(gather|sweep|splitm|igsplit|igsfa|prod|pair|subtree|top) stage (\d+))\]( layers (\d+))?"


def covered_stages(text):
    """The stages the debug lines of ONE call name, launch by launch, in the order they were written."""
    import re
    out = []
    for ln in text.splitlines():
        m = re.match(STEP_LINE, ln)
        if not m:
            continue
        first = int(m.group(3)) if m.group(3) is not None else 0
        n = 2 if m.group(1) == "front" else int(m.group(5)) if m.group(5) else 1
        out += list(range(first, first + n))
    return out


# ------------------------------------------------------------------------------------------------------------------------- the list
def nets():
    """{name: (constructor, switches the handle is planned under)} of every net of the per-node, batch-independence and shape tests."""
    out = {}
    for a, b in PROD_PAIRS:
        out["prod%d%d" % (a, b)] = ((lambda a=a, b=b: prod_layer_net(a, b)), {})
    out["prod_uneven"] = (prod_uneven_net, {})
    for name in IG_UNFOLDED:
        out["ig_" + name] = ((lambda name=name: ig_unfolded_net(name)), NOFOLD)
    for mo in IG_FOLDED:
        out["igfold%d" % mo] = ((lambda mo=mo: ig_folded_net(mo)), {})
    out["mixed"] = (mixed_net, {})
    return out
