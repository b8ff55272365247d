"""CPU: the premises of tests/test_stage_shapes_gpu.py, through the planner's stand-alone driver (tests/hoist_plan_driver.cpp: the blob
parser and the planner alone, the plan the library makes).  Per net of tests/stage_shape_cases.py every stage's kind, tile widths,
K-blocks, product-column blocks, fold and node count; over their union every instantiation of k_stage_prod, k_igsfa and k_igfold; and
the launch shapes the batch sizes were chosen for, from the rule of sweep_shape / launch_igsfa as restated in the cases file.
Conditions on the tests' inputs, not measurements: if a generator drifts, change the net, not these.  (The nets are not added to
tests/golden/fused_plan_digests.json, which records the pre-split planner.)"""
import os
import re
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import blob
from tests import hoist_cases
from tests import stage_shape_cases as cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stage_shapes") / "plan_driver"
    b = hoist_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def stages(driver, tmp_path, named_flows, env=None):
    """{name: [{field: text} per stage]} of one driver run; a net the planner refuses (no FUSED plan) fails here."""
    files = []
    for k, (_, flow) in enumerate(named_flows):
        p = tmp_path / ("s%d.bin" % k)
        p.write_bytes(blob.flow_to_blob(flow))
        files.append(str(p))
    e = {k: v for k, v in os.environ.items() if not k.startswith("HIGSFA_")}
    e.update(env or {})
    r = subprocess.run([str(driver)] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=e)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    parts = text.split("== ")[1:]
    assert len(parts) == len(named_flows)
    out = {}
    for (name, _), part in zip(named_flows, parts):
        lines = part.splitlines()[1:]
        assert lines[0].startswith("hoisted:"), (name, lines[0])      # else "refused: ...": not FUSED
        fields = lines[1].split(": ")[1].split()
        st = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in lines) if m}
        out[name] = [st[i] for i in range(len(st))]
    return out


def ints(stage, *names):
    return tuple(int(stage[n]) for n in names)


def test_product_layers_cover_every_tile_width(driver, tmp_path):
    """prod_layer_net(mt1, mt2): a gather and ONE product stage of 64 nodes with exactly those tile widths, one K-block, and the
    product-column blocks of its width (2 .. 6, the last pair product reading feature p - 1 <= 60); all 16 pairs."""
    got = stages(driver, tmp_path, [("%d%d" % pr, cases.prod_layer_net(*pr)) for pr in cases.PROD_PAIRS])
    seen = set()
    for mt1, mt2 in cases.PROD_PAIRS:
        st = got["%d%d" % (mt1, mt2)]
        assert [int(s["kind"]) for s in st] == [1, 3]
        p, s = cases.prod_dims(mt1, mt2)
        assert ints(st[1], "mt1", "mt2", "kb1", "neb", "n_nodes", "p_max", "s_max", "has_clip", "ig_folded", "nf") == \
            (mt1, mt2, 1, cases.prod_neb(p), 64, p, s, 1, 0, 2)
        seen.add(ints(st[1], "mt1", "mt2"))
    assert seen == set(cases.PROD_PAIRS) and len(seen) == 16
    assert {cases.prod_neb(cases.prod_dims(m, 1)[0]) for m in (1, 2, 3, 4)} == {3, 4, 5, 6}


def test_product_shapes_of_the_batch_sizes():
    """The rule of sweep_shape on a 64-node layer at cases.ROWS: the shrunk default (1 x 1, 2 x 1), the default, 4 x 1 chosen, 4 x 2 and
    8 x 2 — the last two on odd tile counts, so a wave's second tile is absent in the last tile group."""
    assert [cases.tiles(n) for n in cases.ROWS] == [1, 2, 5, 13, 27, 51, 109]
    assert {n: cases.prod_shape(cases.tiles(n), 64) for n in cases.ROWS} == cases.PROD_SHAPES_64
    assert cases.tiles(425) % 2 == 1 and cases.tiles(805) % 2 == 1 and cases.tiles(1738) % 2 == 1
    # prod_uneven's top layer of 6 nodes never leaves the default
    assert {cases.prod_shape(cases.tiles(n), 6) for n in cases.ROWS} == {(1, 1), (2, 1), (4, 1)}


def test_uneven_product_net(driver, tmp_path):
    """prod_uneven_net: both layers table-driven; layer 0 is as wide as its widest node (two z-tiles, 3 blocks of product columns
    for 21 + 19), 9 KiB of fragments per node: with 52 KiB less the z images of 8 x 2, 4 x 2 and 4 x 1 waves launch_prod groups
    2, 3 and 4 nodes, and 3 does not divide 64.  Layer 1: 24 K-blocks (overlapping fields), a HeadNode folded into 11 outputs."""
    st = stages(driver, tmp_path, [("u", cases.prod_uneven_net())])["u"]
    assert [int(s["kind"]) for s in st] == [1, 3, 3]
    assert ints(st[1], "mt1", "mt2", "kb1", "neb", "n_nodes", "p_max", "s_max", "node_blocks") == (2, 1, 1, 3, 64, 20, 9, 9)
    assert ints(st[2], "mt1", "mt2", "kb1", "neb", "n_nodes", "p_max", "s_max") == (1, 1, 24, 3, 6, 13, 11)
    per_node = 9 * 1024 + int(st[1]["bias_floats"]) * 4 + 8
    npg = {nw * t: (52 * 1024 - nw * t * 2 * 1024 - 3 * 128) // per_node for nw, t in ((8, 2), (4, 2), (4, 1))}
    assert npg == {16: 2, 8: 3, 4: 4} and 64 % 3


def test_unfolded_igsfa_nets_cover_every_instantiation(driver, tmp_path):
    """ig_unfolded_net under HIGSFA_IG_NOFOLD=1: a gather and two unfolded iGSFA stages with the (nodes, MS, MO, kb1) the cases file
    states; over the five nets all ten (MS, MO) of pick_igsfa and all four K-block capacities; net "c" has the 64-node layer of
    6 blocks that takes 12 x 2.  Without the switch the same nets fold (so the switch is what keeps them on k_igsfa)."""
    flows = [(n, cases.ig_unfolded_net(n)) for n in cases.IG_UNFOLDED]
    got = stages(driver, tmp_path, flows, cases.NOFOLD)
    pairs, caps = set(), set()
    for name, c in cases.IG_UNFOLDED.items():
        st = got[name]
        assert [int(s["kind"]) for s in st] == [1, 2, 2], name
        assert [ints(s, "n_nodes", "mt1", "mt2", "kb1") for s in st[1:]] == c["want"], name
        for s in st[1:]:
            assert ints(s, "ig_folded", "neb") == (0, 0)
            assert int(s["ig_has_lr"]) == int(c["kw"].get("with_lr", True))
            pairs.add(ints(s, "mt1", "mt2"))
            caps.add((int(s["kb1"]) + 1) // 2 * 2)
    assert pairs == set(cases.IG_PAIRS) and len(pairs) == 10
    assert caps == {2, 4, 6, 8}
    assert cases.IG_UNFOLDED["c"]["want"][0] == (64, 1, 3, 6)
    folded = stages(driver, tmp_path, flows)
    assert all(int(s["ig_folded"]) == 1 or int(s["kind"]) != 2 for st in folded.values() for s in st)


def test_igsfa_shapes_of_the_batch_sizes():
    """launch_igsfa's rule at cases.ROWS: the 64-node layer of 6 blocks runs 12 x 2, 8 x 2 and 4 x 2 chosen and the fallbacks 4 x 2,
    2 x 2, 1 x 2 and 1 x 1; a 64-node layer of another block count 8 x 2 twice; a folded layer of 256 nodes 8 x 2 from 425 rows."""
    c6 = {n: cases.ig_shape(cases.tiles(n), 64, 6, False) for n in cases.ROWS}
    assert c6 == {1: (1, 1, True), 17: (1, 2, True), 70: (2, 2, True), 195: (4, 2, True), 425: (4, 2, False), 805: (8, 2, False), 1738: (12, 2, False)}
    c4 = {n: cases.ig_shape(cases.tiles(n), 64, 4, False) for n in cases.ROWS}
    assert c4 == {**c6, 1738: (8, 2, False)}
    f = {n: cases.ig_shape(cases.tiles(n), 256, 6, True) for n in cases.ROWS}
    assert f == {1: (1, 1, True), 17: (1, 2, True), 70: (2, 2, True), 195: (4, 2, False), 425: (8, 2, False), 805: (8, 2, False), 1738: (8, 2, False)}


def test_folded_igsfa_nets(driver, tmp_path):
    """ig_folded_net(mo): every layer a folded iGSFA stage (65 .. 128 inputs per node) with the (nodes, MO, kb1) the cases file states:
    256 nodes with MO = 1 .. 4, and a top of at most 8 nodes and 8 blocks, which is k_igfold_split's at every batch size of the
    tests (nodes x tiles <= 16384).  The two-function expansions: identity and |x|^0.8 (the compile-time form) on variants 1 and 3."""
    got = stages(driver, tmp_path, [(str(mo), cases.ig_folded_net(mo)) for mo in cases.IG_FOLDED])
    for mo, c in cases.IG_FOLDED.items():
        st = got[str(mo)]
        assert [int(s["kind"]) for s in st] == [1] + [2] * len(c["want"]), mo
        assert [ints(s, "n_nodes", "mt2", "kb1") for s in st[1:]] == c["want"], mo
        for s in st[1:]:
            assert ints(s, "ig_folded", "ig_has_lr", "nf") == (1, 0, 2) and s["mt1"] == s["mt2"]
        assert c["want"][0] == (256, mo, 6)
        assert ints(st[-1], "n_nodes")[0] <= 8 and ints(st[-1], "kb1")[0] <= 8
        assert ints(st[-1], "n_nodes")[0] * cases.tiles(cases.N_REF) <= 16384
    assert {c["want"][0][1] for c in cases.IG_FOLDED.values()} == {1, 2, 3, 4}
    assert {c["want"][-1][1] for c in cases.IG_FOLDED.values()} == {1, 2, 3, 4}      # k_igfold_split's output tiles as well


def test_split_line_net(driver, tmp_path):
    """ig_split_line_net: one folded stage of 8 nodes, 5 blocks, two functions — k_igfold_split's conditions; 8 x 2048 tiles is the
    last batch on its side of the line, 8 x 2049 the first on k_igfold's."""
    st = stages(driver, tmp_path, [("s", cases.ig_split_line_net())])["s"]
    assert [int(s["kind"]) for s in st] == [1, 2]
    assert ints(st[1], "n_nodes", "mt2", "kb1", "ig_folded", "nf") == (8, 2, 5, 1, 2)
    assert [8 * cases.tiles(n) for n in cases.SPLIT_LINE_ROWS] == [16384, 16392]


def test_mixed_net(driver, tmp_path):
    """mixed_net plans FUSED with no gather: ordinary (from the caller's rows), product, folded iGSFA, ordinary."""
    st = stages(driver, tmp_path, [("m", cases.mixed_net())])["m"]
    assert [int(s["kind"]) for s in st] == cases.MIXED_KINDS
    assert [int(s["from_x"]) for s in st] == [1, 0, 0, 0]
    assert [int(s["n_nodes"]) for s in st] == [64, 16, 4, 1]
    assert ints(st[1], "mt1", "mt2", "kb1", "neb", "has_clip") == (1, 2, 4, 3, 1)
    assert ints(st[2], "mt1", "mt2", "kb1", "ig_folded") == (2, 2, 8, 1)
