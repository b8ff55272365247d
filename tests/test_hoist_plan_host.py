"""CPU: the planner's hoist pass (hoist_first_affines, csrc/hg_fused_plan.cpp) through a stand-alone driver with its own main
(tests/hoist_plan_driver.cpp, linked against the blob parser and the planner alone).  With FusedOptions::hoist off the planner is
what tests/test_fused_plan_host.py pins; here it is on: which links are taken, what stays as recorded, and the float64 fold itself
against numpy's on seeded draws (tests/plan_cases.reseed: no linear-algebra result of this machine reaches the comparison as an
input)."""
import re
import shutil
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import blob
from pyfaceanalysis_amd import nodes as N
from tests import helpers, hoist_cases, plan_cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hoist") / "hoist_plan_driver"
    b = hoist_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def plans(driver, tmp_path, named_blobs):
    """{name: (hoisted stage indices, plan lines)} of one driver run."""
    files = []
    for k, (_, b) in enumerate(named_blobs):
        p = tmp_path / ("f%d.bin" % k)
        p.write_bytes(b)
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    parts = text.split("== ")[1:]
    assert len(parts) == len(named_blobs)
    out = {}
    for (name, _), part in zip(named_blobs, parts):
        lines = part.splitlines()[1:]
        assert lines[0].startswith("hoisted:"), lines[0]
        out[name] = ([int(v) for v in lines[0].split()[1:]], lines[1:])
    return out


def stage_fields(lines):
    """{stage index: {field: text}} of one net's plan lines."""
    fields = lines[0].split(": ")[1].split()
    return {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in lines) if m}


def links(driver, tmp_path, blobs):
    """Per blob {hoisted stage: [(columns of z, children in the order their tiles are added) per node]} of one driver --links run."""
    files = []
    for k, b in enumerate(blobs):
        p = tmp_path / ("l%d.bin" % k)
        p.write_bytes(b)
        files.append(str(p))
    r = subprocess.run([str(driver), "--links"] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    parts = text.split("== ")[1:]
    assert len(parts) == len(blobs)
    out = []
    for part in parts:
        st = {}
        for ln in part.splitlines()[1:]:
            w = ln.split()
            assert w[0] == "parent" and w[3] == "cols" and w[5] == "kids", ln
            st.setdefault(int(w[1]), []).append((int(w[4]), [int(v) for v in w[6:]]))
            assert len(st[int(w[1])]) == int(w[2]) + 1
        out.append(st)
    return out


def recorded_blob(name):
    return next(b for n, env, b in plan_cases.cases() if n == name and not env)


def test_presets_hoist_the_links_the_rule_selects(driver, tmp_path):
    """U11L-128: sum_in on exactly stages 4-10 (the 60 -> 60 links); stages 0-3 keep every recorded line except the digests of
    stage 3's weights and biases, which now hold the folded second affine.  U11L-64: its 60 -> 60 links, one layer later.  T3L-8,
    T5L-16 and the lower links of both U11L nets have P > S: left alone."""
    names = ("U11L-128", "U11L-64", "T5L-16", "T3L-8")
    got = plans(driver, tmp_path, [(n, recorded_blob(n)) for n in names])
    golden = plan_cases.load_golden()
    assert got["U11L-128"][0] == [4, 5, 6, 7, 8, 9, 10]
    assert got["U11L-64"][0] == [5, 6, 7, 8, 9, 10]
    assert got["T5L-16"][0] == [] and got["T3L-8"][0] == []
    for name in ("T5L-16", "T3L-8"):      # nothing hoisted: the recorded plan, line by line
        assert got[name][1] == golden[name]
    lines, want = got["U11L-128"][1], golden["U11L-128"]
    for k in range(1 + 3 * 4):      # the field list and three lines per stage 0..3
        if lines[k].startswith("stage 3 arrays:"):
            a, e = lines[k].split(), want[k].split()
            assert len(a) == len(e)
            differ = [x.split("=")[0] for x, y in zip(a, e) if x != y]
            assert differ == ["afrag", "bias"], differ
            assert [x.split(":")[0] for x in a] == [y.split(":")[0] for y in e]      # same lengths
        else:
            assert lines[k] == want[k], k
    fields = lines[0].split(": ")[1].split()
    stage = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in lines) if m}
    rec = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in want) if m}
    for si in range(4, 11):
        s, r = stage[si], rec[si]
        assert int(s["ks1_tile"]) == 0 and s["ks2_tile"] == r["ks2_tile"]
        assert int(s["node_blocks"]) == int(r["node_blocks"]) - int(r["kb1"]) * int(r["mt1"]) == 32
        assert int(s["kb1"]) == 2 * int(s["mt1"])
        assert int(s["mfma16_tile"]) * 2 == int(r["mfma16_tile"])      # half the issued MFMAs: 60 x 120 of 60 x 240 per node
    name4 = next(ln for ln in lines if ln.startswith("stage 4 name:"))
    assert "first affine folded" in name4 and "plain 16-row tiles only" in name4


def test_links_that_must_stay(driver, tmp_path):
    """Overlapping fields (a child column read twice, children shared between parents), product expansions, iGSFA nodes on either
    side of a link, linear-only layers: nothing is hoisted, and the plan is the one the planner makes with the pass off."""
    cases = [("overlapping_net", recorded_blob("overlapping_net")), ("product_hier_net", recorded_blob("product_hier_net")),
             ("fuzz_igsfa_net_1", recorded_blob("fuzz_igsfa_net_1")), ("linear_u11l_96", recorded_blob("linear_u11l_96")),
             ("igsfa_parent", blob.flow_to_blob(plan_cases.reseed(hoist_cases.igsfa_after_ordinary(), 31)))]
    got = plans(driver, tmp_path, cases)
    golden = plan_cases.load_golden()
    for name, _ in cases:
        assert got[name][0] == [], name
        if name in golden:
            assert got[name][1] == golden[name], name


def test_test_nets_hoist_where_the_gpu_tests_expect(driver, tmp_path):
    """The nets of tests/test_hoist_gpu.py: chained links with parents of 2, 3 and 4 tiles, four children per parent, and a
    sub-tree fuzz net with an eligible link."""
    cases = [("chain", blob.flow_to_blob(hoist_cases.chain_net())), ("quad", blob.flow_to_blob(hoist_cases.quad_net())),
             ("small", blob.flow_to_blob(hoist_cases.small_net()))]
    cases += [("fuzz%d" % s, blob.flow_to_blob(helpers.subtree_fuzz_net(s))) for s in range(8)]
    got = plans(driver, tmp_path, cases)
    # the node-group sizes tests/test_hoist_gpu.py::test_ragged_node_groups counts on: KiB of fragments per node of a hoisted stage
    st = stage_fields(got["chain"][1])
    assert [(int(st[i]["n_nodes"]), int(st[i]["node_blocks"])) for i in (2, 3, 4, 5, 6)] == hoist_cases.CHAIN_SUM_STAGES
    st = stage_fields(got["quad"][1])
    assert [(int(st[i]["n_nodes"]), int(st[i]["node_blocks"])) for i in (2, 3, 4)] == hoist_cases.QUAD_SUM_STAGES
    assert got["chain"][0] == [2, 3, 4, 5, 6]
    assert got["quad"][0] == [2, 3, 4]
    assert got["small"][0] == [2]
    fields = got["chain"][1][0].split(": ")[1].split()
    st = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in got["chain"][1]) if m}
    assert [int(st[i]["mt1"]) for i in (2, 3, 4, 5, 6)] == [2, 3, 4, 4, 4]
    st = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in got["quad"][1]) if m}
    assert [int(st[i]["kb1"]) // int(st[i]["mt1"]) for i in (2, 3, 4)] == [4, 4, 2]
    assert got["fuzz%d" % hoist_cases.FUZZ_SEED][0], "the fuzz net of the GPU test has no hoisted link"


def test_ragged_nets_hoist_as_described(driver, tmp_path):
    """hoist_cases.ragged_net: four parents of 1, 3, 4 and 8 children and of one z-tile (k_stage_sum<1, ...>, a K-block table padded
    to eight entries), children recorded in first-read order, which is not ascending; with 18 or 20 columns in the layer above, whose
    last tile then holds 2 or 4 rows, exactly that link is refused between two that are taken.  ragged_wide_net: parents of 1, 2, 3
    and 3 tiles on a three-tile layer."""
    nets = [("ragged", hoist_cases.ragged_net()), ("ragged18", hoist_cases.ragged_net(p3=18)), ("ragged20", hoist_cases.ragged_net(p3=20)),
            ("wide", hoist_cases.ragged_wide_net())]
    blobs = [(n, blob.flow_to_blob(f)) for n, f in nets]
    got = plans(driver, tmp_path, blobs)
    assert got["ragged"][0] == [2, 3, 4]
    assert got["ragged18"][0] == [2, 4] and got["ragged20"][0] == [2, 4]
    assert got["wide"][0] == [2, 3, 4]
    st = stage_fields(got["ragged"][1])
    assert [(int(st[i]["mt1"]), int(st[i]["kb1"]), int(st[i]["n_nodes"])) for i in (2, 3, 4)] == [(1, 8, 4), (2, 4, 2), (1, 2, 1)]
    assert [(int(st[i]["n_nodes"]), int(st[i]["node_blocks"])) for i in (2, 3, 4)] == hoist_cases.RAGGED_SUM_STAGES
    for name in ("ragged18", "ragged20"):      # the refused stage multiplies: K-blocks of the two-tile children, times its own two tiles
        st = stage_fields(got[name][1])
        assert [(int(st[i]["mt1"]), int(st[i]["kb1"])) for i in (2, 3, 4)] == [(1, 8), (2, 4), (1, 2)]
        name3 = next(ln for ln in got[name][1] if ln.startswith("stage 3 name:"))
        assert "first affine folded" not in name3
    st = stage_fields(got["wide"][1])
    assert [(int(st[i]["mt1"]), int(st[i]["kb1"]), int(st[i]["n_nodes"])) for i in (2, 3, 4)] == [(3, 24, 4), (3, 6, 2), (2, 4, 1)]
    assert int(st[1]["mto"]) == 3      # the children store three tiles each, whatever their own parent fills
    ln = links(driver, tmp_path, [b for _, b in blobs])
    groups = hoist_cases.RAGGED_GROUPS
    assert any(g != sorted(g) for g in groups)
    for k in range(4):
        assert [kids for _, kids in ln[k][2]] == groups
    assert [p for p, _ in ln[0][2]] == [6, 12, 14, 10] and [p for p, _ in ln[0][3]] == [21, 21]
    assert sorted(ln[1]) == [2, 4] and sorted(ln[2]) == [2, 4]
    assert [(p + 15) // 16 for p, _ in ln[3][2]] == [1, 2, 3, 3]


def test_order_probe_premises(driver, tmp_path):
    """hoist_cases.order_probe_net: the one parent is hoisted, its children are recorded as 1, 2, 0 (first read), and the float64 bias
    vector of the fold is exactly zero — what tests/test_hoist_gpu.py::test_children_are_added_in_first_read_order rests on."""
    flow = hoist_cases.order_probe_net()
    b = blob.flow_to_blob(flow)
    assert plans(driver, tmp_path, [("probe", b)])["probe"][0] == [2]
    assert links(driver, tmp_path, [b]) == [{2: [(5, [1, 2, 0])]}]
    p = tmp_path / "probe.bin"
    p.write_bytes(b)
    r = subprocess.run([str(driver), "--dump", str(p)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    bias = [float(v) for v in lines[0].split("bias")[1].split()]
    assert lines[0].startswith("parent 2 0 kids 1 2 0 bias") and bias == [0.0] * 5
    w = {int(ln.split()[2]): np.array([float(v) for v in ln.split(" W ")[1].split()]) for ln in lines if ln.startswith("child")}
    assert np.array_equal(w[2], -w[1]) and np.abs(w[1]).max() > 1e3 * np.abs(w[0]).max()
    assert np.array_equal(w[1].astype(np.float32).astype(np.float64) * -1, w[2].astype(np.float32))
    x = hoist_cases.order_probe_rows(8)
    assert np.array_equal(x[:, 8:12], x[:, 4:8])


def test_fuzz_seeds_cover_the_irregular_links(driver, tmp_path):
    """Conditions on the inputs of tests/test_hoist_gpu.py, not measurements: across hoist_cases.HOIST_FUZZ_SEEDS the hoisted stages
    have 1, 2, 3 and 4 z-tiles; parents of 1, 2, 3, at least 5, and 8 children; at least three stages whose nodes differ in child
    count and two whose nodes differ in tile count; at least three nets have a refused link above a taken one, and at least nine
    have a taken link at all.  If the generator drifts, change its constants, not these."""
    seeds = hoist_cases.HOIST_FUZZ_SEEDS
    assert len(seeds) == 12
    blobs = [("fz%d" % s, blob.flow_to_blob(hoist_cases.hoist_fuzz_net(s))) for s in seeds]
    got = plans(driver, tmp_path, blobs)      # (asserts that every net has a fused plan)
    ln = links(driver, tmp_path, [b for _, b in blobs])
    mt1, n_kids, differ_kids, differ_tiles, refused_above, taken = set(), set(), 0, 0, 0, 0
    for (name, _), per_stage in zip(blobs, ln):
        hoisted, lines = got[name]
        st = stage_fields(lines)
        assert sorted(per_stage) == hoisted
        assert all(int(st[i]["kind"]) == 0 for i in st) and len(st) <= 5
        taken += bool(hoisted)
        refused_above += bool(hoisted) and any(i not in hoisted for i in range(min(hoisted), len(st)))
        for i in hoisted:
            mt1.add(int(st[i]["mt1"]))
            counts = {len(kids) for _, kids in per_stage[i]}
            assert max(counts) * int(st[i]["mt1"]) == int(st[i]["kb1"])
            n_kids |= counts
            differ_kids += len(counts) > 1
            differ_tiles += len({(p + 15) // 16 for p, _ in per_stage[i]}) > 1
    assert mt1 == {1, 2, 3, 4}
    assert {1, 2, 3, 8} <= n_kids and any(k >= 5 for k in n_kids)
    assert differ_kids >= 3 and differ_tiles >= 2
    assert refused_above >= 3 and taken >= 9
    assert tuple(s for s in seeds if got["fz%d" % s][0]) == hoist_cases.HOIST_FUZZ_TAKEN


def _affine_parts(node):
    """(W, c) of y = e @ W + c for a trained PCA / SFA node."""
    if isinstance(node, N.SFANode):
        return node.sf, -node._bias[0]
    return node.v, -(node.avg[0] @ node.v)


@pytest.mark.parametrize("make", [hoist_cases.small_net, lambda: hoist_cases.chain_net(dims=[(5, 6), (7, 9), (8, 12), (10, 12), (9, 7)], side=16),
                                  hoist_cases.ragged_net, hoist_cases.ragged_wide_net])
def test_fold_matches_numpy_float64(driver, tmp_path, make):
    """The driver's --dump of the normal form after the pass: per child the folded second affine A2_c A1_p[rows of c, :] (its own
    constants gone), per parent ONE bias vector sum_c (b2_c - a_p[rows c]) A1_p[rows c, :]; numpy's float64 fold of the same seeded
    draws agrees within 1e-12 of the largest entry."""
    flow = plan_cases.reseed(make(), 77)
    p = tmp_path / "net.bin"
    p.write_bytes(blob.flow_to_blob(flow))
    r = subprocess.run([str(driver), "--dump", str(p)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    parents, children = {}, {}
    for ln in text.splitlines():
        w = ln.split()
        if w[0] == "parent":
            kb = w.index("bias")
            parents[(int(w[1]), int(w[2]))] = ([int(v) for v in w[4:kb]], np.array([float(v) for v in w[kb + 1:]]))
        elif w[0] == "child":
            rows, cols = int(w[4]), int(w[5])
            assert float(w[7]) == 0.0
            children[(int(w[1]), int(w[2]))] = np.array([float(v) for v in w[9:]]).reshape(rows, cols)
    assert parents and children
    layers = [n for n in flow if isinstance(n, N.Layer)]
    boards = [n for n in flow if isinstance(n, N.Switchboard)]
    checked = 0
    for (pi, pj), (kids, bias) in parents.items():
        conn = np.asarray(boards[pi].connections)
        child_nodes = layers[pi - 1].nodes
        widths = [c.output_dim for c in child_nodes]
        col0 = np.concatenate([[0], np.cumsum(widths)])
        pnode = layers[pi].nodes[pj]
        in_off = sum(n.input_dim for n in layers[pi].nodes[:pj])
        mine = conn[in_off:in_off + pnode.input_dim]
        pca = pnode.flow[0]
        owner = np.searchsorted(col0, mine, side="right") - 1
        order = []
        for o in owner:
            if o not in order:
                order.append(int(o))
        assert order == kids
        want_bias = np.zeros(pca.output_dim)
        for ci in kids:
            rows = np.nonzero(owner == ci)[0]
            local = mine[rows] - col0[ci]
            w2, c2 = _affine_parts(child_nodes[ci].flow[-1])
            want = w2[:, local] @ pca.v[rows, :]
            got = children[(pi - 1, ci)]
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
            want_bias += (c2[local] - pca.avg[0, rows]) @ pca.v[rows, :]
            checked += 1
        assert np.abs(bias - want_bias).max() <= 1e-12 * np.abs(want_bias).max()
    assert checked == len(children)
