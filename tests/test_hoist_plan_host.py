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
    assert got["chain"][0] == [2, 3, 4, 5, 6]
    assert got["quad"][0] == [2, 3, 4]
    assert got["small"][0] == [2]
    fields = got["chain"][1][0].split(": ")[1].split()
    st = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in got["chain"][1]) if m}
    assert [int(st[i]["mt1"]) for i in (2, 3, 4, 5, 6)] == [2, 3, 4, 4, 4]
    st = {int(m.group(1)): dict(zip(fields, m.group(2).split())) for m in (re.match(r"stage (\d+): (.*)", ln) for ln in got["quad"][1]) if m}
    assert [int(st[i]["kb1"]) // int(st[i]["mt1"]) for i in (2, 3, 4)] == [4, 4, 2]
    assert got["fuzz%d" % hoist_cases.FUZZ_SEED][0], "the fuzz net of the GPU test has no hoisted link"


def _affine_parts(node):
    """(W, c) of y = e @ W + c for a trained PCA / SFA node."""
    if isinstance(node, N.SFANode):
        return node.sf, -node._bias[0]
    return node.v, -(node.avg[0] @ node.v)


@pytest.mark.parametrize("make", [hoist_cases.small_net, lambda: hoist_cases.chain_net(dims=[(5, 6), (7, 9), (8, 12), (10, 12), (9, 7)], side=16)])
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
