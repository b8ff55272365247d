"""CPU: what the planner records for summed links (Planner::plan_pairs, csrc/hg_fused_plan.cpp) through a stand-alone
driver with its own main (tests/pair_plan_driver.cpp, linked against the blob parser and the planner alone).  A hoisted stage whose
nodes all have exactly two children gets pair_kids, kb1tab_pre and bias_pre; every other hoisted stage stays unpaired and says so on
its line; a plan without hoisted links is the recorded one."""
import re
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import blob
from tests import hoist_cases, pair_cases, plan_cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair") / "pair_plan_driver"
    b = pair_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def run(driver, tmp_path, named_blobs, *flags):
    files = []
    for k, (_, b) in enumerate(named_blobs):
        p = tmp_path / ("p%d.bin" % k)
        p.write_bytes(b)
        files.append(str(p))
    r = subprocess.run([str(driver)] + list(flags) + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    parts = text.split("== ")[1:]
    assert len(parts) == len(named_blobs)
    return {name: part.splitlines()[1:] for (name, _), part in zip(named_blobs, parts)}


def parse(lines):
    """({hoisted stage: [children per node]} of the normal form, {stage: {field: value, name, kids, tab, bias, biaspre}} of the plan)."""
    links, stages = {}, {}
    for ln in lines:
        head, _, rest = ln.partition(": ")
        w = head.split()
        if w[0] == "link":
            links.setdefault(int(w[1]), []).append([int(v) for v in rest.split()])
            assert len(links[int(w[1])]) == int(w[2]) + 1
        elif w[0] == "stage":
            v = rest.split()
            stages[int(w[1])] = {k: int(x) for k, x in zip(v[0::2], v[1::2])}
        elif w[0] == "name":
            stages[int(w[1])]["name"] = rest
        elif w[0] in ("kids", "tab"):
            stages[int(w[1])][w[0]] = [int(v) for v in rest.split()]
        elif w[0] in ("bias", "biaspre"):
            stages[int(w[1])][w[0]] = rest.split()
        else:
            raise AssertionError(ln)
    return links, stages


def check_paired(links, stages, si):
    """Stage si is paired, and its tables are what DESIGN.md §6.10 says."""
    s, below = stages[si], stages[si - 1]
    assert s["sum_in"] == 1 and s["paired"] == 1, si
    assert "first affine folded" in s["name"] and "plain 16-row tiles only" in s["name"] and "; paired: " in s["name"]
    n, mt1, bf = s["n_nodes"], s["mt1"], s["bias_floats"]
    kids = [s["kids"][2 * j:2 * j + 2] for j in range(n)]
    assert len(s["kids"]) == 2 * n
    assert kids == links[si]                                               # FNode::kids order: first read
    assert sorted(s["kids"]) == list(range(below["n_nodes"]))              # the pairs partition the child stage
    tab = s["tab"]
    assert len(tab) == 2 * (n * mt1 + 8)                                   # and the eight spare entries every table carries
    for j in range(n):
        for mt in range(mt1):
            assert tab[2 * (j * mt1 + mt):2 * (j * mt1 + mt) + 2] == [j * mt1 + mt, 1]
    assert tab[2 * n * mt1:] == [0] * 16
    assert len(s["bias"]) == len(s["biaspre"]) == n * bf and bf >= mt1 * 16
    for j in range(n):
        assert s["biaspre"][j * bf:j * bf + mt1 * 16] == ["80000000"] * (mt1 * 16)
        assert s["biaspre"][j * bf + mt1 * 16:(j + 1) * bf] == s["bias"][j * bf + mt1 * 16:(j + 1) * bf]
    return kids


def check_unpaired(stages, si, text):
    s = stages[si]
    assert s["sum_in"] == 1 and s["paired"] == 0, si
    assert "first affine folded" in s["name"] and "; unpaired: " + text in s["name"], s["name"]
    assert "kids" not in s and "tab" not in s and "biaspre" not in s


def recorded_blob(name):
    return next(b for n, env, b in plan_cases.cases() if n == name and not env)


def test_two_way_links_are_paired(driver, tmp_path):
    """chain_net's two-way links (parents of 2, 3 and 4 tiles), small_net (its pair is reached through a permuting switchboard: the
    order is first read), U11L-128's links 3 -> 4 .. 9 -> 10 (in every other layer a node's sibling is a row away) and the three-pair
    net, whose first-read order is descending inside a pair."""
    nets = [("chain", blob.flow_to_blob(hoist_cases.chain_net())), ("small", blob.flow_to_blob(hoist_cases.small_net())),
            ("U11L-128", recorded_blob("U11L-128")), ("three", blob.flow_to_blob(pair_cases.three_pair_net()))]
    got = {name: parse(lines) for name, lines in run(driver, tmp_path, nets).items()}
    want = {"chain": [2, 3, 4, 5, 6], "small": [2], "U11L-128": [4, 5, 6, 7, 8, 9, 10], "three": [2, 3, 4]}
    kids = {}
    for name, (links, stages) in got.items():
        assert sorted(links) == want[name]
        assert [si for si in stages if stages[si]["sum_in"]] == want[name]
        for si in stages:
            if si not in want[name]:
                assert stages[si]["paired"] == 0 and "paired" not in stages[si]["name"]
        kids[name] = {si: check_paired(links, stages, si) for si in want[name]}
    assert kids["three"][3] == pair_cases.GROUPS_3 and kids["three"][4] == pair_cases.GROUPS_4
    assert any(a > b for a, b in kids["three"][4]) and any(abs(a - b) > 1 for a, b in kids["three"][3])
    assert [got["three"][1][si][k] for si in (2, 3, 4) for k in ("mt1", "mt2")] == [4] * 6      # the shape the pair kernel is built for
    # U11L-128: siblings adjacent where the layer halves x, a row apart where it halves y
    apart = {si: {abs(a - b) for a, b in kids["U11L-128"][si]} for si in want["U11L-128"]}
    assert any(d != {1} for d in apart.values()) and any(d == {1} for d in apart.values()), apart
    assert got["U11L-128"][1][4]["n_nodes"] == 64 and got["U11L-128"][1][5]["n_nodes"] == 32


def test_other_child_counts_stay_unpaired(driver, tmp_path):
    """quad_net (four children per parent; its last link is a pair merge and is paired), ragged_net (1, 3, 4 and 8 children in one
    layer; two-way links above it) and order_probe_net (three children): unpaired, and described as such on the parent's line."""
    nets = [("quad", blob.flow_to_blob(hoist_cases.quad_net())), ("ragged", blob.flow_to_blob(hoist_cases.ragged_net())),
            ("probe", blob.flow_to_blob(hoist_cases.order_probe_net()))]
    got = {name: parse(lines) for name, lines in run(driver, tmp_path, nets).items()}
    links, stages = got["quad"]
    assert sorted(links) == [2, 3, 4]
    check_unpaired(stages, 2, "4 children per node")
    check_unpaired(stages, 3, "4 children per node")
    check_paired(links, stages, 4)
    links, stages = got["ragged"]
    assert sorted(links) == [2, 3, 4] and links[2] == hoist_cases.RAGGED_GROUPS
    check_unpaired(stages, 2, "1 to 8 children per node")
    check_paired(links, stages, 3)
    check_paired(links, stages, 4)
    links, stages = got["probe"]
    assert links == {2: [[1, 2, 0]]}
    check_unpaired(stages, 2, "3 children per node")


def test_plans_without_hoisted_links_are_the_recorded_ones(driver, tmp_path):
    """FusedOptions::pair rides on ::hoist: with hoist off the planner prints the recorded plan (tests/golden/fused_plan_digests.json),
    line by line, whether pair is on or not — the fields it adds stay empty and no line of a stage changes."""
    names = ("U11L-128", "U11L-64", "T5L-16", "subtree_fuzz_net_0")
    got = run(driver, tmp_path, [(n, recorded_blob(n)) for n in names], "--off")
    golden = plan_cases.load_golden()
    for n in names:
        assert got[n] == golden[n], n
        assert not any(re.search(r"paired|pairs in a plan", ln) for ln in got[n])
