"""CPU: the premises of tests/test_ordinary_stages_gpu.py, through the planner's stand-alone driver (tests/hoist_plan_driver.cpp --call /
--rule: the blob parser, the planner and the call plan alone, nothing of HIP).  Every (net, switches, rows) of
tests/ordinary_stage_cases.py is planned and its sweep, split-m and first-layer steps are held to the literal tables of the cases
file: route, shape, kbf, fs, rem4, pk, nodes per group, tile groups and tile parts.  Over their union every instantiation pick_stage
(csrc/hg_fused.hip) can return, both T and both REM forms of k_stage_splitm at every (mt1n, mt2n), and the k_stage0 forms.
stage_sweep_shape is held to its restatement over a grid, with the fact that its candidate 4 x 2 is never chosen.  One run of the
same driver is built with AddressSanitizer and UndefinedBehaviorSanitizer.  Conditions on the tests' inputs, not measurements: if a
generator drifts, change the net, not the tables."""
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import blob
from tests import hoist_cases
from tests import ordinary_stage_cases as cases
from tests.test_call_plan_host import call_plans

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
NETS = cases.nets()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ordinary_stages") / "plan_driver"
    b = hoist_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def plan_all(exe, tmp, names, sanitized=False, args=(), tag="o"):
    """{name: {tiles: [launch dicts]}} of the named nets, one driver run per (switches, batch sizes)."""
    groups = {}
    for name in names:
        _, make, env, rows = NETS[name]
        groups.setdefault((tuple(sorted(env.items())), rows), []).append((name, blob.flow_to_blob(make())))
    out = {}
    for gi, ((env, rows), members) in enumerate(groups.items()):
        got = call_plans(exe, tmp, members, sorted({cases.tiles(n) for n in rows}), dict(env), args, tag="%s%d_" % (tag, gi), sanitized=sanitized)
        for name, plan in got.items():
            assert plan is not None, name
            out[name] = {t: cases.launches("\n".join(s["line"] for s in steps)) for t, steps in plan[1].items()}
            for t, steps in plan[1].items():      # every stage of a call named exactly once, by a line the GPU test can read
                assert cases.covered_stages("\n".join(s["line"] for s in steps)) == list(range(plan[0]["stages"])), (name, t)
    return out


@pytest.fixture(scope="module")
def plans(driver, tmp_path_factory):
    return plan_all(driver, tmp_path_factory.mktemp("ordinary_plans"), list(NETS))


def test_every_case_launches_what_the_tables_say(plans):
    """plan_call on every (net, switches, rows): the steps above the first-layer kernel are exactly cases.want — route, stage, nodes,
    tile widths, K-blocks, shape, nodes per group, node groups, tile groups, tile parts (one workgroup per CU), kbf, fs, rem4, pk; for
    k_stage_splitm T, waves, the REM form and the grid.  The first step is the first-layer kernel's ("[front0]": no net here fuses
    layers 0 and 1, none needs a gather)."""
    assert set(plans) == set(NETS)
    for name, (_, _, _, rows) in NETS.items():
        for n in rows:
            got = plans[name][cases.tiles(n)]
            assert got[0]["route"] == "front0", (name, n)
            assert cases.held(got[1:], cases.want(name, n)), (name, n, got[1:], cases.want(name, n))


def test_the_tables_hold_the_design_of_each_family():
    """The tables themselves, against the design they were made for.  Family 1: 1 x 1, 2 x 1 and 4 x 1 at 1, 2 and 5 tiles for every
    pair; 8 x 1 first at 109, 51, 27 or 13 tiles by pair; 8 x 2 at 163 tiles (odd: the last wave's second tile is absent); nodes per
    group 10, 8, 6, 5, 4, 3, 2, 1 with a short last group where they do not divide 256; tile_groups > parts > 1 at (1, 1): 11 over 6;
    kbf 4 at T = 2 for (2, 2) and (3, 3) alone.  Family 2: the first 8 x 2 of each remainder net and its prefetch form.  Family 3:
    where k_stage_splitm ends."""
    assert [cases.tiles(n) for n in cases.ROWS] == [1, 2, 5, 13, 27, 51, 109, 163]
    first_8x1 = {109: [(1, 1), (1, 2)], 51: [(1, 3), (1, 4), (2, 1)], 27: [(2, 2), (2, 3), (3, 1)]}
    npgs = set()
    for pr in cases.PAIRS:
        name = "ord%d%d" % pr
        sh = {cases.tiles(n): cases.want(name, n)[0] for n in cases.ROWS}
        assert [sh[t]["shape"] for t in (1, 2, 5)] == [(1, 1), (2, 1), (4, 1)] and sh[163]["shape"] == (8, 2), name
        t81 = [t for t in sorted(sh) if sh[t]["shape"] == (8, 1)]
        assert t81[:1] == [next((t for t, prs in first_8x1.items() if pr in prs), 13)], name
        assert {sh[t]["shape"] for t in sh} == {(1, 1), (2, 1), (4, 1), (8, 1), (8, 2)}, name
        assert {sh[t]["kbf"] for t in sh if sh[t]["shape"][1] == 2} == ({4} if pr in ((2, 2), (3, 3)) else {0}), name
        assert all(sh[t]["fs"] == 1 and sh[t]["rem4"] == 0 and sh[t]["ng"] == -(-256 // sh[t]["npg"]) for t in sh)
        npgs.add(sh[1]["npg"])
    assert npgs == {10, 8, 6, 5, 4, 3, 2, 1}
    top = cases.want("ord11", 2600)[0]
    assert (top["tile_groups"], top["parts"]) == (11, 6) and 256 % top["npg"]
    assert [cases.want("ordgen%d%d" % (m, m), 2600)[0]["fs"] for m in (3, 4)] == [0, 0]
    first_8x2 = {"remA2": (163, 4), "remA3": (51, 4), "remB2": (109, 3), "remB3": (51, 3)}
    for name, (t0, kbf) in first_8x2.items():
        for tag, fs in (("", 1), ("+gen", 0)):
            sh = {cases.tiles(n): cases.want(name + tag, n)[0] for n in cases.ROWS}
            assert min(t for t in sh if sh[t]["shape"] == (8, 2)) == t0 and sh[t0]["kbf"] == kbf, name
            assert all(sh[t]["rem4"] == 1 and sh[t]["fs"] == fs for t in sh)
            off = {cases.tiles(n): cases.want(name + tag + "+norem4", n)[0] for n in cases.ROWS}
            assert all(off[t]["rem4"] == 0 and off[t]["shape"] == sh[t]["shape"] for t in off)
            assert off[t0]["kbf"] == (4 if kbf == 4 else 0)      # three K-blocks are prefetched whole only with remainder tiles
    for mt in (2, 3):
        for tag in ("", "+gen"):
            assert [s["pk"] for s in cases.want("pk%d%s" % (mt, tag), 2600)] == [-1, 1] and cases.want("pk%d%s" % (mt, tag), 2600)[1]["kbf"] == 3
            assert [s["pk"] for s in cases.want("pk%d%s+nosoa" % (mt, tag), 2600)] == [-1, -1] and cases.want("pk%d%s+nosoa" % (mt, tag), 2600)[1]["kb1"] == 3
            assert cases.want("pk%d%s+nopack" % (mt, tag), 2600)[1]["kb1"] == 4
    # family 3: the 256-node layer on k_stage_splitm at 1 .. 4 tiles (T = 2 from two), waves = max(mt1, mt2); the sweep from five
    for pr in cases.PAIRS:
        w = {cases.tiles(n): cases.want("ord%d%d:d" % pr, n)[0] for n in cases.ROWS_ORD_D}
        assert [(w[t]["route"], w[t].get("T")) for t in (1, 2, 3, 4)] == [("splitm", 1), ("splitm", 2), ("splitm", 2), ("splitm", 2)]
        assert w[1]["waves"] == max(pr) and w[5]["route"] == "sweep" and w[163]["shape"] == (8, 2)
    for name in ("twin11:d", "twin23:d", "twin32:d", "twin44:d", "nf24:d", "linear:d"):
        w = {cases.tiles(n): cases.want(name, n)[0] for n in cases.ROWS_SMALL}
        assert [(w[t]["route"], w[t].get("T")) for t in (1, 2, 5, 13, 27)] == [("splitm", 1)] * 3 + [("splitm", 2), ("sweep", None)], name
    assert all(cases.want("nf33:d", n)[0]["route"] == "sweep" for n in cases.ROWS_SMALL)      # mt1 x nf = 9: never k_stage_splitm
    assert cases.want("linear:d", 1)[0]["waves"] == 2      # no second affine: mt1 waves


def test_union_of_the_cases_reaches_every_instantiation(plans, driver, tmp_path):
    """From the planned steps (not from the tables): every one of pick_stage's 49 k_stage instantiations, k_stage_splitm<T, REM> for both
    T and both REM, at all 16 run-time (mt1n, mt2n) for T = 1 and T = 2 without remainder tiles, and the REM form at (2, 2) and (3, 3),
    the only widths a remainder-tile stage has; a T = 2 launch of either kernel on an odd tile count; tile_groups > parts > 1 with a
    short last node group."""
    sweeps, splits = [], []
    for name, by_tiles in plans.items():
        for t, ls in by_tiles.items():
            sweeps += [dict(l, tiles=t, name=name) for l in ls if l["route"] == "sweep"]
            splits += [dict(l, tiles=t, name=name) for l in ls if l["route"] == "splitm"]
    assert {cases.instantiation(l) for l in sweeps} == cases.pick_stage_instantiations()
    assert {l["shape"] for l in sweeps} == {(8, 2), (8, 1), (4, 1), (2, 1), (1, 1)}      # 4 x 2 is never chosen: see the rule's test
    assert {(l["T"], l["mt"]) for l in splits if not l["rem4"]} >= {(T, pr) for T in (1, 2) for pr in cases.PAIRS}
    assert {(l["T"], l["mt"]) for l in splits if l["rem4"]} == {(T, (m, m)) for T in (1, 2) for m in (2, 3)}
    assert any(l["T"] == 2 and l["tiles"] % 2 for l in splits) and any(l["T"] == 2 and l["tiles"] % 2 and l["rem4"] for l in splits)
    assert any(l["shape"] == (8, 2) and l["tiles"] % 2 for l in sweeps)
    assert any(l["tile_groups"] > l["parts"] > 1 and l["nodes"] % l["npg"] for l in sweeps)
    # the K-blocks of the nets around k_stage_splitm's batch of eight (the split-m line does not carry them: the sweep's does)
    kb = call_plans(driver, tmp_path, [(str(k), blob.flow_to_blob(cases.kb_net(k))) for k in cases.KB_NODES], (1,), cases.SWEEP_ONLY, tag="kb")
    assert {k: [(l["nodes"], l["kb1"]) for l in cases.launches(kb[k][1][1][1]["line"])] for k in kb} == {str(k): [(n, k)] for k, n in cases.KB_NODES.items()}
    assert {l["name"] for l in splits if l["name"].startswith("kb")} == {"kb%d:d" % k for k in cases.KB_NODES}


def test_sweep_rule_and_the_candidate_that_is_never_chosen(driver):
    """stage_sweep_shape over tiles 1 .. 300 x node groups 1 .. 300 against cases.sweep_shape.  Its candidates are 8x2, 8x1, 4x2, 4x1 in that
    order, each taken when waves x tiles <= batch tiles and ceil(batch tiles / (waves x tiles)) x groups >= 256: the condition of 4 x 2
    is the condition of 8 x 1 (eight tiles per tile group either way), which stands before it — 4 x 2 is never returned, so the ordinary
    sweep runs T = 2 only as 8 x 2.  (Pinned, not changed here: DESIGN.md §6.13.)"""
    r = subprocess.run([str(driver), "--rule", "sweepgrid", "300", "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    assert len(rows) == 300 and all(len(row) == 300 for row in rows)
    for t in range(1, 301):
        assert rows[t - 1] == ["%dx%d" % cases.sweep_shape(t, g) for g in range(1, 301)], t
    seen = {v for row in rows for v in row}
    for t, g in ((1, 1), (8, 32), (16, 32), (163, 26), (300, 300)):      # the single-point form, which the by-hand tests use, is the same rule
        one = subprocess.run([str(driver), "--rule", "sweep", str(t), str(g)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert one.returncode == 0 and one.stdout.decode().strip() == rows[t - 1][g - 1]
    assert seen == {"8x2", "8x1", "4x1", "2x1", "1x1"}
    # sweep_tile_parts against cases.tile_parts, which holds the device's lines at the occupancy they report
    for g in (1, 9, 26, 36, 86, 128, 256):
        for tg in (1, 2, 4, 7, 11, 14, 33):
            for occ in (1, 2, 3, 4):
                one = subprocess.run([str(driver), "--rule", "parts", str(g), str(tg), str(occ)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
                assert one.returncode == 0 and int(one.stdout.decode()) == cases.tile_parts(g, tg, occ), (g, tg, occ)
    assert all(cases.sweep_shape(t, g) != (4, 2) for t in range(1, 301) for g in range(1, 301))


def test_front_steps(driver, tmp_path):
    """Family 4: one-layer nets of every tile-width pair at 3, 4 and 5 tiles: the step is the first-layer kernel's alone; T = 1 below
    four tiles, T = 4 from four tiles where mt1 x mt2 <= 4, T = 1 above that product; persistent (k_stage0p) at (1, 1) alone; without
    16-byte loads (--no-vec4) never persistent, the same T."""
    members = [("front%d%d" % pr, blob.flow_to_blob(cases.front_net(*pr))) for pr in cases.PAIRS]
    t = sorted({cases.tiles(n) for n in cases.FRONT_ROWS})
    assert t == [3, 4, 5]
    for vec4 in (True, False):
        got = call_plans(driver, tmp_path, members, t, {}, () if vec4 else ("--no-vec4",), tag="f%d_" % vec4)
        for pr in cases.PAIRS:
            facts, calls = got["front%d%d" % pr]
            assert facts["stages"] == 1
            for n in cases.FRONT_ROWS:
                ls = cases.launches("\n".join(s["line"] for s in calls[cases.tiles(n)]))
                assert ls == [cases.front_want(pr, n, vec4)], (pr, n, vec4)
    assert sum(cases.front_want(pr, 64)["T"] == 4 for pr in cases.PAIRS) == 8 and sum(cases.front_want(pr, 64)["persistent"] for pr in cases.PAIRS) == 1
    assert all(cases.front_want(pr, 48)["T"] == 1 for pr in cases.PAIRS)


def test_ordinary_call_plans_under_asan_ubsan(tmp_path):
    """The same driver built with AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program) plans one net of every
    family and switch set at its batch sizes, to the same tables."""
    exe = tmp_path / "plan_driver_asan"
    r = hoist_cases.build_driver(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        pytest.skip("sanitizer build not possible here: " + r.stdout.decode(errors="replace")[-300:])
    names = ["ord33", "remB3+gen+norem4", "pk3+gen+nosoa", "remB2:d", "kb17:d", "nf33:d", "linear:d"]
    got = plan_all(exe, tmp_path, names, sanitized=True, tag="a")
    for name in names:
        for n in NETS[name][3]:
            assert cases.held(got[name][cases.tiles(n)][1:], cases.want(name, n)), (name, n)
