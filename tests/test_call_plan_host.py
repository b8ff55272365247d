"""CPU: the executor's per-call launch rules (csrc/hg_fused_call.cpp: plan_call and its second phase) through the planner's stand-alone
driver (tests/hoist_plan_driver.cpp --call / --rule: the blob parser, the planner and the call plan alone, nothing of HIP).  The
library's own rule is held to its restatements in tests/stage_shape_cases.py and to the literal tables tests/test_stage_shapes_plan_host.py
pins those to; sweep_tile_parts and the ordinary sweep's shapes to values worked out by hand; the k_stage_splitm and k_igfold_split
lines; invariants of the step list over every net the plan tests know; and one run of the same driver under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import blob
from tests import fold01_cases, hoist_cases, pair_cases, plan_cases
from tests import stage_shape_cases as cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

STEP = re.compile(r"step (\w+) stage (\d+) covered (\d+) summed (\d) set (-?\d+) blocks (-?\d+) \| (.*)")
PLAN = re.compile(r"plan stages (\d+) fuse01 (\d) fold01 (\d) tail_begin (-?\d+)")
TILES = (1, 2, 3, 4, 8, 9, 27, 64, 65, 109, 256, 257, 512, 1024)
SWEEPS = ("sweep", "sumpair")      # both run the node-group sweep (k_stage, k_stage_sum / k_stage_sum_pair)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("call_plan") / "plan_driver"
    b = hoist_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def call_plans(exe, tmp_path, named_blobs, tiles, env=None, args=(), tag="c", sanitized=False):
    """{name: None (the planner refuses the net) or (plan facts, {tiles: [step dicts]})} of one driver run."""
    files = []
    for k, (_, b) in enumerate(named_blobs):
        p = tmp_path / ("%s%d.bin" % (tag, k))
        p.write_bytes(b)
        files.append(str(p))
    e = {k: v for k, v in os.environ.items() if not k.startswith("HIGSFA_")}
    e.update(env or {})
    if sanitized:
        e.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "--call", ",".join(str(t) for t in tiles)] + list(args) + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=e)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
    parts = text.split("== ")[1:]
    assert len(parts) == len(named_blobs)
    out = {}
    for (name, _), part in zip(named_blobs, parts):
        lines = part.splitlines()[1:]
        assert not lines[0].startswith("failed"), (name, lines[0])
        if lines[0].startswith("refused"):
            out[name] = None
            continue
        m = PLAN.match(lines[0])
        facts = dict(zip(("stages", "fuse01", "fold01", "tail_begin"), (int(g) for g in m.groups())))
        calls, cur = {}, None
        for ln in lines[1:]:
            if ln.startswith("call tiles "):
                cur = calls.setdefault(int(ln.split()[2]), [])
                continue
            m = STEP.match(ln)
            assert m, (name, ln)
            cur.append(dict(route=m.group(1), stage=int(m.group(2)), covered=int(m.group(3)), summed=int(m.group(4)), set=int(m.group(5)),
                            blocks=int(m.group(6)), line=m.group(7)))
        assert sorted(calls) == sorted(tiles), name
        out[name] = (facts, calls)
    return out


def shape_launches(steps):
    """The product and iGSFA sweeps of a step list, as tests/test_stage_shapes_gpu.py reads them from the device's lines."""
    out = []
    for st in steps:
        m = re.match(cases.PROD_LINE, st["line"])
        if m:
            v = [int(g) for g in m.groups()]
            assert st["route"] == "prod"
            out.append(dict(kind="prod", stage=v[0], nodes=v[1], widths=(v[2], v[3]), shape=(v[5], v[6])))
        m = re.match(cases.IG_LINE, st["line"])
        if m:
            v = [int(g) for g in m.groups()]
            assert st["route"] == "igsweep"
            out.append(dict(kind="igsfa", stage=v[0], nodes=v[1], kb1=v[2], shape=(v[3], v[4]), tile_groups=v[7]))
    return out


def by_switches(nets):
    groups = {}
    for name, (make, env) in nets.items():
        groups.setdefault(tuple(sorted(env.items())), []).append((name, blob.flow_to_blob(make())))
    return groups


@pytest.fixture(scope="module")
def shape_plans(driver, tmp_path_factory):
    """Every net of tests/stage_shape_cases.py under its own switches at the tile counts of cases.ROWS."""
    tmp = tmp_path_factory.mktemp("shape_plans")
    out = {}
    for gi, (env, members) in enumerate(by_switches(cases.nets()).items()):
        out.update(call_plans(driver, tmp, members, [cases.tiles(n) for n in cases.ROWS], dict(env), tag="g%d_" % gi))
    return out


def test_product_and_igsfa_steps_are_the_restated_rules(shape_plans):
    """plan_call's product and iGSFA sweeps of every net and batch size of the stage-shape tests are exactly what cases.prod_shape /
    cases.ig_shape say (cases.expected_launches, which the GPU test holds the device's debug lines to): kind, stage, nodes, shape, tile
    widths and K-blocks; an iGSFA shape is the fallback exactly where no candidate gave every CU a workgroup."""
    assert set(shape_plans) == set(cases.nets())
    for name, plan in shape_plans.items():
        assert plan is not None, name
        for rows in cases.ROWS:
            t = cases.tiles(rows)
            got, want = shape_launches(plan[1][t]), cases.expected_launches(name, rows)
            assert [(g["kind"], g["stage"], g["nodes"], g["shape"]) for g in got] == [(w["kind"], w["stage"], w["nodes"], w["shape"]) for w in want], (name, rows)
            for g, w in zip(got, want):
                if g["kind"] == "prod":
                    assert g["widths"] == w["widths"]
                else:
                    assert g["kb1"] == w["kb1"]
                    chosen = g["shape"] in ((12, 2), (8, 2), (4, 2)) and g["shape"][0] * g["shape"][1] <= t and g["tile_groups"] * g["nodes"] >= 256
                    assert chosen == (not w["fallback"]), (name, rows)


def test_literal_shape_tables(shape_plans, driver, tmp_path):
    """The same steps against the literal tables of tests/test_stage_shapes_plan_host.py: PROD_SHAPES_64 on every 64-node product layer;
    c6 on ig_c's 64 nodes of 6 blocks, c4 on ig_e's 64 nodes of 4 blocks, f on igfold1's 256 folded nodes; and the line between
    k_igfold_split and k_igfold at 8 x 2048 | 8 x 2049 tiles."""
    def shapes(name, stage):
        return {n: [g["shape"] for g in shape_launches(shape_plans[name][1][cases.tiles(n)]) if g["stage"] == stage] for n in cases.ROWS}
    for a, b in cases.PROD_PAIRS:
        assert shapes("prod%d%d" % (a, b), 1) == {n: [s] for n, s in cases.PROD_SHAPES_64.items()}
    assert shapes("prod_uneven", 1) == {n: [s] for n, s in cases.PROD_SHAPES_64.items()}
    c6 = {1: (1, 1), 17: (1, 2), 70: (2, 2), 195: (4, 2), 425: (4, 2), 805: (8, 2), 1738: (12, 2)}
    assert cases.IG_UNFOLDED["c"]["want"][0] == (64, 1, 3, 6) and cases.IG_UNFOLDED["e"]["want"][0] == (64, 3, 4, 4)
    assert shapes("ig_c", 1) == {n: [s] for n, s in c6.items()}
    assert shapes("ig_e", 1) == {n: [s] for n, s in {**c6, 1738: (8, 2)}.items()}
    f = {1: (1, 1), 17: (1, 2), 70: (2, 2), 195: (4, 2), 425: (8, 2), 805: (8, 2), 1738: (8, 2)}
    assert cases.IG_FOLDED[1]["want"][0] == (256, 1, 6)
    assert shapes("igfold1", 1) == {n: [s] for n, s in f.items()}
    t0, t1 = (cases.tiles(n) for n in cases.SPLIT_LINE_ROWS)
    assert (8 * t0, 8 * t1) == (16384, 16392)
    line = call_plans(driver, tmp_path, [("s", blob.flow_to_blob(cases.ig_split_line_net()))], (t0, t1))["s"][1]
    assert [(s["route"], s["stage"]) for s in line[t0]][1] == ("igsplit", 1) and line[t0][1]["line"].startswith("[igsplit stage 1] nodes 8 ")
    assert [(s["route"], s["stage"]) for s in line[t1]][1] == ("igsweep", 1)
    assert [(g["nodes"], g["kb1"], g["shape"]) for g in shape_launches(line[t1])] == [(8, 5, (8, 2))] and shape_launches(line[t0]) == []


def rule(exe, *args):
    r = subprocess.run([str(exe), "--rule"] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0, r.stdout
    return r.stdout.decode().strip()


def test_sweep_tile_parts_by_hand(driver):
    """cost(parts) = ceil(groups padded to 8 x parts / (256 occ)) x (0.35 + ceil(tile_groups / parts)), the smallest parts of the least
    cost.  64 groups, 8 tile groups, one workgroup per CU: parts 1 .. 4 fit one round (8.35, 4.35, 3.35, 2.35), 5 .. 8 need two
    (8: 2 x 1.35 = 2.7): 4.  Two per CU: parts 8 is one round of 1.35: 8.  256 groups, 4 tile groups: every part is a round more
    (4.35, 2 x 2.35, 3 x 2.35, 4 x 1.35): 1."""
    assert rule(driver, "parts", 64, 8, 1) == "4"
    assert rule(driver, "parts", 64, 8, 2) == "8"
    assert rule(driver, "parts", 256, 4, 1) == "1"


def test_ordinary_sweep_shapes_by_hand(driver):
    """The first of 8x2, 8x1, 4x2, 4x1 with waves x tiles <= batch tiles and ceil(tiles / (waves x tiles)) x node groups >= 256, else
    4x1, its waves halved while the workgroup holds more tiles than the batch.  32 node groups: 256 tiles give 16 tile groups of 8x2
    (512); 64 tiles 4 of 8x2 (128), 8 of 8x1 (256); 32 tiles 2, 4, 4 (64, 128, 128) and 8 of 4x1 (256); 16 tiles reach 128 at
    most: the default; 2 tiles and 1 tile shrink it."""
    want = {256: "8x2", 64: "8x1", 32: "4x1", 16: "4x1", 2: "2x1", 1: "1x1"}
    assert {t: rule(driver, "sweep", t, 32) for t in want} == want


def test_splitm_line(driver, tmp_path):
    """mixed_net's top layer has one node (at most 4: k_stage_splitm takes it while nodes x tiles <= 8192).  Without the top-of-hierarchy
    launch (HIGSFA_TAIL=0) 8192 tiles are on the k_stage_splitm side of the line, 8193 on the sweep's."""
    got = call_plans(driver, tmp_path, [("m", blob.flow_to_blob(cases.mixed_net()))], (8192, 8193), {"HIGSFA_TAIL": "0"})["m"][1]
    assert [(s["route"], s["stage"]) for s in got[8192]][-1] == ("splitm", 3) and got[8192][-1]["line"].startswith("[splitm stage 3] nodes 1 ")
    assert [(s["route"], s["stage"]) for s in got[8193]][-1] == ("sweep", 3) and got[8193][-1]["line"].startswith("[sweep stage 3] nodes 1 ")


def invariant_nets():
    """[(name, switches, blob)]: every net of the plan, hoist, pair, fold and stage-shape tests (plan_cases has the synthetic U11L-128,
    U11L-64 and the 96-pixel U11L among its own)."""
    out = [(name, dict(env), b) for name, env, b in plan_cases.cases()]
    flows = {"chain": hoist_cases.chain_net(), "quad": hoist_cases.quad_net(), "small": hoist_cases.small_net(), "ragged": hoist_cases.ragged_net(),
             "ragged18": hoist_cases.ragged_net(p3=18), "ragged_wide": hoist_cases.ragged_wide_net(), "order_probe": hoist_cases.order_probe_net(),
             "igsfa_after_ordinary": hoist_cases.igsfa_after_ordinary(), "three_pair": pair_cases.three_pair_net(), "igsfa_layer1": fold01_cases.igsfa_layer1_net()}
    flows.update({"hoist_fuzz_%d" % s: hoist_cases.hoist_fuzz_net(s) for s in hoist_cases.HOIST_FUZZ_SEEDS})
    flows.update({"fold_" + k: make() for k, make in fold01_cases.HOST_NETS.items()})
    flows.update({"fold_gpu_" + k: make() for k, make in fold01_cases.GPU_NETS.items()})
    flows.update({"fold_refused_" + k: make() for k, (make, env, _) in fold01_cases.REFUSED.items() if not env})
    out += [(name, {}, blob.flow_to_blob(f)) for name, f in flows.items()]
    out += [(name, dict(env), blob.flow_to_blob(make())) for name, (make, env) in cases.nets().items()]
    sweep_only = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0", "HIGSFA_SUM_LDS": "128", "HIGSFA_PAIR_WGS": "1"}
    out.append(("three_pair+sweep_only", sweep_only, blob.flow_to_blob(flows["three_pair"])))      # tests/test_pair_gpu.py's switches: summed links at every size
    for name in ("U11L-128", "U11L-64"):      # the link 0 -> 1 fused but not folded
        out.append((name + "+HIGSFA_NO_FOLD01", {"HIGSFA_NO_FOLD01": "1"}, [b for n, _, b in plan_cases.cases() if n == name][0]))
    out.append(("fold_w13_p20_s17+HIGSFA_NO_FOLD01", {"HIGSFA_NO_FOLD01": "1"}, blob.flow_to_blob(fold01_cases.HOST_NETS["w13_p20_s17"]())))
    return out


def check_steps(name, facts, tiles, steps, vec4):
    ns = facts["stages"]
    assert sum((list(range(s["stage"], s["stage"] + s["covered"])) for s in steps), []) == list(range(ns)), (name, tiles)
    assert all(s["route"] != "top" for s in steps[:-1]), (name, tiles)
    if steps[-1]["route"] == "top":
        assert facts["tail_begin"] >= 0 and steps[-1]["stage"] >= facts["tail_begin"]
    assert len({s["set"] for s in steps if s["route"] == "subtree"}) <= 1, (name, tiles)
    assert all(s["set"] == -1 for s in steps if s["route"] != "subtree")
    for i, s in enumerate(steps):
        assert s["blocks"] > 0, (name, tiles, s)
        if s["summed"]:
            assert s["route"] in SWEEPS and i > 0 and steps[i - 1]["route"] == "sumpair", (name, tiles, s)
        if s["route"] == "sumpair":
            nxt = steps[i + 1]
            assert nxt["route"] in SWEEPS and nxt["summed"] and nxt["stage"] == s["stage"] + 1 and s["covered"] == 1, (name, tiles, s)
        if s["route"] in ("front01d", "front01p", "front0p", "front0", "gather"):
            assert i == 0 and s["stage"] == 0
        if s["route"] not in ("subtree", "top"):
            assert s["covered"] == (2 if s["route"] in ("front01d", "front01p") else 1), (name, tiles, s)
    front = steps[0]
    pair = front["route"] in ("front01d", "front01p")
    if not facts["fuse01"]:
        assert not pair, (name, tiles)
    elif facts["fold01"]:
        assert pair and (vec4 or front["route"] == "front01p"), (name, tiles)      # a folded plan has one arithmetic: the pair kernels'
    elif not vec4:
        assert not pair, (name, tiles)      # an unfolded plan: the unfused kernels
    elif tiles >= 2:
        assert pair, (name, tiles)          # (a pass of the pair kernels is one or two tiles)
    return pair


def test_route_invariants(driver, tmp_path):
    """Over every net of the plan tests, at tile counts around every threshold: the steps cover every stage exactly once, in ascending
    order; a top step is last; all sub-tree steps of a call come from one set; a step that reads a summed link runs the node-group
    sweep right after the summed-pair step that stored it, and every summed-pair step is followed by such a reader; every grid is
    positive; the front step covers two stages exactly when the plan fused layers 0 and 1 and the pair kernels take the call.
    Without 16-byte loads (--no-vec4) an unfolded plan goes to the unfused kernels and a folded plan stays on k_stage01p."""
    groups = {}
    for name, env, b in invariant_nets():
        groups.setdefault(tuple(sorted(env.items())), []).append((name, b))
    seen = {"planned": 0, "pair": 0, "unfolded_pair": 0, "folded_novec": 0, "unfolded_novec": 0, "sumpair": 0, "subtree": 0, "top": 0}
    for gi, (env, members) in enumerate(groups.items()):
        for vec4 in (True, False):
            got = call_plans(driver, tmp_path, members, TILES, dict(env), () if vec4 else ("--no-vec4",), tag="i%d_%d_" % (gi, vec4))
            for name, plan in got.items():
                if plan is None:
                    continue
                facts, calls = plan
                seen["planned"] += vec4
                for t in TILES:
                    pair = check_steps(name, facts, t, calls[t], vec4)
                    seen["pair"] += pair and vec4
                    seen["unfolded_pair"] += pair and vec4 and not facts["fold01"]
                    seen["folded_novec"] += pair and not vec4
                    seen["unfolded_novec"] += bool(facts["fuse01"]) and not facts["fold01"] and not vec4
                    for k in ("sumpair", "subtree", "top"):
                        seen[k] += any(s["route"] == k for s in calls[t])
    assert all(seen.values()), seen      # every clause above was reached


def test_call_plan_under_asan_ubsan(tmp_path):
    """The same driver built with AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program) plans every call of the
    stage-shape nets."""
    exe = tmp_path / "plan_driver_asan"
    r = hoist_cases.build_driver(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        pytest.skip("sanitizer build not possible here: " + r.stdout.decode(errors="replace")[-300:])
    n = 0
    for gi, (env, members) in enumerate(by_switches(cases.nets()).items()):
        got = call_plans(exe, tmp_path, members, [cases.tiles(n_) for n_ in cases.ROWS] + [1024], dict(env), tag="a%d_" % gi, sanitized=True)
        assert all(p is not None for p in got.values())
        n += len(got)
    assert n == len(cases.nets())
