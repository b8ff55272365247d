"""CPU: the fused planner (csrc/hg_fused_plan.cpp) as a host-only unit.  A stand-alone driver linked against the blob parser
and the planner alone — no HIP library — prints every plan (tests/plan_digest.hpp: all scalars, an FNV-1a 64 digest of every
packed array, the sub-tree runs, the per-call choices around their edges), and the output is compared line by line with
tests/golden/fused_plan_digests.json, which was recorded from the commit BEFORE the planner was split out of hg_fused.hip (its
make_fused_executor patched to print the same lines through the same routine), not from this code.

No linear-algebra result may reach a digest (tests/plan_cases.py): every weight is a draw of a seeded numpy Generator, the
presets are structures only, so the recorded file holds on any machine."""
import re
import shutil

import pytest

from tests import plan_cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def golden():
    return plan_cases.load_golden()


def test_plans_match_the_recorded_digests(tmp_path, golden):
    exe = tmp_path / "plan_digest_driver"
    b = plan_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    got = plan_cases.run_driver(exe, tmp_path)
    assert sorted(got) == sorted(golden)
    for name in sorted(got):
        assert len(got[name]) == len(golden[name]), name
        for k, (a, e) in enumerate(zip(got[name], golden[name])):
            assert a == e, "%s, line %d:\n  planned  %s\n  recorded %s" % (name, k, a, e)


def test_recorded_plans_cover_every_planner_branch(golden):
    """The recorded plans hold each branch of the planner at least once: 4x4 remainder tiles, packed remainder blocks lane- and
    slot-major, the fused front kernel and its direct form, the four stage kinds, a folded and an unfolded iGSFA stage, a
    top-of-hierarchy launch of one layer and of three, sub-tree runs of both sets, and a refusal."""
    stages, tail_layers, sets, fuse01 = [], set(), set(), set()
    for lines in golden.values():
        if not lines[0].startswith("stage fields: "):
            continue
        fields = lines[0].split(": ")[1].split()
        mine = [dict(zip(fields, ln.split(": ", 1)[1].split())) for ln in lines if re.match(r"stage \d+: ", ln)]
        assert mine and all(len(s) == len(fields) for s in mine)
        stages += mine
        for ln in lines:
            m = re.match(r"plan: .* tail_begin=(-?\d+) .* fuse01=(\d)", ln)
            if m:
                fuse01.add(int(m.group(2)))
                tail_layers.add(len(mine) - int(m.group(1)) if int(m.group(1)) >= 0 else 0)
            m = re.match(r"sub-run \d+: .* set=(\d)", ln)
            if m:
                sets.add(int(m.group(1)))
    for flag in ("rem4", "pack_out", "pack_soa", "direct_ok"):
        assert any(s[flag] == "1" for s in stages), flag
    assert {s["kind"] for s in stages} == {"0", "1", "2", "3"}
    assert any(s["pack_out"] == "1" and s["pack_soa"] == "0" for s in stages)
    assert {s["ig_folded"] for s in stages if s["kind"] == "2"} == {"0", "1"}
    assert {0, 1, 3} <= tail_layers and sets == {0, 1} and fuse01 == {0, 1}
    refused = [lines for lines in golden.values() if lines[0].startswith("refused: ")]
    assert refused and any("LDS" in lines[0] for lines in refused)


def test_preset_structures_are_the_presets(nets):
    """plan_cases.preset_structure builds what synth.build_preset trains, weights aside (checked on the presets that train in a
    moment; the U11L presets follow the same rules from the same table)."""
    for name, kind in (("T3L-8", "pca_exp_sfa"), ("T5L-16", "pca_exp_sfa"), ("T5L-16", "igsfa")):
        trained = nets(name, node_kind=kind) if kind != "pca_exp_sfa" else nets(name)
        built = plan_cases.preset_structure(name, kind)
        assert [plan_cases.shape_of(n) for n in built] == [plan_cases.shape_of(n) for n in trained], (name, kind)
