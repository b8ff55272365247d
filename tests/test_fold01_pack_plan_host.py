"""CPU: the planner's packing of the folded link's one-row k-steps (Planner::plan_fold01_pack, csrc/hg_fused_plan.cpp)
through a stand-alone driver with its own main (tests/fold01_pack_plan_driver.cpp, linked against the blob parser and the planner alone).

With FusedOptions::fold01 and fold01_pack on, for the nets of tests/fold01_cases.py, a net whose layer-0 first bias is not zero and
U11L-128: the packed k-step's fragments (fold_last), the folded fragments with register 3 gone, and layer 0's first affine and bias with
the row of feature 12 repeated, element by element against numpy float64 to one float32 ulp and at the stated lane groups — even
child: k-rows 0 and 2 of the packed k-step, tile rows 3 and 11 of its first affine; odd child: k-rows 1 and 3, tile rows 7 and 15, row
3 zero.  With fold01_pack off the whole plan is the one recorded before the option existed.  The refusals and the issued counts."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import blob
from pyfaceanalysis_amd import nodes as N
from tests import fold01_pack_cases as cases
from tests import plan_cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fold01_pack") / "fold01_pack_plan_driver"
    b = cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def run(driver, tmp_path, flow, opts=(), env=None, name="net"):
    p = tmp_path / (name + ".bin")
    p.write_bytes(blob.flow_to_blob(flow))
    e = {k: v for k, v in os.environ.items() if k not in plan_cases.SWITCHES}
    e.update(env or {})
    r = subprocess.run([str(driver)] + list(opts) + [str(p)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=e)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    lines = text.splitlines()
    assert lines[0] == "== %s.bin" % name and lines[1].startswith("fold01 "), lines[:2]
    head = lines[1].split()
    out = {"fold01": int(head[1]), "pack": int(head[3]), "s0_transpose": int(head[5]), "padded_flops": int(head[7]), "given": int(head[9]),
           "note": lines[2][len("note "):], "pack_note": lines[3][len("pack_note "):], "name1": lines[4][len("name1 "):],
           "issue": {int(w[1]): (int(w[2]), int(w[3])) for w in (ln.split() for ln in lines if ln.startswith("issue "))},
           "digest": [ln[2:] for ln in lines if ln.startswith("D ")], "F": {}, "last": {}, "a1": {}, "a1_plain": {}, "b1": {}, "b1_plain": {}}
    for ln in lines[5:]:
        w = ln.split()
        if w[0] == "F":
            out["F"][(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float32).reshape(32, 32)
        elif w[0] == "last":
            out["last"][(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float32)
        elif w[0] in ("a1", "a1_plain"):
            out[w[0]][int(w[1])] = np.array(w[2:], dtype=np.float32).reshape(16, 16)
        elif w[0] in ("b1", "b1_plain"):
            out[w[0]][int(w[1])] = np.array(w[2:], dtype=np.float32)
    return out


def within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


def q_of_row(i):
    return 4 * (i & 3) + (i >> 2)


def first_affine(fnode):
    """(W, b) of z0 = (x - float32(a)) @ W + b for the linear nodes in front of a layer-0 node's expansion, float64: the front kernels
    subtract the mean rounded to float32 and the plan's first bias carries the remainder, (float32(a) - a) @ W."""
    lin = []
    for n in fnode.flow:
        if isinstance(n, N.GeneralExpansionNode):
            break
        lin.append(n)
    W, b = lin[0].v, np.zeros(lin[0].output_dim)
    for n in lin[1:]:
        b = (b - n.avg[0]) @ n.v
        W = W @ n.v
    a = lin[0].avg[0]
    return W, b + (a.astype(np.float32).astype(np.float64) - a) @ W


def second_affine(node):
    return (node.sf, -node._bias[0]) if isinstance(node, N.SFANode) else (node.v, -(node.avg[0] @ node.v))


def folded(flow, q):
    """[F_c0, F_c1] as 32 x 32 (row = 16 x function + z0 feature, column = z1 feature) of layer-1 node q, float64."""
    layers = [n for n in flow if isinstance(n, N.Layer)]
    boards = [n for n in flow if isinstance(n, N.Switchboard)]
    l0, l1 = layers[0].nodes, layers[1].nodes
    conn = np.asarray(boards[1].connections)
    w0 = l0[0].output_dim
    p0 = first_affine(l0[0])[0].shape[1]
    in_off = sum(n.input_dim for n in l1[:q])
    mine = conn[in_off:in_off + l1[q].input_dim]
    pca = l1[q].flow[0]
    P = pca.output_dim
    out = []
    for sl in range(2):
        ci = 2 * q + sl
        rows = np.nonzero((mine >= ci * w0) & (mine < (ci + 1) * w0))[0]
        assert rows.size == w0
        w2, _ = second_affine(l0[ci].flow[-1])
        want = w2[:, mine[rows] - ci * w0] @ pca.v[rows, :]
        full = np.zeros((32, 32))
        full[0:p0, :P] = want[:p0]
        full[16:16 + p0, :P] = want[p0:]
        out.append(full)
    return out, P


def check_packed(got, flow, nodes):
    l0 = [n for n in flow if isinstance(n, N.Layer)][0].nodes
    for q in nodes:
        fulls, P = folded(flow, q)
        for sl in range(2):
            F = got["F"][(q, sl)]
            want = fulls[sl].copy()
            assert np.all(want[12, :P] != 0) and np.all(want[28, :P] != 0)
            want[[12, 28]] = 0.0      # register 3 of both functions: gone from fold_frag
            assert np.array_equal(F[want == 0], np.zeros_like(F[want == 0])), (q, sl)
            assert within_one_ulp(F, want), (q, sl)
        for mt in range(2):
            last = got["last"][(q, mt)]
            want = np.zeros(64)
            for g in range(4):
                child, func = g % 2, g // 2      # lane group 0: child 0 identity, 1: child 1 identity, 2: child 0 power, 3: child 1 power
                for i in range(16):
                    col = q_of_row(i) if mt == 0 else 16 + (i & 3)
                    want[16 * g + i] = fulls[child][16 * func + 12, col]
            assert within_one_ulp(last, want), (q, mt)
            assert np.array_equal(last == 0, want == 0) and np.count_nonzero(want) == 4 * (16 if mt == 0 else 4 * (P - 16)), (q, mt)
        for ci in (2 * q, 2 * q + 1):
            W, b = first_affine(l0[ci])
            assert W.shape == (16, 13)
            plain, plain_b = np.zeros((16, 16)), np.zeros(16)
            for i in range(16):
                f = q_of_row(i)
                if f < 13:
                    plain_b[i] = b[f]
                    for k in range(16):      # k slot 4 r + g holds input position 4 r + g, or 4 g + r in a transposed plan
                        plain[i, k] = W[(4 * (k & 3) + (k >> 2)) if got["s0_transpose"] else k, f]
            assert within_one_ulp(got["a1_plain"][ci], plain) and within_one_ulp(got["b1_plain"][ci], plain_b), ci
            assert not plain[[7, 11, 15]].any() and plain[3].all()
            want, want_b = plain.copy(), plain_b.copy()
            for row in ((11,) if ci % 2 == 0 else (7, 15)):
                want[row], want_b[row] = plain[3], plain_b[3]
            if ci % 2:
                want[3], want_b[3] = 0.0, 0.0
            assert within_one_ulp(got["a1"][ci], want) and within_one_ulp(got["b1"][ci], want_b), ci
            assert np.array_equal(got["a1"][ci] == 0, want == 0) and np.array_equal(got["b1"][ci] == 0, want_b == 0), ci
            # the repeated rows are the plan's own floats, moved
            src = got["a1_plain"][ci][3]
            for row in ((3, 11) if ci % 2 == 0 else (7, 15)):
                assert np.array_equal(got["a1"][ci][row], src) and got["b1"][ci][row] == got["b1_plain"][ci][3], (ci, row)


@pytest.mark.parametrize("name", cases.PACKED)
def test_packed_arrays_match_numpy_float64(driver, tmp_path, name):
    """Every layer-1 node of the 16 + 8 node nets: fold_last, fold_frag without register 3, the repeated row and bias of layer 0; the
    issued counts (4 x 16x16x4 per layer-0 node, 23 + 23 per layer-1 node in place of 26 + 26: 480 FLOP per row and node fewer) and
    what describe says."""
    flow = cases.HOST_NETS[name]()
    got = run(driver, tmp_path, flow, name=name)
    n1 = 8
    assert got["fold01"] == 1 and got["pack"] == 1 and got["note"].startswith("link 0 -> 1 folded")
    assert got["pack_note"].startswith("one-row k-steps packed") and got["pack_note"] in got["name1"] and got["note"] in got["name1"]
    assert "issues %d x 16x16x4 + %d x 4x4x1" % (23 * n1, 23 * n1) in got["pack_note"]
    assert got["issue"] == {0: (8 * n1, 0), 1: (23 * n1, 23 * n1)}
    assert got["given"] - got["padded_flops"] == (768 + 480) * n1
    assert len(got["last"]) == 2 * n1 and len(got["F"]) == 2 * n1 and len(got["a1"]) == 2 * n1
    check_packed(got, flow, range(n1))
    if name == "two_affine":      # the bias of feature 12 is a real number there
        assert all(got["b1_plain"][ci][3] != 0 for ci in range(2 * n1))
    off = run(driver, tmp_path, flow, opts=("--pack", "0"), name=name)
    assert off["pack"] == 0 and off["pack_note"] == "" and not off["last"] and off["issue"] == {0: (8 * n1, 0), 1: (26 * n1, 26 * n1)}
    assert off["given"] == got["given"] and off["given"] - off["padded_flops"] == 768 * n1


def test_u11l_128(driver, tmp_path):
    """U11L-128's structure with drawn weights: 1024 + 512 nodes, the first, two middle and the last layer-1 node element by element;
    FusedPlan::padded_flops 9 815 040 -> 9 569 280 per sub-image, the figure hg_info reports unchanged."""
    flow = plan_cases.reseed(plan_cases.preset_structure("U11L-128"), 777)
    nodes = (0, 1, 255, 511)
    got = run(driver, tmp_path, flow, opts=("--nodes", ",".join(map(str, nodes))), name="U11L-128")
    off = run(driver, tmp_path, flow, opts=("--pack", "0"), name="U11L-128")
    assert got["fold01"] == 1 and got["pack"] == 1 and off["fold01"] == 1 and off["pack"] == 0
    assert off["padded_flops"] == 9815040 and got["padded_flops"] == 9569280 and got["given"] == off["given"]
    assert off["issue"] == {0: (4096, 0), 1: (26 * 512, 26 * 512)} and got["issue"] == {0: (4096, 0), 1: (23 * 512, 23 * 512)}
    assert sorted(got["last"]) == sorted((q, mt) for q in nodes for mt in range(2))
    check_packed(got, flow, nodes)


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refusals_are_named(driver, tmp_path, name):
    """A layer 0 of 12, 14 or 16 outputs, fold01 off, HIGSFA_NO_REM4: not packed, stage 1's line says why, no packed array exists (the
    driver fails where one does) and the plan issues what it issues without the option."""
    make, opts, env, words = cases.REFUSED[name]
    got = run(driver, tmp_path, make(), opts=opts, env=env, name=name)
    off = run(driver, tmp_path, make(), opts=tuple(opts) + ("--pack", "0"), env=env, name=name)
    assert got["pack"] == 0 and not got["last"] and not got["a1"]
    assert got["pack_note"].startswith("the link's one-row k-steps stay as they are: ") and words in got["pack_note"], got["pack_note"]
    assert got["pack_note"] in got["name1"] and off["pack_note"] == ""
    assert got["fold01"] == (1 if name in ("w14", "w16") else 0)
    assert got["padded_flops"] == off["padded_flops"] and got["issue"] == off["issue"] and got["given"] == off["given"]


def test_switched_off_the_plan_is_the_recorded_one(driver, tmp_path):
    """fold01 on, fold01_pack off: the plan as tests/plan_digest.hpp prints it (every scalar, every array's digest, the stage names) and
    the folded arrays' digests equal what the planner gave before it had the option (tests/golden/fold01_pack_off_digests.json,
    recorded from that commit with this driver built -DPLAN_WITHOUT_PACK).  Weights drawn element by element: no BLAS result in it."""
    with open(cases.GOLDEN) as f:
        golden = json.load(f)
    flows = cases.digest_flows()
    flows["U11L-128"] = plan_cases.reseed(plan_cases.preset_structure("U11L-128"), 777)
    assert sorted(golden) == sorted(flows)
    for name, flow in flows.items():
        got = run(driver, tmp_path, flow, opts=("--pack", "0", "--digest"), name=name)
        assert got["fold01"] == 1 and len(got["digest"]) > 8
        assert hashlib.sha256("\n".join(got["digest"]).encode()).hexdigest() == golden[name], name


def test_driver_under_sanitizers(tmp_path):
    """The driver once more with -fsanitize=address,undefined on a packed net and the refusals: a clean exit."""
    exe = tmp_path / "fold01_pack_plan_driver_san"
    b = cases.build_driver(exe, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    assert run(exe, tmp_path, cases.HOST_NETS["two_affine"](), name="two_affine")["pack"] == 1
    for name, (make, opts, env, _) in cases.REFUSED.items():
        assert run(exe, tmp_path, make(), opts=opts, env=env, name=name)["pack"] == 0
