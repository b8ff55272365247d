"""CPU: the planner's fold of the link 0 -> 1 (Planner::plan_fold01, csrc/hg_fused_plan.cpp) through a stand-alone driver with its
own main (tests/fold01_plan_driver.cpp, linked against the blob parser and the planner alone).  With FusedOptions::fold01 off the
planner is what tests/test_fused_plan_host.py pins; here it is on.  The folded fragments and bias, un-permuted by the driver, against
the same fold done in numpy float64 from the nodes: every element the float32 rounding of the float64 value to within one float32
ulp (the two float64 sums may differ in order).  And the refusals, which hg_flow_describe must name."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import blob
from pyfaceanalysis_amd import nodes as N
from tests import fold01_cases

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fold01") / "fold01_plan_driver"
    b = fold01_cases.build_driver(exe)
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    return exe


def run(driver, tmp_path, flow, env=None, name="net"):
    p = tmp_path / (name + ".bin")
    p.write_bytes(blob.flow_to_blob(flow))
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([str(driver), str(p)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=e)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    lines = text.splitlines()
    assert lines[0] == "== %s.bin" % name and lines[1].startswith("fold01 "), lines[:2]
    head = lines[1].split(" note ")[0].split()
    out = {"fold01": int(head[1]), "fuse01": int(head[3]), "padded_flops": int(head[5]), "given": int(head[7]),
           "note": lines[1].split(" note ", 1)[1], "name0": lines[2][len("name0 "):], "name1": lines[3][len("name1 "):],
           "issue": {int(w[1]): (int(w[2]), int(w[3])) for w in (ln.split() for ln in lines if ln.startswith("issue "))},
           "chunks": next(int(ln.split()[1]) for ln in lines if ln.startswith("chunks ")), "bias": {}, "F": {}}
    for ln in lines:
        w = ln.split()
        if w[0] == "bias":
            out["bias"][int(w[1])] = np.array(w[2:], dtype=np.float32)
        elif w[0] == "F":
            out["F"][(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float32).reshape(32, 32)
    return out


def _affine_parts(node):
    """(W, c) of y = e @ W + c for a trained PCA / SFA node."""
    if isinstance(node, N.SFANode):
        return node.sf, -node._bias[0]
    return node.v, -(node.avg[0] @ node.v)


def within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


@pytest.mark.parametrize("name", sorted(fold01_cases.HOST_NETS))
def test_fold_matches_numpy_float64(driver, tmp_path, name):
    """F_c = A2_c A1_q[rows of c, :] and bias'_q = b1_q + sum_c (b2_c - a_q[rows c]) A1_q[rows c, :] - sum_c a2_c F_c, element by
    element; rows and columns the net does not have are zero; the issue counts are 4 x 16x16x4 per layer-0 node and
    26 x 16x16x4 + 26 x 4x4x1 per layer-1 node, 768 FLOP per row and layer-1 node fewer than the flow as given."""
    flow = fold01_cases.HOST_NETS[name]()
    got = run(driver, tmp_path, flow, name=name)
    assert got["fold01"] == 1 and got["fuse01"] == 1 and got["note"].startswith("link 0 -> 1 folded")
    assert got["note"] in got["name1"]
    layers = [n for n in flow if isinstance(n, N.Layer)]
    boards = [n for n in flow if isinstance(n, N.Switchboard)]
    l0, l1 = layers[0].nodes, layers[1].nodes
    conn = np.asarray(boards[1].connections)
    w0 = l0[0].output_dim
    p0 = l0[0].flow[0].output_dim
    assert len(l0) == 16 and len(l1) == 8 and len(got["bias"]) == 8 and len(got["F"]) == 16
    assert got["chunks"] >= 2
    n1 = len(l1)
    assert got["issue"] == {0: (4 * 2 * n1, 0), 1: (26 * n1, 26 * n1)}
    assert got["given"] - got["padded_flops"] == 768 * n1
    assert "issues %d x 16x16x4 for layer 0 and %d x 16x16x4 + %d x 4x4x1 for this layer" % (8 * n1, 26 * n1, 26 * n1) in got["name1"]
    assert "issued: %d x 16x16x4 + %d x 4x4x1" % (18 * n1, 18 * n1) in got["name1"]      # the stage line itself: the flow as given
    for q, pnode in enumerate(l1):
        in_off = sum(n.input_dim for n in l1[:q])
        mine = conn[in_off:in_off + pnode.input_dim]
        pca = pnode.flow[0]
        P = pca.output_dim
        want_bias = np.zeros(P)
        for sl in range(2):
            ci = 2 * q + sl
            rows = np.nonzero((mine >= ci * w0) & (mine < (ci + 1) * w0))[0]
            assert rows.size == w0
            local = mine[rows] - ci * w0
            w2, c2 = _affine_parts(l0[ci].flow[-1])
            want = w2[:, local] @ pca.v[rows, :]              # [2 p0 x P], float64
            want_bias += (c2[local] - pca.avg[0, rows]) @ pca.v[rows, :]
            F = got["F"][(q, sl)]
            full = np.zeros((32, 32))
            full[0:p0, :P] = want[:p0]
            full[16:16 + p0, :P] = want[p0:]
            assert np.array_equal(F[full == 0], np.zeros_like(F[full == 0]))
            assert within_one_ulp(F, full), (q, sl, float(np.abs(F - full).max()))
        full_b = np.zeros(32)
        full_b[:P] = want_bias
        assert np.array_equal(got["bias"][q][P:], np.zeros(32 - P, dtype=np.float32))
        assert within_one_ulp(got["bias"][q], full_b), (q, float(np.abs(got["bias"][q] - full_b).max()))
    # distinct weights per node: no two nodes' folded matrices agree (a swapped pair of children would pass otherwise)
    mats = [got["F"][k] for k in sorted(got["F"])]
    assert all(not np.array_equal(mats[i], mats[k]) for i in range(len(mats)) for k in range(i))


@pytest.mark.parametrize("name", sorted(fold01_cases.REFUSED))
def test_refusals_are_named(driver, tmp_path, name):
    """Layer-1 affines of 21 outputs, HIGSFA_NO_REM4, a second function that is no |x|^p, an iGSFA layer 1: not folded, stage 1's
    line says why, no folded array exists and the plan issues what the flow as given issues."""
    make, env, words = fold01_cases.REFUSED[name]
    got = run(driver, tmp_path, make(), env=env, name=name)
    assert got["fold01"] == 0 and not got["F"] and not got["bias"]
    assert got["note"].startswith("link 0 -> 1 stays as it is: ") and words in got["note"], got["note"]
    assert got["note"] in got["name1"]
    assert got["given"] == got["padded_flops"]


def test_driver_under_sanitizers(tmp_path):
    """The driver once more with -fsanitize=address,undefined on two folded nets and the refusals: a clean exit."""
    exe = tmp_path / "fold01_plan_driver_san"
    b = fold01_cases.build_driver(exe, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-3000:]
    for name in ("w13_p20_s17", "w16_p17_s20"):
        assert run(exe, tmp_path, fold01_cases.HOST_NETS[name](), name=name)["fold01"] == 1
    for name, (make, env, _) in fold01_cases.REFUSED.items():
        assert run(exe, tmp_path, make(), env=env, name=name)["fold01"] == 0
