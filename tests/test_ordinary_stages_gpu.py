"""GPU: the ordinary stage kind (affine -> expansion -> affine) on the device at every instantiation and launch rule: k_stage at each of
pick_stage's 49 instantiations and each shape of the node-group sweep, k_stage_splitm at every run-time (mt1n, mt2n) with both T and
both REM forms, and the first-layer kernels k_stage0 / k_stage0p (csrc/hg_fused.hip) — held to the float64 oracle node by node and
layer by layer, and a row's bits independent of the batch it travels in.  Nets, batch sizes and what each call must launch:
tests/ordinary_stage_cases.py, whose tables tests/test_ordinary_stages_plan_host.py holds plan_call to on the CPU.

Every handle is planned under HIGSFA_DEBUG, so every launch writes one line ("[sweep stage i] ... shape AxB ... kbf K fs F rem4 R pk P",
"[splitm stage i] ... mt1 a mt2 b rem4 R tiles T waves W", "[front0] persistent P tiles T vec4 V"; csrc/hg_fused_call.cpp: format_step).
The tests read them with capfd and hold them to the tables: a case that falls into another route or shape fails, it does not pass on
another kernel.  Rows go in through the device entry, one call per batch (test_stage_shapes_gpu.device_call, with its NaN guard rows
behind the output).  DESIGN.md §6.13 has the table by instantiation and the measured errors.  Which test holds what:

  (a) per node against the oracle, the lines of the call      test_per_node_against_the_oracle (every net, every size, every layer)
  (b) every instantiation and shape ran, on its own case      test_shapes_reached_family_1 / _2 / _3, test_front_kernels
  (c) a row's bits do not depend on its batch                 test_rows_bit_identical_across_batch_sizes: under SWEEP_ONLY the shape changes
                                                              with the size, under the default switches (":d") the route does, from
                                                              k_stage_splitm to the sweep
  (d) a NaN row stays in its row                              test_nan_stays_in_its_row: the second tile of an 8 x 2 wave, of a T = 2 split-m
                                                              workgroup
  (e) n_cols, float64 output                                  test_output_options
  packed input: three forms, one arithmetic                   test_packed_input_forms_agree"""
import contextlib
import os

import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import _capi
from pyfaceanalysis_amd import nodes as N
from pyfaceanalysis_amd.flow import Flow
from tests import ordinary_stage_cases as cases
from tests.test_hoist_gpu import per_node_errors
from tests.test_stage_shapes_gpu import GUARD, device_call, strided_rows, to_device

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's budget, of the node's max|ref|
DRAW_TOL = 1e-5     # a draw on which the GENERIC plan is above this is badly conditioned: replace it (none had to be: DESIGN.md §6.13)
NETS = cases.nets()
NAMES = tuple(NETS)

_INPUTS = {}        # input width -> (host rows, device rows): one matrix per width, shared by every net of that width, never changed
_RAN = {}           # (net, rows) -> the launches of one full call, as its debug lines name them


def inputs(d):
    if d not in _INPUTS:
        x = cases.inputs(d, 9000 + d)
        _INPUTS[d] = (x, to_device(x))
    return _INPUTS[d]


@contextlib.contextmanager
def switches(env):
    """The planner's switches are read once, when a handle is made."""
    env = dict(env, HIGSFA_DEBUG="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(capfd, flow, xd, n, **kw):
    """One device call and the launches its debug lines name; the lines name every stage of the handle exactly once."""
    capfd.readouterr()
    y = device_call(flow, xd, n, **kw)
    err = capfd.readouterr().err
    n_stages = flow.info(nodenr=kw.get("nodenr")).n_stages - 1      # (the last entry is the pass that writes the caller's rows)
    assert cases.covered_stages(err) == list(range(n_stages)), err[-2000:]
    return y, cases.launches(err)


def check_launches(name, rows, got):
    """The launches that ran are the ones the (net, rows) was sized for: the first-layer kernel, then cases.want line by line (tile
    parts aside: they follow the occupancy the runtime reports)."""
    assert got and got[0]["route"] == "front0", (name, rows, got)
    assert cases.held(got[1:], cases.want(name, rows), parts=False), (name, rows, got[1:], cases.want(name, rows))
    _RAN[(name, rows)] = [dict(g, name=name, rows=rows, tiles=cases.tiles(rows)) for g in got[1:]]
    return _RAN[(name, rows)]


class Case(object):
    """One net under its switches: the fused flow (its handles, prefixes included, planned under HIGSFA_DEBUG and the net's switches),
    optionally the generic flow, and the features of ONE call of the largest batch — computed once, never changed."""

    def __init__(self, name, generic=True):
        _, make, self.env, self.rows = NETS[name]
        self.name = name
        self.nodes = make()
        self.x, self.xd = inputs(self.nodes[0].input_dim)
        self.layers = [k for k, nd in enumerate(self.nodes) if isinstance(nd, N.Layer)]
        self.n_ref = max(self.rows)
        with switches(self.env):
            self.flow = Flow(self.nodes, output_dtype=np.float32)
            self.generic = Flow(self.nodes, output_dtype=np.float32, force_generic=True) if generic else None
            for k in self.layers:
                self.flow.info(nodenr=k)
                if generic:
                    self.generic.info(nodenr=k)
            assert self.flow.info().plan_kind == _capi.HG_PLAN_FUSED and (not generic or self.generic.info().plan_kind == _capi.HG_PLAN_GENERIC)
        self.y = device_call(self.flow, self.xd, self.n_ref)

    def close(self):
        self.flow.close()
        if self.generic is not None:
            self.generic.close()


@pytest.fixture(scope="module")
def _inputs_store(native_lib):
    yield
    _INPUTS.clear()
    _RAN.clear()


@pytest.fixture(scope="module", params=NAMES)
def case(request, _inputs_store):
    """Module-scoped and parametrised: pytest runs the tests of one net together, then the net's flows are closed."""
    c = Case(request.param)
    yield c
    c.close()


def test_per_node_against_the_oracle(case, capfd):
    """(a) Every layer of the net at every batch size, node by node, against the float64 oracle: rows [:rows] through the prefix
    nodes[:k + 1] (nodenr=k) for each k that holds a Layer, on about 30 rows strided over the whole batch with the last row; per node
    max|d| / max|ref| over the node's columns <= 1e-4 (test_hoist_gpu.per_node_errors).  The oracle and the generic plan, the yardstick
    of the draw's conditioning, run once per net on the union of those rows; a draw on which the generic plan is above 1e-5 is to be
    replaced.  The debug lines of the full call must be the ones this (net, rows) was sized for, and name every stage once.
    Measured on MI355X (DESIGN.md §6.13 has the table), worst node of any layer and size: 4.1e-7 .. 9.4e-7 fused against 4.1e-7 .. 9.1e-7
    generic on the nets of one and two functions, 1.8e-6 against 2.1e-6 on those of three and four (nf24, nf33)."""
    c = case
    if c.name.startswith("kb"):      # the split-m line does not carry the K-blocks: the plan listing does
        assert "fused stage 1: %d nodes, K-blocks %d," % (cases.KB_NODES[int(c.name[2:-2])], int(c.name[2:-2])) in c.flow.describe()
    idx = {n: strided_rows(n) for n in c.rows}
    union = np.unique(np.concatenate(list(idx.values())))
    xu = to_device(c.x[union])
    ref, gen = {}, {}
    for k in c.layers:
        ref[k] = oracle.execute_flow(c.nodes[:k + 1], c.x[union])
        gen[k] = device_call(c.generic, xu, len(union), nodenr=k)
    for n in c.rows:
        sel = np.searchsorted(union, idx[n])
        worst = {"fused": (0.0, -1, -1), "generic": (0.0, -1, -1)}
        for k in c.layers:
            y, got = run(capfd, c.flow, c.xd, n, nodenr=k)
            assert y.shape == (n, c.nodes[k].output_dim)
            if k == c.layers[-1]:
                check_launches(c.name, n, got)
                assert np.array_equal(y, c.y[:n])      # the prefix that ends in the last layer is the full net
            for h, yy in (("fused", y[idx[n]]), ("generic", gen[k][sel])):
                errs = per_node_errors(c.nodes[k], yy, ref[k][sel])
                j = int(np.argmax(errs))
                worst[h] = max(worst[h], (errs[j], k, j))
        with capfd.disabled():
            print("%s, %d rows, worst node: %s" % (c.name, n, "; ".join("%s %.3e (flow index %d, node %d)" % ((h,) + worst[h]) for h in ("fused", "generic"))))
        assert worst["generic"][0] <= DRAW_TOL, ("replace this draw", c.name, worst["generic"])
        assert worst["fused"][0] <= TOL, (c.name, n, worst["fused"])


def test_rows_bit_identical_across_batch_sizes(case):
    """(c) A row's features do not depend on the batch it came in: rows [:n] at every size of the net equal those rows of ONE call of the
    largest size, bit for bit, and so does a window from the middle that starts inside a tile.  Under SWEEP_ONLY the launch shape, the
    node group's tile parts and the prefetch form change with the size; under the default switches (":d") the route changes, from
    k_stage_splitm to the node-group sweep — k_stage_splitm adds "the same products in the same order as the k_stage REM
    instantiations", and the README promises the same bits for N = 1 .. 4096."""
    c = case
    bad = []
    for n in c.rows:
        y = device_call(c.flow, c.xd, n)
        if not np.array_equal(y, c.y[:n]):
            d = np.abs(y.astype(np.float64) - c.y[:n])
            bad.append((n, float(d.max() / np.abs(c.y[:n]).max()), int((d > 0).any(axis=0).sum()), y.shape[1]))
    first = c.n_ref // 3 + 5
    for n in sorted({min(c.n_ref // 3, m) for m in c.rows}):
        y = device_call(c.flow, c.xd, n, first=first)
        if not np.array_equal(y, c.y[first:first + n]):
            bad.append(("window of %d at %d" % (n, first), float(np.abs(y.astype(np.float64) - c.y[first:first + n]).max() / np.abs(c.y).max())))
    print("%s: %s" % (c.name, "rows keep their bits at %s" % (c.rows,) if not bad else "rows change bits: %s" % bad))
    assert not bad, (c.name, bad)


def t2_sizes(name):
    """The largest batch size of the net at which a stage under test runs the sweep at 8 x 2, and the largest at which it runs
    k_stage_splitm at T = 2 (either may be missing)."""
    out = set()
    for kind in ("sweep", "splitm"):
        for n in sorted(NETS[name][3], reverse=True):
            if any(w["route"] == kind and (w.get("T") == 2 or w.get("shape", (0, 0))[1] == 2) for w in cases.want(name, n)):
                out.add(n)
                break
    return sorted(out)


NO_T2 = ("nf33:d",)      # a 64-node layer that never leaves the sweep: 4 x 1 at most at its sizes


def test_nan_stays_in_its_row(case, capfd):
    """(d) One NaN pixel in a row of an ODD tile — the second tile of its wave in an 8 x 2 sweep (a wave takes tiles 2 j and 2 j + 1)
    and of its workgroup in k_stage_splitm at T = 2 — at the largest size at which the net runs 8 x 2 and the largest at which it runs
    k_stage_splitm at T = 2: every other row is bit-identical to the clean run, the row comes back non-finite; nothing is written
    behind the batch (device_call's guard rows)."""
    c = case
    sizes = t2_sizes(c.name)
    assert (not sizes) == (c.name in NO_T2), c.name
    for n in sizes or [c.n_ref]:
        tile = (cases.tiles(n) // 2) | 1
        row = min(16 * tile + 5, n - 1)
        assert row // 16 == tile or not sizes
        bad = c.x[:n].copy()
        bad[row, c.nodes[0].input_dim // 2 + 3] = np.nan
        y, got = run(capfd, c.flow, to_device(bad), n)
        check_launches(c.name, n, got)
        keep = np.ones(n, dtype=bool)
        keep[row] = False
        assert np.array_equal(y[keep], c.y[:n][keep]), n
        assert not np.isfinite(y[row]).all(), n


def test_output_options(case):
    """(e) n_cols below the layer's width gives the first columns of the full call, bit for bit (1, 5, 17 and one short of the width);
    float64 output is the float32 output widened."""
    import torch
    c = case
    n = sorted(c.rows)[len(c.rows) // 2]
    width = c.y.shape[1]
    for k in sorted({1, 5, 17, width - 1}):
        assert 0 < k < width
        assert np.array_equal(device_call(c.flow, c.xd, n, n_cols=k), c.y[:n, :k]), k
    dev = c.xd.device
    y = torch.full((n + GUARD, width), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    c.flow.execute_device(c.xd.data_ptr(), np.float32, n, c.xd.shape[1], y.data_ptr(), np.float64, width, width, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    c.flow.check_errors()
    out = y.cpu().numpy()
    assert np.isnan(out[n:]).all() and np.array_equal(out[:n], c.y[:n].astype(np.float64))


def ran(family, capfd):
    """The launches of one full call per (net, rows) of a family, each held to its design by check_launches: what
    test_per_node_against_the_oracle recorded, or — when that test did not run — calls of handles made here."""
    out = []
    for name, (fam, _, _, rows) in NETS.items():
        if fam != family:
            continue
        if any((name, n) not in _RAN for n in rows):
            c = Case(name, generic=False)
            try:
                for n in rows:
                    check_launches(name, n, run(capfd, c.flow, c.xd, n)[1])
            finally:
                c.close()
        for n in rows:
            out += _RAN[(name, n)]
    return out


def test_shapes_reached_family_1(_inputs_store, capfd):
    """(b) k_stage<MT1, MT2, T>, all 16 pairs: each pair ran 1 x 1, 2 x 1, 4 x 1, 8 x 1 and 8 x 2 and nothing else (4 x 2 is never chosen:
    T = 2 is reached only as 8 x 2), 8 x 2 on an odd tile count; the plain instantiation at T = 1 and T = 2 except where pick_stage
    has a better one — (2, 2) and (3, 3) at T = 2 take the whole-visit prefetch of four K-blocks (kbf 4; (3, 3) with the expansion at
    compile time), (4, 4) the compile-time expansion at both T — and ord_general runs the run-time expansion beside them: <3, 3, 2, kbf
    4> and the plain <4, 4, T>.  Node groups of 10, 8, 6, 5, 4, 3, 2, 1 nodes, a short last group, tile_groups > parts > 1."""
    got = ran(1, capfd)
    inst = {cases.instantiation(r) for r in got}
    for pr in cases.PAIRS:
        mine = [r for r in got if r["name"] == "ord%d%d" % pr]
        assert {r["shape"] for r in mine} == {(8, 2), (8, 1), (4, 1), (2, 1), (1, 1)}, pr
        assert any(r["shape"] == (8, 2) and r["tiles"] % 2 for r in mine), pr
    plain = {("k_stage", a, b, t, False, 0, False, -1) for a, b in cases.PAIRS for t in (1, 2)}
    special = {("k_stage", 2, 2, 2, False, 4, False, -1), ("k_stage", 3, 3, 2, False, 4, True, -1), ("k_stage", 4, 4, 1, False, 0, True, -1),
               ("k_stage", 4, 4, 2, False, 0, True, -1), ("k_stage", 3, 3, 2, False, 4, False, -1)}
    assert inst == (plain - {("k_stage", 2, 2, 2, False, 0, False, -1), ("k_stage", 3, 3, 2, False, 0, False, -1)}) | special
    assert {r["shape"] for r in got} == {(8, 2), (8, 1), (4, 1), (2, 1), (1, 1)}
    assert {r["npg"] for r in got} == {10, 8, 6, 5, 4, 3, 2, 1}
    assert any(r["nodes"] % r["npg"] and r["tile_groups"] > r["parts"] > 1 for r in got)
    assert any(r["shape"] == (8, 2) and r["tile_groups"] > r["parts"] > 1 for r in got)      # (which launches: by the occupancy; (1, 1) at one per CU)


def test_shapes_reached_family_2(_inputs_store, capfd):
    """(b) The remainder-tile, prefetch and packed-input forms, each on the case sized for it: <2, 2, T, REM> and <3, 3, T, REM> at T = 1
    and (remC*, two K-blocks) T = 2; kbf 4 REM (remA*) and kbf 3 REM (remB*) at 8 x 2, the latter with the expansion at compile time
    for (3, 3); under HIGSFA_NO_REM4 the same nets on the non-REM forms — kbf 4, and for three K-blocks the plain <2, 2, 2> and <3, 3, 2>,
    which no net of family 1 reaches; pk 1 kbf 3 at (2, 2) and at (3, 3) with both expansions, against the same nets under
    HIGSFA_NO_SOA (kbf 3, lane-major packed block) and HIGSFA_NO_PACK (four K-blocks: kbf 4)."""
    got = ran(2, capfd)
    inst = {cases.instantiation(r) for r in got}
    rem = {("k_stage", m, m, t, True, 0, False, -1) for m in (2, 3) for t in (1, 2)}
    kbf = {("k_stage", m, m, 2, True, k, False, -1) for m in (2, 3) for k in (3, 4)} | {("k_stage", 3, 3, 2, True, 3, True, -1)}
    off = {("k_stage", m, m, t, False, 0, False, -1) for m in (2, 3) for t in (1, 2)} | {("k_stage", m, m, 2, False, 4, False, -1) for m in (2, 3)} | \
          {("k_stage", 3, 3, 2, False, 4, True, -1)}
    pk = {("k_stage", 3, 3, 2, True, 3, True, 1), ("k_stage", 3, 3, 2, True, 3, False, 1), ("k_stage", 2, 2, 2, True, 3, False, 1)}
    assert inst == rem | kbf | off | pk
    for name, m, t0, k in (("remA2", 2, 163, 4), ("remA3", 3, 51, 4), ("remB2", 2, 109, 3), ("remB3", 3, 51, 3)):
        for tag in ("", "+gen"):
            mine = [r for r in got if r["name"] == name + tag]
            assert all(r["rem4"] == 1 for r in mine) and min(r["tiles"] for r in mine if r["shape"] == (8, 2)) == t0
            assert {r["kbf"] for r in mine if r["shape"][1] == 2} == {k} and {r["shape"] for r in mine} == {(8, 2), (8, 1), (4, 1), (2, 1), (1, 1)}
            assert all(r["rem4"] == 0 for r in got if r["name"] == name + tag + "+norem4")
    for m in (2, 3):
        for tag in ("", "+gen"):
            top = {sw: [r for r in got if r["name"] == "pk%d%s%s" % (m, tag, sw) and r["stage"] == 2 and r["tiles"] == 163] for sw in ("", "+nosoa", "+nopack")}
            assert [(r["pk"], r["kbf"], r["kb1"], r["shape"]) for r in top[""]] == [(1, 3, 3, (8, 2))]
            assert [(r["pk"], r["kbf"], r["kb1"], r["shape"]) for r in top["+nosoa"]] == [(-1, 3, 3, (8, 2))]
            assert [(r["pk"], r["kbf"], r["kb1"], r["shape"]) for r in top["+nopack"]] == [(-1, 4, 4, (8, 2))]
    assert any(r["shape"] == (8, 2) and r["tiles"] % 2 and r["pk"] == 1 for r in got)


def test_shapes_reached_family_3(_inputs_store, capfd):
    """(b) k_stage_splitm<T, REM>: T = 1 and T = 2 at all 16 run-time (mt1n, mt2n) without remainder tiles, waves = max(mt1n, mt2n), T = 2
    on three tiles (an absent second tile); the REM form at (2, 2) and (3, 3), T = 1 and T = 2; 8, 9, 16 and 17 K-blocks (one batch of
    eight, a second of one, two, a third of one) at T = 1 and T = 2; mt1 x nf = 8 with four functions; a linear layer; and the line to
    the sweep from either side — mt1 x nf = 9 on the sweep even at one tile."""
    got = ran(3, capfd)
    sp = [r for r in got if r["route"] == "splitm"]
    assert {(r["T"], r["mt"]) for r in sp if not r["rem4"] and r["name"].startswith("ord")} == {(t, pr) for t in (1, 2) for pr in cases.PAIRS}
    assert all(r["waves"] == max(r["mt"]) for r in sp if r["name"] != "linear:d")
    for pr in cases.PAIRS:
        assert any(r["name"] == "ord%d%d:d" % pr and r["T"] == 2 and r["tiles"] == 3 for r in sp), pr
        assert any(r["name"] == "ord%d%d:d" % pr and r["route"] == "sweep" and r["shape"] == (8, 2) for r in got), pr
    assert {(r["T"], r["mt"]) for r in sp if r["rem4"]} == {(t, (m, m)) for t in (1, 2) for m in (2, 3)}
    assert any(r["rem4"] and r["T"] == 2 and r["tiles"] == 3 for r in sp)
    for kb in cases.KB_NODES:
        assert {r["T"] for r in sp if r["name"] == "kb%d:d" % kb} == {1, 2}, kb
    assert {r["T"] for r in sp if r["name"] == "nf24:d"} == {1, 2} and {r["T"] for r in sp if r["name"] == "linear:d"} == {1, 2}
    assert {(r["route"], r["waves"]) for r in sp if r["name"] == "linear:d"} == {("splitm", 2)}
    assert {r["route"] for r in got if r["name"] == "nf33:d"} == {"sweep"} and any(r["name"] == "nf33:d" and r["tiles"] == 1 for r in got)
    for name in ("twin11:d", "twin23:d", "twin32:d", "twin44:d"):
        assert [(r["route"], r.get("T")) for r in got if r["name"] == name] == [("splitm", 1)] * 3 + [("splitm", 2), ("sweep", None)], name


@pytest.mark.parametrize("mt", (2, 3))
def test_packed_input_forms_agree(_inputs_store, mt):
    """The third layer of pk_net reads its children's remainder rows from one packed block: slot-major (pk 1), lane-major
    (HIGSFA_NO_SOA) or, with packing off (HIGSFA_NO_PACK), as a K-block per child.  Slot-major against lane-major: plan_slot_major
    promises "the same products in the same order", so the bits are the same at every size.  Unpacked against packed: the remainder
    rows of a child are then a K-block of their own behind the child's full tile — the second child's are added AFTER its full
    tile, in the packed forms before it — so only the oracle binds the two (test_per_node_against_the_oracle holds all three to it); what they do is printed."""
    for tag in ("", "+gen"):
        ys = {}
        for sw in ("", "+nosoa", "+nopack"):
            c = Case("pk%d%s%s" % (mt, tag, sw), generic=False)
            ys[sw] = {n: device_call(c.flow, c.xd, n) for n in (1, 70, 2600)}
            c.close()
        for n in (1, 70, 2600):
            assert np.array_equal(ys[""][n], ys["+nosoa"][n]), (mt, tag, n)
            d = np.abs(ys[""][n].astype(np.float64) - ys["+nopack"][n]).max() / np.abs(ys[""][n]).max()
            print("pk%d%s, %d rows: packed against unpacked input max|d| / max|y| = %.3e" % (mt, tag, n, d))
            assert d <= TOL


@pytest.mark.parametrize("pair", cases.PAIRS, ids=lambda p: "%dx%d" % p)
def test_front_kernels(native_lib, capfd, pair):
    """Family 4, k_stage0<MT1, MT2, T, XT> / k_stage0p: a one-layer net of 16 nodes at 3, 4 and 5 tiles and 70 rows (a ragged last tile), rows of
    integer-valued pixels as uint8, float32 and float64.  The line must say T = 1 below four tiles, T = 4 from four where mt1 x mt2 <= 4
    and T = 1 above, persistent (k_stage0p) at (1, 1) alone; every call against the float64 oracle per node (all rows) within 1e-4, the
    three input types the same bits, rows [:n] the bits of the largest call; and rows whose stride forbids 16-byte loads (257 elements:
    "vec4 0") the bits of the same rows contiguous.
    Measured on MI355X: worst node 3.3e-7 .. 6.7e-7 fused, 3.4e-7 .. 7.5e-7 generic over the 16 pairs."""
    import torch
    nodes = cases.front_net(*pair)
    n_ref = max(cases.FRONT_ROWS)
    x8 = np.random.default_rng(9300 + 16 * pair[0] + pair[1]).integers(0, 256, size=(n_ref, 256), dtype=np.uint8)
    ref = oracle.execute_flow(nodes, x8.astype(np.float64))
    with switches({}):
        flow = Flow(nodes, output_dtype=np.float32)
        generic = Flow(nodes, output_dtype=np.float32, force_generic=True)
        assert flow.info().plan_kind == _capi.HG_PLAN_FUSED and generic.info().plan_kind == _capi.HG_PLAN_GENERIC
    try:
        yg = device_call(generic, to_device(x8.astype(np.float32)), n_ref)
        eg = max(per_node_errors(nodes[1], yg, ref))
        y_ref = None
        seen = set()
        for dt in cases.FRONT_DTYPES:
            xd = to_device(x8.astype(dt))
            for n in sorted(cases.FRONT_ROWS, reverse=True):
                y, got = run(capfd, flow, xd, n)
                assert got == [cases.front_want(pair, n)], (pair, dt, n, got)
                seen.add((got[0]["T"], got[0]["persistent"]))
                if y_ref is None:
                    y_ref = y
                assert np.array_equal(y, y_ref[:n]), (dt, n)
            # a row stride of 257 elements: no 16-byte loads
            wide = torch.zeros((n_ref, 257), dtype=xd.dtype, device=xd.device)
            wide[:, :256] = xd
            for n in (64, 70):
                capfd.readouterr()
                out = torch.full((n + GUARD, y_ref.shape[1]), float("nan"), dtype=torch.float32, device=xd.device)
                torch.cuda.synchronize(xd.device)
                flow.execute_device(wide.data_ptr(), np.dtype(dt), n, 257, out.data_ptr(), np.float32, y_ref.shape[1], y_ref.shape[1],
                                    stream=torch.cuda.current_stream(xd.device).cuda_stream)
                torch.cuda.synchronize(xd.device)
                flow.check_errors()
                got = cases.launches(capfd.readouterr().err)
                assert got == [cases.front_want(pair, n, vec4=False)], (pair, dt, n, got)
                o = out.cpu().numpy()
                assert np.isnan(o[n:]).all() and np.array_equal(o[:n], y_ref[:n]), (dt, n)
        assert seen == ({(1, 0), (4, int(pair == (1, 1)))} if pair in cases.FRONT_T4 else {(1, 0)})
        ef = max(per_node_errors(nodes[1], y_ref, ref))
        with capfd.disabled():
            print("front%d%d: worst node fused %.3e, generic %.3e" % (pair + (ef, eg)))
        assert eg <= DRAW_TOL, ("replace this draw", pair, eg)
        assert ef <= TOL
    finally:
        flow.close()
        generic.close()
