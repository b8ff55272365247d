"""GPU: summed links — between two hoisted layers that both run the node-group sweep, the lower one stores
(bias + child 0's tiles) + child 1's tiles once per node of the upper one (k_stage_sum_pair) and the upper one reads that as a hoisted
layer of one child per node whose first bias is -0.0f.  The features are the bits of the plan that stores every child's tiles
(HIGSFA_NO_PAIR=1), and every layer stays within the project's budget of the float64 oracle, node by node.

The net is tests/pair_cases.three_pair_net: fused stages 2, 3 and 4 are 60 -> 60 layers of 12, 6 and 3 nodes with two children each, the
upper two behind permuting switchboards.  Every handle is planned under SWEEP_ONLY, so that a net this small reaches the node-group
sweep at all, with HIGSFA_SUM_LDS=128 (a pair group holds two pairs: stage 3's three pairs make a group of two and a group of one) and
HIGSFA_PAIR_WGS=1 (the executor's threshold on pair groups x tile groups, which nothing this small would reach).  The links 2 -> 3 and
3 -> 4 are then stored summed: stage 2 runs the pair kernel on layer 1's two partial tile sets per node, stage 3 runs it on a summed
input and stage 4 reads a summed input with k_stage_sum.  The link 1 -> 2 stays as it is (its producer multiplies)."""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import nodes as N
from pyfaceanalysis_amd.flow import Flow
from tests import pair_cases

pytestmark = pytest.mark.gpu
TOL = 1e-4                                                    # the project's budget, of max|ref|
SWEEP_ONLY = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0"}
PAIRED = dict(SWEEP_ONLY, HIGSFA_SUM_LDS="128", HIGSFA_PAIR_WGS="1")
PLAIN = dict(PAIRED, HIGSFA_NO_PAIR="1")
# a single tile (one wave), a full tile, two and three tiles (fewer waves than eight, an odd tile count), nine and seventeen tiles on
# eight waves (a last tile group short).  At these sizes every tile group has a workgroup of its own, so one more size, 8336 rows
# (521 tiles, 66 tile groups), has more tile groups than a launch of these node groups is split into: workgroups walk on to a second
# tile group and prefetch across the step
ROWS = (1, 16, 17, 33, 130, 257)
N_BIG = 8336


def load(monkeypatch, nodes, env, prefixes=()):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    flow = Flow(nodes, output_dtype=np.float32)
    flow.info()
    for k in prefixes:
        flow.info(nodenr=k)
    for k in env:
        monkeypatch.delenv(k)
    return flow


class Case(object):
    """The net, its rows, and the two handles with the prefixes of every layer — made once."""

    def __init__(self, monkeypatch):
        self.nodes = pair_cases.three_pair_net()
        self.ks = [k for k, nd in enumerate(self.nodes) if isinstance(nd, N.Layer)]
        self.x = np.random.default_rng(950).normal(size=(N_BIG, self.nodes[0].input_dim)).astype(np.float32)
        self.paired = load(monkeypatch, self.nodes, PAIRED, self.ks)
        self.plain = load(monkeypatch, self.nodes, PLAIN, self.ks)
        self.y = self.plain.execute(self.x)


@pytest.fixture(scope="module")
def case(native_lib):
    mp = pytest.MonkeyPatch()
    c = Case(mp)
    yield c
    c.paired.close()
    c.plain.close()
    mp.undo()


def test_described_and_launched(case, monkeypatch, capfd):
    """describe() says which hoisted layers are paired, and HIGSFA_NO_PAIR=1 says so too; a handle planned with HIGSFA_DEBUG reports
    the pair launches of stages 2 and 3 (and none under HIGSFA_NO_PAIR=1): the comparisons below do compare two different paths."""
    d1 = [ln for ln in case.paired.describe().splitlines() if "first affine folded" in ln]
    d0 = [ln for ln in case.plain.describe().splitlines() if "first affine folded" in ln]
    assert len(d1) == len(d0) == 3
    assert all("; paired: " in ln for ln in d1) and all("unpaired: switched off (HIGSFA_NO_PAIR)" in ln for ln in d0)
    for env, want in ((PAIRED, True), (PLAIN, False)):
        flow = load(monkeypatch, case.nodes, dict(env, HIGSFA_DEBUG="1"))
        capfd.readouterr()
        y = flow.execute(case.x[:130])
        err = capfd.readouterr().err
        flow.close()
        assert np.array_equal(y, case.y[:130])
        assert ("[pair stage 2]" in err and "[pair stage 3]" in err) == want and ("[pair stage" in err) == want, err[-2000:]
        assert "[pair stage 4]" not in err and "[pair stage 1]" not in err


@pytest.mark.parametrize("n", ROWS + (N_BIG,))
def test_rows_have_the_unpaired_bits(case, n):
    """The paired handle against HIGSFA_NO_PAIR=1, and both against ONE call of all rows: np.array_equal."""
    y1, y0 = case.paired.execute(case.x[:n]), case.plain.execute(case.x[:n])
    assert np.array_equal(y0, case.y[:n])
    assert np.array_equal(y1, y0)
    if n >= 130:
        assert np.array_equal(case.paired.execute(case.x[64:64 + 33]), case.y[64:97])


def test_every_layer_per_node_against_the_oracle(case):
    """Every Layer through execute(x, nodenr=k), node by node, against the float64 oracle at the project's budget — the second opinion
    that shares no code with the pair kernel (a prefix's last layer stores its own output; the links below it are summed as in the
    full net) — and the same bits from both handles, layer by layer."""
    rows = np.arange(0, 130, 4)
    x = case.x[:130]
    worst = (0.0, -1, -1)
    for k in case.ks:
        ref = oracle.execute_flow(case.nodes[:k + 1], x[rows])
        y1, y0 = case.paired.execute(x, nodenr=k), case.plain.execute(x, nodenr=k)
        assert np.array_equal(y1, y0), k
        d, c0 = np.abs(y1[rows].astype(np.float64) - ref), 0
        for j, nd in enumerate(case.nodes[k].nodes):
            c1 = c0 + nd.output_dim
            worst = max(worst, (float(d[:, c0:c1].max() / np.abs(ref[:, c0:c1]).max()), k, j))
            c0 = c1
        assert c0 == ref.shape[1]
    print("three-pair net, worst node: %.3e of its max|ref| (flow index %d, node %d)" % worst)
    assert worst[0] <= TOL, worst


def test_two_lanes_give_the_serial_bits(case, monkeypatch):
    """Two steps in flight on the two lanes of one paired handle, different rows on each: the serial bits."""
    import torch
    dev = torch.device("cuda", 0)
    k = case.y.shape[1]
    from pyfaceanalysis_amd.sharded import _side_stream
    _side_stream(torch, dev)      # (the process's shared side stream first, as in tests/test_hoist_gpu.py)
    flow = load(monkeypatch, case.nodes, PAIRED)
    assert flow.set_lanes(2) and flow.lanes() == 2
    xs = [torch.from_numpy(case.x[:257]).to(dev), torch.from_numpy(case.x[257:257 + 130]).to(dev)]
    ys = [torch.zeros((x.shape[0], k), dtype=torch.float32, device=dev) for x in xs]
    torch.cuda.synchronize(dev)
    for rnd in range(2):
        for lane in (0, 1):
            x, y = xs[lane], ys[lane]
            flow.step_lane_device(lane, x.data_ptr(), np.float32, x.shape[0], x.shape[1], y.data_ptr(), np.float32, k, k)
        for lane in (0, 1):
            flow.lane_join(lane)
        torch.cuda.synchronize(dev)
        assert np.array_equal(ys[0].cpu().numpy(), case.y[:257]) and np.array_equal(ys[1].cpu().numpy(), case.y[257:387]), rnd
    flow.check_errors()
    flow.close()
