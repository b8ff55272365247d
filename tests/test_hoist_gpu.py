"""GPU: hoisted links — layers whose first affine the planner folded into the second affine of the layer
below, so that they start from the sum of their children's tiles.  Every kernel family that can run such a layer (k_stage_sum,
k_stage_splitm, the layer routine of k_tail and k_subtree) must give a row the same bits, the float64 oracle stays within the
project's budget, and HIGSFA_NO_HOIST=1 restores the unhoisted plan."""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import synth
from pyfaceanalysis_amd.flow import Flow
from tests import helpers, hoist_cases

pytestmark = pytest.mark.gpu
TOL = 1e-4                                                    # the project's budget, of max|ref|
SIZES = (1, 16, 17, 100, 130, 512, 728, 1100, 1738)          # k_subtree sets, k_stage_splitm, k_stage(_sum), every k_tail depth
N_REF = 1738
# every layer on the node-group sweep (k_stage / k_stage_sum): no k_stage_splitm, no top-of-hierarchy launch, no sub-trees
SWEEP_ONLY = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0"}


def rel_err(y, ref):
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max() / np.abs(ref).max())


def load(monkeypatch, nodes, env=None):
    """A flow whose handle was planned under the switches `env` (they are read once, when the handle is made)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    flow = Flow(nodes, output_dtype=np.float32)
    flow.info()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return flow


class Case(object):
    """One net: its input rows, the float64 oracle on a few of them, and the default handle's features of all N_REF rows —
    computed once, never changed."""

    def __init__(self, nodes, seed):
        self.nodes = nodes
        d = nodes[0].input_dim
        self.x = np.random.default_rng(seed).normal(size=(N_REF, d)).astype(np.float32)
        self.idx = np.arange(0, N_REF, 61)
        self.ref = oracle.execute_flow(nodes, self.x[self.idx])
        self.flow = Flow(nodes, output_dtype=np.float32)
        self.y = self.flow.execute(self.x)


_CASES = {}


@pytest.fixture(scope="module")
def case(native_lib):
    def get(name):
        if name not in _CASES:
            nodes = {"chain": hoist_cases.chain_net, "quad": hoist_cases.quad_net,
                     "fuzz": lambda: helpers.subtree_fuzz_net(hoist_cases.FUZZ_SEED)}[name]()
            _CASES[name] = Case(nodes, 900 + len(_CASES))
        return _CASES[name]
    yield get
    for c in _CASES.values():
        c.flow.close()
    _CASES.clear()


NETS = ("chain", "quad", "fuzz")


@pytest.mark.parametrize("name", NETS)
def test_hoisted_plan_within_budget_and_described(case, monkeypatch, name):
    """(b), (c): the hoisted plan and the HIGSFA_NO_HOIST=1 plan both meet 1e-4 of max|ref| against the float64 oracle; describe()
    names the hoisted layers in one and not in the other."""
    c = case(name)
    plain = load(monkeypatch, c.nodes, {"HIGSFA_NO_HOIST": "1"})
    y0 = plain.execute(c.x[c.idx])
    e1, e0 = rel_err(c.y[c.idx], c.ref), rel_err(y0, c.ref)
    print("%s: hoisted %.3e, HIGSFA_NO_HOIST=1 %.3e of max|ref|; hoisted against unhoisted %.3e" % (name, e1, e0, rel_err(c.y[c.idx], y0.astype(np.float64))))
    assert e1 <= TOL and e0 <= TOL
    d1, d0 = c.flow.describe(), plain.describe()
    assert "first affine folded" in d1 and "first affine folded" not in d0
    hoisted = [ln for ln in d1.splitlines() if "first affine folded" in ln]
    want = {"chain": 5, "quad": 3}.get(name)
    assert want is None or len(hoisted) == want
    assert len(d1.splitlines()) == len(d0.splitlines())
    # hg_info counts the flow as given, algorithmic and issued on the unhoisted tiling; what the hoisted plan issues is in describe()
    assert c.flow.info().padded_flops_per_row == plain.info().padded_flops_per_row
    assert c.flow.info().flops_per_row == plain.info().flops_per_row
    issued = lambda d: sum(int(ln.split("issued: ")[1].split(" x 16x16x4")[0]) for ln in d.splitlines() if "issued: " in ln)
    assert issued(d1) < issued(d0)
    plain.close()


@pytest.mark.parametrize("name", NETS)
def test_rows_bit_identical_across_batch_sizes(case, name):
    """(a): a row's features do not depend on the batch it came in: sizes that take the sub-tree launches of both sets, k_stage_splitm,
    the node-group sweep and the top-of-hierarchy launch at one, two and three layers, against ONE call of 1738 rows."""
    c = case(name)
    for n in SIZES:
        assert np.array_equal(c.flow.execute(c.x[:n]), c.y[:n]), n
    assert np.array_equal(c.flow.execute(c.x[300:300 + 130]), c.y[300:430])


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("env", [{"HIGSFA_TAIL": "0"}, {"HIGSFA_TAIL": "1"}, {"HIGSFA_TAIL": "2"}, {"HIGSFA_TAIL": "3"}, SWEEP_ONLY,
                                 {"HIGSFA_SUBTREE": "0"}, {"HIGSFA_NO_FSPEC": "1"}], ids=lambda e: "+".join("%s=%s" % kv for kv in e.items()))
def test_rows_bit_identical_across_kernel_families(case, monkeypatch, name, env):
    """(a): the same bits whichever kernel runs a hoisted layer — every depth of the top-of-hierarchy launch, no sub-trees, and
    every layer above the front kernel on the node-group sweep (k_stage_sum with parents of 2, 3 and 4 tiles and of 2, 3 and 4
    children, with and without the compile-time expansion)."""
    c = case(name)
    flow = load(monkeypatch, c.nodes, env)
    for n in (17, 130, 728, N_REF):
        assert np.array_equal(flow.execute(c.x[:n]), c.y[:n]), n
    flow.close()


def test_two_lanes_give_the_serial_bits(case):
    """(e): two steps in flight on the two lanes of one handle, different rows on each."""
    import torch
    c = case("chain")
    dev = torch.device("cuda", 0)
    k = c.y.shape[1]
    # the process's shared side stream first, as ShardedFlow makes it: which hardware queue a stream lands on depends on how many were
    # created before it (sharded._side_stream), and lane streams made ahead of it move the gather of every later test
    from pyfaceanalysis_amd.sharded import _side_stream
    _side_stream(torch, dev)
    flow = Flow(c.nodes, output_dtype=np.float32)
    assert flow.set_lanes(2) and flow.lanes() == 2
    xs = [torch.from_numpy(c.x[:728]).to(dev), torch.from_numpy(c.x[728:728 + 130]).to(dev)]
    ys = [torch.zeros((x.shape[0], k), dtype=torch.float32, device=dev) for x in xs]
    torch.cuda.synchronize(dev)
    for rnd in range(2):
        for lane in (0, 1):
            x, y = xs[lane], ys[lane]
            flow.step_lane_device(lane, x.data_ptr(), np.float32, x.shape[0], x.shape[1], y.data_ptr(), np.float32, k, k)
        for lane in (0, 1):
            flow.lane_join(lane)
        torch.cuda.synchronize(dev)
        assert np.array_equal(ys[0].cpu().numpy(), c.y[:728]) and np.array_equal(ys[1].cpu().numpy(), c.y[728:858]), rnd
    flow.check_errors()
    flow.close()


def test_u11l_128_error_against_the_oracle(native_lib, nets, monkeypatch):
    """(d): trained U11L-128, 64 rows: the hoisted plan stays within DESIGN.md §3.4's "<= 3e-6 everywhere" of max|ref|.
    Measured on MI355X: hoisted 1.33e-6 (first 20 columns 1.06e-6), unhoisted 1.49e-6 (1.26e-6); the two plans differ
    by 1.31e-6 of max|y|."""
    nodes = nets("U11L-128")
    x = synth.make_subimages(64, 128, dtype=np.float32)
    ref = oracle.execute_flow(nodes, x)
    hoisted = load(monkeypatch, nodes)
    plain = load(monkeypatch, nodes, {"HIGSFA_NO_HOIST": "1"})
    y1, y0 = hoisted.execute(x), plain.execute(x)
    e1, e0 = rel_err(y1, ref), rel_err(y0, ref)
    e1_20, e0_20 = rel_err(y1[:, :20], ref[:, :20]), rel_err(y0[:, :20], ref[:, :20])
    print("U11L-128, 64 rows, max|d|/max|ref|: hoisted %.3e (first 20 columns %.3e), unhoisted %.3e (%.3e); hoisted against unhoisted %.3e"
          % (e1, e1_20, e0, e0_20, rel_err(y1, y0.astype(np.float64))))
    assert sum("first affine folded" in ln for ln in hoisted.describe().splitlines()) == 7
    assert e1 <= 3e-6
    hoisted.close()
    plain.close()
