"""GPU: hoisted links — layers whose first affine the planner folded into the second affine of the layer
below, so that they start from the sum of their children's tiles.  Every kernel family that can run such a layer (k_stage_sum,
k_stage_splitm, the layer routine of k_tail and k_subtree) must give a row the same bits, the float64 oracle stays within the
project's budget, and HIGSFA_NO_HOIST=1 restores the unhoisted plan.

Besides three regular nets (chain, quad, one sub-tree fuzz seed: every parent of a layer alike, children read in ascending order) the
nets of tests/hoist_cases.py that are not: ragged, ragged_wide, small and the twelve seeds of hoist_fuzz_net, whose premises
tests/test_hoist_plan_host.py pins on the CPU.  Which test puts which irregular case on the device:

  parents of one z-tile (k_stage_sum<1, ...>)       ragged stages 2 and 4 under SWEEP_ONLY: test_rows_bit_identical_across_kernel_families,
                                                    test_every_layer_per_node_against_the_oracle, test_ragged_node_groups
  parents of one layer with 1, 3, 4 and 8           ragged, ragged_wide (K-block table padded to eight children; one child: k_stage_sum
  children; n_kids of 1, 3 and 5..8                 leaves its child loop at once; eight: all of k_stage_splitm's KB blocks):
                                                    the three tests over NETS, test_every_layer_per_node_against_the_oracle,
                                                    test_two_lanes_give_the_serial_bits_ragged; 2, 5, 6, 7 children:
                                                    test_fuzz_rows_bit_identical_across_kernel_families
  parents of one layer with different widths and    ragged_wide stage 2 (1, 2, 3 and 3 of three tiles; the children of the narrow
  tile counts                                       parents store zero tiles): the tests over NETS, the per-node test; fuzz seeds
  a permuting switchboard in front of hoisted       small, ragged, ragged_wide, every fuzz seed (children first read in an order
  parents                                           that is not ascending): the per-node test is the one that tells a wrong ORDER
                                                    or an added padding entry from a right one — all families could share either
                                                    (an order that only rounds otherwise: test_children_are_added_in_first_read_order,
                                                    a net on which the order decides the value)
  a refused link between two taken ones             hoist_cases.ragged_net(p3=18) and (p3=20): test_refused_link_between_two_taken
  ragged node groups in k_stage_sum                 test_ragged_node_groups (HIGSFA_SUM_LDS: groups of one, and a last group short)
  n_cols on a hoisted top layer                     test_n_cols_on_a_hoisted_top_layer
  uneven child counts on the step lanes             test_two_lanes_give_the_serial_bits_ragged"""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import synth
from pyfaceanalysis_amd.flow import Flow
from pyfaceanalysis_amd import nodes as N
from tests import helpers, hoist_cases

pytestmark = pytest.mark.gpu
TOL = 1e-4                                                    # the project's budget, of max|ref|
SIZES = (1, 16, 17, 100, 130, 512, 728, 1100, 1738)          # k_subtree sets, k_stage_splitm, k_stage(_sum), every k_tail depth
N_REF = 1738
# every layer on the node-group sweep (k_stage / k_stage_sum): no k_stage_splitm, no top-of-hierarchy launch, no sub-trees
SWEEP_ONLY = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0"}


def rel_err(y, ref):
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max() / np.abs(ref).max())


def load(monkeypatch, nodes, env=None, prefixes=()):
    """A flow whose handle, and the handles of its prefixes nodes[:k + 1] for k in `prefixes`, were planned under the switches `env`
    (they are read once, when a handle is made)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    flow = Flow(nodes, output_dtype=np.float32)
    flow.info()
    for k in prefixes:
        flow.info(nodenr=k)
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
            if name.startswith("hf"):
                nodes = hoist_cases.hoist_fuzz_net(int(name[2:]))
            else:
                nodes = {"chain": hoist_cases.chain_net, "quad": hoist_cases.quad_net,
                         "fuzz": lambda: helpers.subtree_fuzz_net(hoist_cases.FUZZ_SEED), "ragged": hoist_cases.ragged_net,
                         "ragged_wide": hoist_cases.ragged_wide_net, "small": hoist_cases.small_net,
                         "ragged18": lambda: hoist_cases.ragged_net(p3=18), "ragged20": lambda: hoist_cases.ragged_net(p3=20)}[name]()
            _CASES[name] = Case(nodes, 900 + len(_CASES))
        return _CASES[name]
    yield get
    for c in _CASES.values():
        c.flow.close()
    _CASES.clear()


NETS = ("chain", "quad", "fuzz", "ragged", "ragged_wide", "small")
HF_NETS = tuple("hf%d" % s for s in hoist_cases.HOIST_FUZZ_SEEDS)


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
    want = {"chain": 5, "quad": 3, "ragged": 3, "ragged_wide": 3, "small": 1}.get(name)
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


def _two_lanes(c):
    import torch
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


def test_two_lanes_give_the_serial_bits(case):
    """(e): two steps in flight on the two lanes of one handle, different rows on each."""
    _two_lanes(case("chain"))


def test_two_lanes_give_the_serial_bits_ragged(case):
    """(e) with parents of 1, 3, 4 and 8 children: uneven child counts through step_lane_device."""
    _two_lanes(case("ragged"))


def per_node_errors(layer, y, ref):
    """max|d| over a node's columns / max|ref| over its columns, for every node of the layer that produced y."""
    out, c0 = [], 0
    d = np.abs(np.asarray(y, dtype=np.float64) - ref)
    for nd in layer.nodes:
        c1 = c0 + nd.output_dim
        out.append(float(d[:, c0:c1].max() / np.abs(ref[:, c0:c1]).max()))
        c0 = c1
    assert c0 == ref.shape[1]
    return out


@pytest.mark.parametrize("name", NETS + HF_NETS)
def test_every_layer_per_node_against_the_oracle(case, monkeypatch, name):
    """Every layer of every net, node by node, against the float64 oracle: flow.execute(x, nodenr=k) for each k that holds a Layer.
    A prefix is planned on its own and its last layer is never a folded child, so it returns that layer's true output while the
    layers below are hoisted as in the full net.  Per node max|d| / max|ref| over the node's columns <= 1e-4, the project's
    budget applied where one global norm would hide a small node beside a large one; 33 of 130 rows; the default handle (at this
    batch k_subtree, k_tail, k_stage_splitm), a SWEEP_ONLY handle (k_stage_sum) and the HIGSFA_NO_HOIST=1 plan as the yardstick
    of the draw's conditioning.  An added padding entry or children added in another order than they were folded in is an error of
    the order of the node's output: this is the test that sees one that every family shares.
    Measured on MI355X, worst node of any layer: the named nets hoisted 6.99e-7 (chain), unhoisted 9.46e-7; the fuzz
    seeds 3.80e-6 for both plans (seed 9, last layer), next 1.22e-6 against 1.30e-6 (seed 11)."""
    c = case(name)
    ks = [k for k, nd in enumerate(c.nodes) if isinstance(nd, N.Layer)]
    rows = np.arange(0, 130, 4)
    x = c.x[:130]
    handles = [("hoisted", load(monkeypatch, c.nodes, None, ks)), ("hoisted, node-group sweep", load(monkeypatch, c.nodes, SWEEP_ONLY, ks)),
               ("HIGSFA_NO_HOIST=1", load(monkeypatch, c.nodes, {"HIGSFA_NO_HOIST": "1"}, ks))]
    worst = {h: (0.0, -1, -1) for h, _ in handles}
    for k in ks:
        ref = oracle.execute_flow(c.nodes[:k + 1], x[rows])
        for h, flow in handles:
            errs = per_node_errors(c.nodes[k], flow.execute(x, nodenr=k)[rows], ref)
            j = int(np.argmax(errs))
            worst[h] = max(worst[h], (errs[j], k, j))
    print("%s, worst node: %s" % (name, "; ".join("%s %.3e (flow index %d, node %d)" % ((h,) + worst[h]) for h, _ in handles)))
    for _, flow in handles:
        flow.close()
    for h, _ in handles:
        assert worst[h][0] <= TOL, (h, worst[h])


@pytest.mark.parametrize("seed", hoist_cases.HOIST_FUZZ_TAKEN)
def test_fuzz_rows_bit_identical_across_kernel_families(case, monkeypatch, seed):
    """The seeds of hoist_cases.hoist_fuzz_net whose plan has a hoisted link: every family gives the bits of ONE 1100-row call of the
    default handle; HIGSFA_NO_HOIST=1 against the oracle keeps a second opinion that shares nothing with the hoisted plans."""
    c = case("hf%d" % seed)
    assert "first affine folded" in c.flow.describe()
    y = c.flow.execute(c.x[:1100])
    for env in (None, SWEEP_ONLY, {"HIGSFA_TAIL": "0"}, {"HIGSFA_SUBTREE": "0"}, {"HIGSFA_NO_FSPEC": "1"}):
        flow = load(monkeypatch, c.nodes, env)
        for n in (17, 130, 728, 1100):
            assert np.array_equal(flow.execute(c.x[:n]), y[:n]), (env, n)
        flow.close()
    plain = load(monkeypatch, c.nodes, {"HIGSFA_NO_HOIST": "1"})
    assert "first affine folded" not in plain.describe()
    idx = c.idx[c.idx < 1100]
    e0, e1 = rel_err(plain.execute(c.x[idx]), c.ref[:idx.size]), rel_err(y[idx], c.ref[:idx.size])
    print("hf%d: hoisted %.3e, HIGSFA_NO_HOIST=1 %.3e of max|ref|" % (seed, e1, e0))
    assert e0 <= TOL and e1 <= TOL
    plain.close()


@pytest.mark.parametrize("name", ("ragged18", "ragged20"))
def test_refused_link_between_two_taken(case, monkeypatch, name):
    """ragged_net with 18 or 20 columns at stage 3 (a last tile of 2 or 4 rows: the pass leaves the link alone): stage 2 is a parent
    that sums and a child that stores its own output, stage 3 multiplies and is a folded child, stage 4 sums.  Every family, the
    bits of one call; per node within the budget is test_every_layer's business on ragged, here the last layer."""
    c = case(name)
    folded = ["first affine folded" in ln for ln in c.flow.describe().splitlines() if "] fused stage " in ln]
    assert folded == [False, False, True, False, True]
    assert rel_err(c.y[c.idx], c.ref) <= TOL
    for env in (None, SWEEP_ONLY, {"HIGSFA_TAIL": "0"}, {"HIGSFA_TAIL": "1"}, {"HIGSFA_SUBTREE": "0"}):
        flow = load(monkeypatch, c.nodes, env)
        for n in (17, 130, 728, N_REF):
            assert np.array_equal(flow.execute(c.x[:n]), c.y[:n]), (env, n)
        flow.close()


@pytest.mark.parametrize("env", [None, SWEEP_ONLY, {"HIGSFA_TAIL": "0"}, {"HIGSFA_NO_FSPEC": "1"}], ids=["default", "sweep", "no-tail", "no-fspec"])
def test_children_are_added_in_first_read_order(native_lib, monkeypatch, env):
    """hoist_cases.order_probe_net: the first two children a parent reads cancel exactly, at 2^18 times the third one's size, and the
    bias vector is zero, so z is exact when the tiles are added in first-read order (1, 2, 0) and rounded to 2^-6 of its size in
    any order that puts child 0 before the pair is complete — ascending order, for one.  Every family that adds in the same wrong
    order keeps the others' bits; the float64 oracle within the project's budget is what tells."""
    nodes = hoist_cases.order_probe_net()
    flow = load(monkeypatch, nodes, env)
    assert "first affine folded" in flow.describe()
    for n in (17, 130, 1100):
        x = hoist_cases.order_probe_rows(n)
        rows = np.arange(0, n, max(1, n // 30))
        err = per_node_errors(nodes[-1], flow.execute(x)[rows], oracle.execute_flow(nodes, x[rows]))
        print("order probe, %d rows: %.3e of the node's max|ref|" % (n, err[0]))
        assert err[0] <= TOL, (n, err)
    flow.close()


SUM_STAGES = {"chain": hoist_cases.CHAIN_SUM_STAGES, "quad": hoist_cases.QUAD_SUM_STAGES, "ragged": hoist_cases.RAGGED_SUM_STAGES}


@pytest.mark.parametrize("name,kib", [("chain", 1), ("chain", 40), ("quad", 1), ("quad", 24), ("ragged", 1), ("ragged", 12)])
def test_ragged_node_groups(case, monkeypatch, name, kib):
    """k_stage_sum with node groups that leave a last group short (HIGSFA_SUM_LDS KiB / the KiB of fragments per node, at least 1):
    groups of one node, where the prefetch of the next visit's first child wraps at every node, and a group size that does not
    divide a hoisted layer's node count (3 of chain's 16, of quad's 8 and of ragged's 4).  The same bits as the default handle."""
    c = case(name)
    sizes = [max(1, min(n, kib // blocks)) for n, blocks in SUM_STAGES[name]]
    if kib == 1:
        assert set(sizes) == {1}
    else:
        assert any(g > 1 and n % g for g, (n, _) in zip(sizes, SUM_STAGES[name])), sizes
    flow = load(monkeypatch, c.nodes, dict(SWEEP_ONLY, HIGSFA_SUM_LDS=str(kib)))
    for n in (130, N_REF):
        assert np.array_equal(flow.execute(c.x[:n]), c.y[:n]), n
    flow.close()


@pytest.mark.parametrize("name,nodenr", [("chain", None), ("ragged", None), ("ragged", 5)])
def test_n_cols_on_a_hoisted_top_layer(case, monkeypatch, name, nodenr):
    """flow.execute(x, n_cols=k) is the first k columns of the full call, bit for bit, where the last layer sums its children's tiles:
    chain (20 outputs, a tile and a quarter), ragged (5 outputs: the k that fit) and ragged up to its layer of four parents of 1, 3,
    4 and 8 children (flow index 5; 4 x 24 outputs), on the top-of-hierarchy launch and on the node-group sweep with its unpack."""
    c = case(name)
    out_dim = c.nodes[-1 if nodenr is None else nodenr].output_dim
    assert "first affine folded" in [ln for ln in c.flow.describe(nodenr=nodenr).splitlines() if "] fused stage " in ln][-1]
    ks = [k for k in (1, 5, 16, 17) if k <= out_dim]
    assert len(ks) == (2 if (name, nodenr) == ("ragged", None) else 4)
    for env in (None, SWEEP_ONLY):
        flow = load(monkeypatch, c.nodes, env, () if nodenr is None else (nodenr,))
        for n in (130, N_REF):
            full = flow.execute(c.x[:n], nodenr=nodenr)
            if nodenr is None:
                assert np.array_equal(full, c.y[:n])
            for k in ks:
                assert np.array_equal(flow.execute(c.x[:n], nodenr=nodenr, n_cols=k), full[:, :k]), (env, n, k)
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
