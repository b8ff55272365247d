"""GPU: the node-group sweep kernels after DESIGN.md §6.11 — in k_stage a visit's stores stand in straight-line code (a wave whose
second tile does not exist stores its first tile twice), the packed slot is read a visit ahead and the first K-block of a streaming
visit is multiplied on its own.  None of it may change a bit: every accumulator sees the same products and additions in the same
order.  (k_stage_sum and k_stage_sum_pair were measured with the same change and with the second child's tiles requested a visit
ahead, and keep their old form: §6.11.  Their nets stay here: the cases are the ones a second attempt has to pass.)

Four nets (tests/visit_waits_cases.py), each planned twice: under the sweep-forcing switches, so that nets this small reach k_stage,
k_stage_sum and k_stage_sum_pair at all, and without them (k_stage_splitm, k_tail, k_subtree at these sizes, which the change does
not touch).  The rows 1 .. 81 run one tile per wave (the planner's choice below 8 x 2 tiles per workgroup on 256 workgroups);
test_two_tiles_per_wave_odd_tile_count adds, per net, the batch at which the sweep takes two tiles per wave with an odd tile count:
the last wave of the last tile group then holds a tile that does not exist.

Not checked here: the workspace tile after the batch's last.  No entry of the library reads the activation workspace back; what
the kernels could write past the batch is seen only through the caller's buffer (test_rows_past_the_batch_are_untouched)."""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import nodes as N
from pyfaceanalysis_amd.flow import Flow
from tests import visit_waits_cases as VC
from tests.test_hoist_gpu import per_node_errors

pytestmark = pytest.mark.gpu
TOL = 1e-4                                                    # the project's budget, of a node's max|ref|


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
    """One net: its rows, the sweep handle (with the prefixes of every layer) and the default handle, and ONE call of all 81 rows on
    each — made once, never changed."""

    def __init__(self, monkeypatch, name):
        make, self.env, self.n_big = VC.NETS[name]
        self.nodes = make()
        self.ks = [k for k, nd in enumerate(self.nodes) if isinstance(nd, N.Layer)]
        n = max(VC.N_ALL, (self.n_big or 0) + 16)
        self.x = np.random.default_rng(960 + len(name)).normal(size=(n, self.nodes[0].input_dim)).astype(np.float32)
        self.sweep = load(monkeypatch, self.nodes, self.env, self.ks)
        self.plain = load(monkeypatch, self.nodes, {})
        self.y = self.sweep.execute(self.x[:VC.N_ALL])


_CASES = {}


@pytest.fixture(scope="module")
def case(native_lib):
    mp = pytest.MonkeyPatch()

    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(mp, name)
        return _CASES[name]
    yield get
    for c in _CASES.values():
        c.sweep.close()
        c.plain.close()
    _CASES.clear()
    mp.undo()


@pytest.mark.parametrize("name", sorted(VC.NETS))
def test_sweep_rows_have_the_other_families_bits(case, name):
    """Rows 1, 16, 17, 33, 49 and 81 through the sweep handle: the bits of the handle planned without the sweep-forcing switches, and
    the bits of rows [:n] of ONE 81-row call."""
    c = case(name)
    assert np.array_equal(c.plain.execute(c.x[:VC.N_ALL]), c.y)
    for n in VC.ROWS:
        y = c.sweep.execute(c.x[:n])
        assert np.array_equal(y, c.plain.execute(c.x[:n])), n
        assert np.array_equal(y, c.y[:n]), n


@pytest.mark.parametrize("name", sorted(VC.NETS))
def test_every_layer_per_node_against_the_oracle(case, name):
    """Every layer through the sweep handle's execute(x, nodenr=k), node by node, within 1e-4 of the float64 oracle (a prefix's last
    layer stores its own output; the links below it run as in the full net)."""
    c = case(name)
    rows = np.arange(0, VC.N_ALL, 4)
    x = c.x[:VC.N_ALL]
    worst = (0.0, -1, -1)
    for k in c.ks:
        ref = oracle.execute_flow(c.nodes[:k + 1], x[rows])
        errs = per_node_errors(c.nodes[k], c.sweep.execute(x, nodenr=k)[rows], ref)
        j = int(np.argmax(errs))
        worst = max(worst, (errs[j], k, j))
    print("%s, worst node: %.3e of its max|ref| (flow index %d, node %d)" % ((name,) + worst))
    assert worst[0] <= TOL, worst


@pytest.mark.parametrize("name", sorted(VC.NETS))
def test_rows_past_the_batch_are_untouched(case, name):
    """The caller's output has 16 rows more than the batch, filled with a sentinel: rows [:n] are the bits of the 81-row call, the
    rows past the batch keep the sentinel — 17, 33 and 49 rows end inside a tile, 16 rows end on one."""
    import torch
    c = case(name)
    dev = torch.device("cuda", 0)
    k = c.y.shape[1]
    for n in (1, 16, 17, 33, 49):
        x = torch.from_numpy(c.x[:n]).to(dev)
        y = torch.full((n + 16, k), VC.SENTINEL, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        c.sweep.execute_device(x.data_ptr(), np.float32, n, x.shape[1], y.data_ptr(), np.float32, k, k)
        torch.cuda.synchronize(dev)
        out = y.cpu().numpy()
        assert np.array_equal(out[:n], c.y[:n]), n
        assert np.all(out[n:] == VC.SENTINEL), n
    c.sweep.check_errors()


@pytest.mark.parametrize("name", sorted(k for k, v in VC.NETS.items() if v[2]))
def test_two_tiles_per_wave_odd_tile_count(case, name):
    """The batch at which the sweep takes two tiles per wave, with an odd tile count: the last wave of the last tile group computes its
    first tile twice and stores it twice.  The rows are the bits of the same rows in a call of one tile more (an even count: no wave
    holds a duplicate), the last tile's rows included, and the last rows stay within the budget of the float64 oracle."""
    c = case(name)
    n = c.n_big
    assert ((n + 15) // 16) % 2 == 1
    y_even = c.sweep.execute(c.x[:n + 16])
    y = c.sweep.execute(c.x[:n])
    assert np.array_equal(y, y_even[:n])
    rows = np.concatenate([np.arange(0, n - 16, max(1, n // 12)), np.arange(n - 16, n, 3)])      # a dozen rows and the last tile's
    errs = per_node_errors(c.nodes[-1], y[rows], oracle.execute_flow(c.nodes, c.x[rows]))
    print("%s, %d rows (%d tiles), worst node of the last layer: %.3e of its max|ref|" % (name, n, (n + 15) // 16, max(errs)))
    assert max(errs) <= TOL, errs
