"""GPU: the folded link's four one-row k-steps packed into one inside the front kernels (DESIGN.md §3.1 "The link 0 -> 1", §6.12):
registers 0..2 of both children and both functions, then ONE k-step whose k-rows are feature 12 of child 0, of child 1, and their
powers.  On the nets of tests/fold01_cases.py (layer-0 width 13: packed; width 16: folded, not packed) and on the probe net of
tests/fold01_pack_cases.py, in which every row of F_c except the four of feature 12 is zero — layer 1's first affine is there the
packed k-step alone, and a lane group or a child taken for another shows at the order of the node's output.

130 rows (eight tiles and two rows); rows used 1, 15, 16, 17, 33 and 130.  What must hold: layer 1 node by node and the whole flow
within 1e-4 of the float64 oracle; one set of bits from k_stage01d with either tile queue, from k_stage01p at one and at two tiles
per pass and from its scalar staging (an odd base, an odd pitch); from uint8, float32 and float64 pixels; from every batch size; from
two lanes; a NaN row disturbs no other row; and HIGSFA_NO_FOLD01_PACK=1 gives other bits within the budget."""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd.flow import Flow
from tests import fold01_pack_cases as cases
from tests.test_fold01_gpu import L1, folded_lines, on_device
from tests.test_hoist_gpu import TOL, load, per_node_errors, rel_err

pytestmark = pytest.mark.gpu
SIZES = (1, 15, 16, 17, 33, 130)
N_ROWS = 130
NO_PACK = {"HIGSFA_NO_FOLD01_PACK": "1"}
VARIANTS = (("HIGSFA_NO_WGQ",), ("HIGSFA_NO_DIRECT",), ("HIGSFA_NO_DIRECT", "HIGSFA_NO_FSPEC"))
NETS = tuple(sorted(cases.GPU_NETS))
PACKED = ("probe", "w13_p20_s17")


class Case(object):
    """One net: 130 rows of integer pixels (exact in uint8, float32 and float64), the float64 oracle of layer 1 and of the whole flow
    on them, and the default handle's features for them — computed once, never changed."""

    def __init__(self, nodes, x):
        self.nodes = nodes
        self.x8 = x
        self.ref1 = oracle.execute_flow(nodes[:L1 + 1], x)
        self.ref = oracle.execute_flow(nodes, x)
        self.flow = Flow(nodes, output_dtype=np.float32)
        self.flow.info()
        self.flow.info(nodenr=L1)
        self.y1 = on_device(self.flow, x.astype(np.float32), nodenr=L1)
        self.y = on_device(self.flow, x.astype(np.float32))


_CASES = {}


@pytest.fixture(scope="module")
def case(native_lib):
    def get(name):
        if name not in _CASES:
            nodes = cases.GPU_NETS[name]()
            x = np.random.default_rng(800 + len(_CASES)).integers(0, 256, size=(N_ROWS, nodes[0].input_dim)).astype(np.uint8)
            _CASES[name] = Case(nodes, x)
        return _CASES[name]
    yield get
    for c in _CASES.values():
        c.flow.close()
    _CASES.clear()


def packed_lines(flow, nodenr=None):
    return [ln for ln in flow.describe(nodenr=nodenr).splitlines() if "one-row k-steps packed" in ln]


@pytest.mark.parametrize("name", NETS)
def test_layer1_and_flow_against_the_oracle(case, name):
    """Layer 1 node by node (execute(x, nodenr = layer 1): max|d| over a node's columns / max|ref| over them <= 1e-4, the project's
    budget) at every size, and all features of the whole flow, against the float64 oracle.  The 13-wide nets say so on stage 1's line,
    of the prefix's plan too; the 16-wide one names why not.
    Measured on MI355X, worst layer-1 node of any size / whole flow: see profiles/r25_fold01_pack.txt."""
    c = case(name)
    assert len(folded_lines(c.flow)) == 1
    assert (len(packed_lines(c.flow)) == 1 and len(packed_lines(c.flow, L1)) == 1) == (name in PACKED)
    if name not in PACKED:
        assert "one-row k-steps stay as they are: a layer-0 node has 16 outputs" in c.flow.describe()
    worst = (0.0, -1, -1)
    for n in SIZES:
        y = on_device(c.flow, c.x8[:n].astype(np.float32), nodenr=L1)
        errs = per_node_errors(c.nodes[L1], y, c.ref1[:n])
        j = int(np.argmax(errs))
        worst = max(worst, (errs[j], n, j))
    e = rel_err(c.y, c.ref)
    print("%s: layer 1, worst node %.3e (%d rows, node %d); whole flow %.3e of max|ref|" % ((name,) + worst + (e,)))
    assert worst[0] <= TOL, worst
    assert e <= TOL


@pytest.mark.parametrize("name", NETS)
def test_rows_do_not_depend_on_the_batch(case, name):
    """Rows [:n] of a call of 1, 15, 16, 17 and 33 rows equal those rows of the 130-row call, for layer 1 and for the whole flow."""
    c = case(name)
    x = c.x8.astype(np.float32)
    for n in SIZES:
        assert np.array_equal(on_device(c.flow, x[:n], nodenr=L1), c.y1[:n]), n
        assert np.array_equal(on_device(c.flow, x[:n]), c.y[:n]), n
    assert np.array_equal(on_device(c.flow, x[97:130]), c.y[97:130])


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["uint8", "float32", "float64"])
def test_front_variants_give_one_set_of_bits(case, monkeypatch, name, dtype):
    """The default handle (k_stage01d, one tile queue per chunk), HIGSFA_NO_WGQ (a queue per layer-1 node), HIGSFA_NO_DIRECT
    (k_stage01p, one tile per pass) and HIGSFA_NO_DIRECT + HIGSFA_NO_FSPEC (the generic k_stage01p, two tiles per pass): equal bits
    at every size, for layer 1's output and the whole flow, whatever the pixels' type."""
    c = case(name)
    x = c.x8.astype(dtype)
    assert np.array_equal(on_device(c.flow, x), c.y) and np.array_equal(on_device(c.flow, x, nodenr=L1), c.y1)
    for names in VARIANTS:
        flow = load(monkeypatch, c.nodes, {k: "1" for k in names}, (L1,))
        assert bool(packed_lines(flow)) == (name in PACKED), names      # neither the fold nor the packing depends on the variant
        for n in SIZES:
            assert np.array_equal(on_device(flow, x[:n], nodenr=L1), c.y1[:n]), (names, n)
            assert np.array_equal(on_device(flow, x[:n]), c.y[:n]), (names, n)
        flow.close()


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["uint8", "float32", "float64"])
def test_unaligned_rows_give_the_aligned_bits(case, monkeypatch, name, dtype):
    """A buffer whose base is one element behind an aligned address, and one whose rows are side^2 + 1 elements apart: k_stage01p's
    scalar staging, at one tile per pass (the default handle) and at two (HIGSFA_NO_FSPEC).  The bits of the aligned, dense call."""
    c = case(name)
    x = c.x8.astype(dtype)
    for env in (None, {"HIGSFA_NO_FSPEC": "1"}):
        flow = c.flow if env is None else load(monkeypatch, c.nodes, env)
        for n in SIZES:
            assert np.array_equal(on_device(flow, x[:n], offset=1), c.y[:n]), (env, n, "base")
            assert np.array_equal(on_device(flow, x[:n], pad=1), c.y[:n]), (env, n, "pitch")
        if env is not None:
            flow.close()


@pytest.mark.parametrize("name", PACKED)
def test_a_nan_row_leaves_the_others_alone(case, monkeypatch, name):
    """Rows 5 and 16 all NaN (float32): every other row keeps its bits and these two are not finite; in k_stage01d and in both
    k_stage01p forms.  (The packed k-step adds the two children's registers 3, each lane group's value to the other child's exact
    zero: a NaN stays in its own sub-image's column of the B operand.)"""
    c = case(name)
    x = c.x8[:33].astype(np.float32)
    x[[5, 16]] = np.nan
    keep = np.setdiff1d(np.arange(33), [5, 16])
    for names in ((),) + VARIANTS[1:]:
        flow = c.flow if not names else load(monkeypatch, c.nodes, {k: "1" for k in names}, (L1,))
        y1, y = on_device(flow, x, nodenr=L1), on_device(flow, x)
        assert np.array_equal(y1[keep], c.y1[keep]) and np.array_equal(y[keep], c.y[keep]), names
        assert not np.isfinite(y1[[5, 16]]).any(), names
        if names:
            flow.close()


@pytest.mark.parametrize("name", PACKED)
def test_two_lanes_give_the_serial_bits(case, name):
    """Two steps in flight on the two lanes of one handle, different rows on each, twice."""
    import torch
    from pyfaceanalysis_amd.sharded import _side_stream
    c = case(name)
    dev = torch.device("cuda", 0)
    _side_stream(torch, dev)      # the process's shared side stream first, as tests/test_hoist_gpu.py does
    k = c.y.shape[1]
    flow = Flow(c.nodes, output_dtype=np.float32)
    assert flow.set_lanes(2) and flow.lanes() == 2
    xf = c.x8.astype(np.float32)
    xs = [torch.from_numpy(xf[:97]).to(dev), torch.from_numpy(xf[97:]).to(dev)]
    ys = [torch.zeros((x.shape[0], k), dtype=torch.float32, device=dev) for x in xs]
    torch.cuda.synchronize(dev)
    for rnd in range(2):
        for lane in (0, 1):
            x, y = xs[lane], ys[lane]
            flow.step_lane_device(lane, x.data_ptr(), np.float32, x.shape[0], x.shape[1], y.data_ptr(), np.float32, k, k)
        for lane in (0, 1):
            flow.lane_join(lane)
        torch.cuda.synchronize(dev)
        assert np.array_equal(ys[0].cpu().numpy(), c.y[:97]) and np.array_equal(ys[1].cpu().numpy(), c.y[97:]), rnd
    flow.check_errors()
    flow.close()


@pytest.mark.parametrize("name", PACKED)
def test_the_switch_switches(case, monkeypatch, name):
    """HIGSFA_NO_FOLD01_PACK=1: stage 1's line says so and no line claims packed k-steps; layer 1 and the whole flow stay within the
    budget of the oracle and of the default handle, and differ from it somewhere (another order of products); hg_info's padded
    FLOPs count the flow as given either way."""
    c = case(name)
    plain = load(monkeypatch, c.nodes, NO_PACK, (L1,))
    d0 = plain.describe()
    assert not packed_lines(plain) and len(folded_lines(plain)) == 1
    assert "one-row k-steps stay as they are: switched off (HIGSFA_NO_FOLD01_PACK)" in d0
    n1 = len(c.nodes[L1].nodes)
    assert "this layer then issues %d x 16x16x4 + %d x 4x4x1" % (23 * n1, 23 * n1) in c.flow.describe()
    assert plain.info().padded_flops_per_row == c.flow.info().padded_flops_per_row
    x = c.x8.astype(np.float32)
    y1, y = on_device(plain, x, nodenr=L1), on_device(plain, x)
    plain.close()
    e1 = max(per_node_errors(c.nodes[L1], y1, c.ref1))
    print("%s, HIGSFA_NO_FOLD01_PACK=1: layer 1 worst node %.3e, whole flow %.3e of max|ref|; against the default %.3e of max|y|"
          % (name, e1, rel_err(y, c.ref), rel_err(c.y, y.astype(np.float64))))
    assert e1 <= TOL and rel_err(y, c.ref) <= TOL and rel_err(c.y, y.astype(np.float64)) <= TOL
    assert not np.array_equal(y1, c.y1) and not np.array_equal(y, c.y)
