"""GPU: the link 0 -> 1 folded inside the front kernels (DESIGN.md §3.1 "Hoisted links", §6.8): layer 0's second affine multiplied into
layer 1's first by the planner, so that k_stage01d / k_stage01p go from z0 straight to z1.  On the nets of tests/fold01_cases.py
(layer-0 widths 13 and 16, layer-1 widths 17 and 20, a weight draw per node, nonzero means and biases, 16 chunks) and on trained
U11L-128, at batches of 1, 16, 17 and 33 rows: a single row, one full tile, a tile and a row, and two tiles and a row (the generic
front kernel takes two tiles per pass: a full pass and a short one).

What must hold: layer 1's own output, node by node, within the project's 1e-4 of the float64 oracle, folded and with
HIGSFA_NO_FOLD01=1; the whole U11L-128 flow within §3.4's 3e-6; one set of bits from every front variant, single-tile calls and all
three input types included; the same bits from rows that allow no 16-byte loads (an odd base, an odd pitch), which a folded plan
stages with scalar loads inside k_stage01p because it has no unfused first layer to fall back on."""
import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import synth
from pyfaceanalysis_amd.flow import Flow
from tests import fold01_cases
from tests.test_hoist_gpu import TOL, load, per_node_errors, rel_err

pytestmark = pytest.mark.gpu
SIZES = (1, 16, 17, 33)
N_ROWS = 33
NO_FOLD = {"HIGSFA_NO_FOLD01": "1"}
VARIANTS = (("HIGSFA_NO_WGQ",), ("HIGSFA_NO_DIRECT",), ("HIGSFA_NO_DIRECT", "HIGSFA_NO_FSPEC"))
L1 = 3      # flow index of layer 1: [switchboard, layer 0, switchboard, layer 1, ...]


class Case(object):
    """One net: 33 rows of integer pixels (exact in uint8, float32 and float64), the float64 oracle of layer 1 and of the whole
    flow on them — computed once, never changed."""

    def __init__(self, nodes, x):
        self.nodes = nodes
        self.x8 = x
        self.ref1 = oracle.execute_flow(nodes[:L1 + 1], x)
        self.ref = oracle.execute_flow(nodes, x)


_CASES = {}


@pytest.fixture(scope="module")
def case(native_lib, nets):
    def get(name):
        if name not in _CASES:
            if name == "U11L-128":
                nodes = nets("U11L-128")
                x = synth.make_subimages(N_ROWS, 128, dtype=np.uint8)
            else:
                nodes = fold01_cases.GPU_NETS[name]()
                x = np.random.default_rng(700 + len(_CASES)).integers(0, 256, size=(N_ROWS, nodes[0].input_dim)).astype(np.uint8)
            _CASES[name] = Case(nodes, x)
        return _CASES[name]
    yield get
    _CASES.clear()


NETS = tuple(sorted(fold01_cases.GPU_NETS))


def on_device(flow, x, nodenr=None, offset=0, pad=0):
    """flow.execute_device on a device copy of x whose first element sits `offset` elements behind an aligned base and whose rows are
    `pad` elements apart beyond their width; float32 features back."""
    import torch
    dev = torch.device("cuda", 0)
    n, d = x.shape
    ldx = d + pad
    buf = torch.zeros(n * ldx + offset + 64, dtype=torch.from_numpy(x[:1]).dtype, device=dev)
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + n * ldx].view(n, ldx)
    view[:, :d] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    k = flow.flow[-1 if nodenr is None else nodenr].output_dim
    y = torch.zeros((n, k), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    flow.execute_device(view.data_ptr(), x.dtype.type, n, ldx, y.data_ptr(), np.float32, k, k,
                        stream=torch.cuda.current_stream(dev).cuda_stream, nodenr=nodenr)
    torch.cuda.synchronize(dev)
    flow.check_errors()
    return y.cpu().numpy()


def folded_lines(flow, nodenr=None):
    return [ln for ln in flow.describe(nodenr=nodenr).splitlines() if "link 0 -> 1 folded" in ln]


@pytest.mark.parametrize("name", NETS + ("U11L-128",))
def test_layer1_per_node_against_the_oracle(case, monkeypatch, name):
    """flow.execute(x, nodenr = layer 1) against the float64 oracle, node by node (max|d| over a node's columns / max|ref| over them
    <= 1e-4, tests/test_hoist_gpu.py's measure and budget), at 1, 16, 17 and 33 rows, folded and with HIGSFA_NO_FOLD01=1.  A prefix
    that ends at layer 1 is planned on its own, with the same fold.  A swapped pair of children or a bias on the wrong tile is an
    error of the order of the node's output here; a norm over the top layer could hide either.
    Measured on MI355X, worst node of any size, folded / unfolded: w13_p20_s17 5.25e-7 / 5.44e-7, w16_p17_s20
    5.14e-7 / 5.91e-7, U11L-128 1.91e-6 / 1.14e-6."""
    c = case(name)
    handles = [("folded", load(monkeypatch, c.nodes, None, (L1,))), ("HIGSFA_NO_FOLD01=1", load(monkeypatch, c.nodes, NO_FOLD, (L1,)))]
    assert len(folded_lines(handles[0][1], L1)) == 1 and len(folded_lines(handles[0][1])) == 1
    assert not folded_lines(handles[1][1], L1) and "HIGSFA_NO_FOLD01" in handles[1][1].describe(nodenr=L1)
    worst = {}
    for h, flow in handles:
        for n in SIZES:
            y = on_device(flow, c.x8[:n].astype(np.float32), nodenr=L1)
            errs = per_node_errors(c.nodes[L1], y, c.ref1[:n])
            j = int(np.argmax(errs))
            worst[h] = max(worst.get(h, (0.0, -1, -1)), (errs[j], n, j))
    print("%s, layer 1, worst node: %s" % (name, "; ".join("%s %.3e (%d rows, node %d)" % ((h,) + worst[h]) for h, _ in handles)))
    for _, flow in handles:
        flow.close()
    for h, _ in handles:
        assert worst[h][0] <= TOL, (h, worst[h])


def test_u11l_128_whole_flow_against_the_oracle(case, monkeypatch):
    """Trained U11L-128, 33 rows, all 60 features: within DESIGN.md §3.4's <= 3e-6 of max|ref|, folded and unfolded.  Measured on
    MI355X (§6.8): folded 1.204e-6, HIGSFA_NO_FOLD01=1 1.350e-6; the two plans differ by 1.665e-6 of max|y|."""
    c = case("U11L-128")
    folded, plain = load(monkeypatch, c.nodes), load(monkeypatch, c.nodes, NO_FOLD)
    y1, y0 = on_device(folded, c.x8.astype(np.float32)), on_device(plain, c.x8.astype(np.float32))
    e1, e0 = rel_err(y1, c.ref), rel_err(y0, c.ref)
    print("U11L-128, 33 rows, max|d|/max|ref|: folded %.3e, HIGSFA_NO_FOLD01=1 %.3e; folded against unfolded %.3e of max|y|"
          % (e1, e0, rel_err(y1, y0.astype(np.float64))))
    assert len(folded_lines(folded)) == 1 and not folded_lines(plain)
    folded.close()
    plain.close()
    assert e1 <= 3e-6 and e0 <= 3e-6


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["uint8", "float32", "float64"])
def test_front_variants_give_one_set_of_bits(case, monkeypatch, name, dtype):
    """The default handle (k_stage01d, one tile queue per chunk), HIGSFA_NO_WGQ (a queue per layer-1 node), HIGSFA_NO_DIRECT
    (k_stage01p, one tile per pass) and HIGSFA_NO_DIRECT + HIGSFA_NO_FSPEC (the generic k_stage01p, two tiles per pass, for which
    1 and 16 rows are a batch shorter than a pass): equal bits at every size, for layer 1's output and for the whole flow; and the
    three input types agree with each other, the pixels being integers."""
    c = case(name)
    x = c.x8.astype(dtype)
    base = load(monkeypatch, c.nodes, None, (L1,))
    assert folded_lines(base)
    want1, want = on_device(base, x, nodenr=L1), on_device(base, x)
    assert rel_err(want, c.ref) <= TOL
    if dtype is not np.uint8:
        assert np.array_equal(want, on_device(base, c.x8))
    for n in SIZES:
        assert np.array_equal(on_device(base, x[:n]), want[:n]), n
    for names in VARIANTS:
        flow = load(monkeypatch, c.nodes, {k: "1" for k in names}, (L1,))
        assert folded_lines(flow), names      # the fold does not depend on the variant
        for n in SIZES:
            assert np.array_equal(on_device(flow, x[:n], nodenr=L1), want1[:n]), (names, n)
            assert np.array_equal(on_device(flow, x[:n]), want[:n]), (names, n)
        flow.close()
    base.close()


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["uint8", "float32", "float64"])
def test_unaligned_rows_give_the_aligned_bits(case, monkeypatch, name, dtype):
    """execute_device on a buffer whose base is one element behind an aligned address, and on one whose rows are side^2 + 1 elements
    apart: the two routes to k_stage01p's scalar staging branch.  The bits of the aligned, dense call, for the default handle and
    for the generic front kernel; and with HIGSFA_NO_FOLD01=1, where such rows still take the unfused first-layer kernels."""
    c = case(name)
    x = c.x8.astype(dtype)
    for env in (None, {"HIGSFA_NO_FSPEC": "1"}, NO_FOLD):
        flow = load(monkeypatch, c.nodes, env)
        assert bool(folded_lines(flow)) == (env is not NO_FOLD)
        want = on_device(flow, x)
        for n in SIZES:
            assert np.array_equal(on_device(flow, x[:n], offset=1), want[:n]), (env, n, "base")
            assert np.array_equal(on_device(flow, x[:n], pad=1), want[:n]), (env, n, "pitch")
        flow.close()


def test_switched_off_nothing_folded_runs(case, monkeypatch):
    """HIGSFA_NO_FOLD01=1: describe says so on stage 1's line, no line claims a folded link, the issue counts on the stage lines are
    the flow's as given and no folded count is quoted, and hg_info's padded FLOPs are the same with and without the fold (it counts the flow as given).
    That the features then equal the parent commit's bit for bit was checked with bench.py --dump-outputs of both builds
    (profiles/r14_fold01.txt); here the unfolded handle must differ from the folded one only by rounding."""
    c = case(NETS[0])
    folded, plain = load(monkeypatch, c.nodes), load(monkeypatch, c.nodes, NO_FOLD)
    d1, d0 = folded.describe(), plain.describe()
    line1 = [ln for ln in d0.splitlines() if "] fused stage 1" in ln]
    assert len(line1) == 1 and "stays as it is: switched off (HIGSFA_NO_FOLD01)" in line1[0] and "link 0 -> 1 folded" not in d0
    n1 = len(c.nodes[L1].nodes)
    assert "issues %d x 16x16x4 for layer 0 and %d x 16x16x4 + %d x 4x4x1 for this layer" % (8 * n1, 26 * n1, 26 * n1) in d1
    assert " issues " not in d0
    assert folded.info().padded_flops_per_row == plain.info().padded_flops_per_row
    y1, y0 = on_device(folded, c.x8.astype(np.float32)), on_device(plain, c.x8.astype(np.float32))
    assert rel_err(y0, c.ref) <= TOL and rel_err(y1, y0.astype(np.float64)) <= TOL
    folded.close()
    plain.close()
