"""GPU: the table-driven product stage (k_stage_prod, csrc/hg_fused_prod.hip) and the iGSFA stages (k_igsfa, k_igfold,
k_igfold_split, csrc/hg_fused_igsfa.hip) at every tile width they are instantiated for and every launch shape launch_prod and
launch_igsfa (csrc/hg_fused.hip) pick — held to what the ordinary stage kind is held to: the float64 oracle node by node and layer
by layer, and a row's bits independent of the batch it travels in.  Nets and batch sizes: tests/stage_shape_cases.py, whose premises
tests/test_stage_shapes_plan_host.py pins on the CPU.

Every handle is planned under HIGSFA_DEBUG, so every launch writes one line: a product or iGSFA sweep "[prod stage i] ... shape
AxB ..." / "[igsfa stage i] ... shape AxB ...", every other route a line with a prefix of its own (k_igfold_split: "[igsplit stage
i] ..."; csrc/hg_fused_call.cpp: format_step).  The tests read the product and iGSFA lines with
capfd and hold them to the shapes the cases were sized for: a case that falls into another shape fails, it does not pass on
another kernel.  Rows go in through the device entry, one call per batch (device_call): host rows pass through the host pipeline,
which cuts a call into passes, and the shape would follow the pass.  Which test puts what on the device (DESIGN.md §6.9 has the table by instantiation):

  k_stage_prod<MT1, MT2, T>, all 16 widths, T = 1, 2     prod11 .. prod44: test_per_node_against_the_oracle, test_shapes_reached,
                                                         test_rows_bit_identical_across_batch_sizes
  a narrow node scattered into the widest node's         prod_uneven layer 0 (p = 12 beside 20); node groups of 2, 3 and 4 with a short
  column table; a short last node group                  last group of one at 425 rows: the same three tests
  k_igsfa<MS, MO, T, KBM>: ten (MS, MO), four KBM        ig_a .. ig_e under HIGSFA_IG_NOFOLD=1; 12 x 2 on ig_c's 64 nodes of 6 blocks
  k_igfold<MO, T>, MO = 1 .. 4, both expansion forms,    igfold1 .. igfold4 layer 0 (256 nodes: 8 x 2 from 425 rows, tile_groups >
  the prefetch into the next tile group                  parts from 805)
  k_igfold_split, MO = 1 .. 4                            the tops of igfold1 .. igfold4 (8 or 4 nodes), mixed
  the line between k_igfold_split and k_igfold           test_split_fold_line
  product after ordinary, iGSFA after product            mixed
  n_cols, input dtypes                                   test_n_cols_and_dtypes
  the absent second tile of a T = 2 wave                 test_nan_stays_in_its_row_at_two_tiles_per_wave, every odd tile count
  one line per launch, every stage named once            test_every_launch_of_a_call_is_reported"""
import re

import numpy as np
import pytest

from oracle import mdp_restate as oracle
from pyfaceanalysis_amd import _capi
from pyfaceanalysis_amd import nodes as N
from pyfaceanalysis_amd.flow import Flow
from tests import stage_shape_cases as cases
from tests.test_hoist_gpu import per_node_errors

pytestmark = pytest.mark.gpu
TOL = 1e-4                                                    # the project's budget, of the node's max|ref|
ROWS = cases.ROWS
N_REF = cases.N_REF
NETS = cases.nets()
NAMES = tuple(NETS)

PROD_LINE = re.compile(cases.PROD_LINE)
IG_LINE = re.compile(cases.IG_LINE)


def launches(err):
    """The product and iGSFA launches of captured stderr, in order: dicts of the debug lines' fields."""
    out = []
    for ln in err.splitlines():
        m = PROD_LINE.search(ln)
        if m:
            v = [int(g) for g in m.groups()]
            out.append(dict(kind="prod", stage=v[0], nodes=v[1], mt1=v[2], mt2=v[3], neb=v[4], shape=(v[5], v[6]), npg=v[7], node_groups=v[8],
                            tile_groups=v[9], parts=v[10]))
            continue
        m = IG_LINE.search(ln)
        if m:
            v = [int(g) for g in m.groups()]
            out.append(dict(kind="igsfa", stage=v[0], nodes=v[1], kb1=v[2], shape=(v[3], v[4]), tile_groups=v[7], parts=v[8]))
        else:
            assert "[prod stage" not in ln and "[igsfa stage" not in ln, ln      # a line of another format must not go unread
    return out


stage_table = cases.stage_table                              # what a call must launch, by design: shared with tests/test_call_plan_host.py
expected_launches = cases.expected_launches


def check_launches(name, rows, got):
    """The launches that ran are the ones the case was designed for; returns them merged with what the design says of each."""
    want = expected_launches(name, rows)
    assert [(g["kind"], g["stage"], g["nodes"], g["shape"]) for g in got] == [(w["kind"], w["stage"], w["nodes"], w["shape"]) for w in want], (name, rows)
    for g, w in zip(got, want):
        if g["kind"] == "prod":
            assert (g["mt1"], g["mt2"]) == w["widths"]
        else:
            assert g["kb1"] == w["kb1"]
    return [dict(w, name=name, rows=rows, tiles=cases.tiles(rows), **{k: g[k] for k in g if k not in w}) for g, w in zip(got, want)]


GUARD = 16      # rows behind a call's output, filled with NaN: nothing may be written past the rows asked for


def to_device(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def device_call(flow, xd, n, first=0, nodenr=None, n_cols=None):
    """Rows [first, first + n) of the device tensor xd through ONE call of the device entry.  (Host rows go through the host
    pipeline, which cuts a call into passes of its own choosing: the launch shape would follow the pass, not the batch.)"""
    import torch
    dev = xd.device
    k = flow.flow[-1 if nodenr is None else nodenr].output_dim if n_cols is None else n_cols
    y = torch.full((n + GUARD, k), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    flow.execute_device(xd[first:].data_ptr(), np.dtype(str(xd.dtype).split(".")[1]), n, xd.shape[1], y.data_ptr(), np.float32, k, k,
                        stream=torch.cuda.current_stream(dev).cuda_stream, nodenr=nodenr)
    torch.cuda.synchronize(dev)
    flow.check_errors(nodenr=nodenr)
    out = y.cpu().numpy()
    assert np.isnan(out[n:]).all(), "rows past the batch were written"
    return out[:n]


class Case(object):
    """One net: its rows, a fused and a generic flow (their handles, prefixes included, are planned under HIGSFA_DEBUG and the net's
    own switches the first time they are used), and the features of one call of all N_REF rows — computed once, never changed."""

    def __init__(self, name, seed, monkeypatch):
        make, self.env = NETS[name]
        self.name = name
        self.nodes = make()
        self.x = cases.inputs(self.nodes, seed)
        self.xd = to_device(self.x)
        self.layers = [k for k, nd in enumerate(self.nodes) if isinstance(nd, N.Layer)]
        self.flow = Flow(self.nodes, output_dtype=np.float32)
        self.generic = Flow(self.nodes, output_dtype=np.float32, force_generic=True)
        self.plan(monkeypatch)
        assert self.flow.info().plan_kind == _capi.HG_PLAN_FUSED and self.generic.info().plan_kind == _capi.HG_PLAN_GENERIC
        self.y = device_call(self.flow, self.xd, N_REF)

    def plan(self, monkeypatch):
        for k, v in dict(self.env, HIGSFA_DEBUG="1").items():
            monkeypatch.setenv(k, v)
        for k in self.layers:
            self.flow.info(nodenr=k)
            self.generic.info(nodenr=k)

    def close(self):
        self.flow.close()
        self.generic.close()


_CASES = {}


@pytest.fixture(scope="module")
def _case_store(native_lib):
    yield _CASES
    for c in _CASES.values():
        c.close()
    _CASES.clear()


@pytest.fixture
def case(_case_store, monkeypatch):
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(name, 7100 + NAMES.index(name), monkeypatch)
        return _CASES[name]
    return get


def strided_rows(n, count=30):
    """About `count` rows over the WHOLE batch, the last one included."""
    idx = np.unique(np.concatenate([np.arange(0, n, max(1, n // count)), [n - 1]]))
    return idx


def run(capfd, flow, xd, n, **kw):
    """One device call and the launches its debug lines name."""
    capfd.readouterr()
    y = device_call(flow, xd, n, **kw)
    return y, launches(capfd.readouterr().err)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", NAMES)
def test_per_node_against_the_oracle(case, capfd, name, rows):
    """(a) Every layer of every net at every batch size, node by node, against the float64 oracle: rows [:rows] through the prefix
    nodes[:k + 1] (nodenr=k) for each k that holds a Layer, on about 30 rows strided over the whole batch with the last row; per node max|d| / max|ref| over
    the node's columns <= 1e-4 (test_hoist_gpu.per_node_errors: the project's budget where one global norm would hide a small node
    beside a large one).  The generic plan under the same norm is the yardstick of the draw's conditioning.  The debug lines of the
    full call must name the shape this (net, rows) was sized for.
    Measured on MI355X (DESIGN.md §6.9 has the table), worst node of any layer and size: product nets 3.7e-7 .. 9.2e-7 fused, 4.1e-7 ..
    1.12e-6 generic; unfolded iGSFA 5.3e-7 .. 1.03e-6 against 5.7e-7 .. 1.14e-6; folded iGSFA 9.6e-7 .. 1.29e-6 against 9.7e-7 .. 1.08e-6;
    mixed 6.2e-7 both."""
    c = case(name)
    x = c.x[:rows]
    idx = strided_rows(rows)
    worst = {"fused": (0.0, -1, -1), "generic": (0.0, -1, -1)}
    for k in c.layers:
        ref = oracle.execute_flow(c.nodes[:k + 1], x[idx])
        y, got = run(capfd, c.flow, c.xd, rows, nodenr=k)
        if k == c.layers[-1]:
            check_launches(name, rows, got)
            assert np.array_equal(y, c.y[:rows])      # the prefix that ends in the last layer is the full net
        for h, yy in (("fused", y), ("generic", device_call(c.generic, c.xd, rows, nodenr=k))):
            assert yy.shape == (rows, c.nodes[k].output_dim)
            errs = per_node_errors(c.nodes[k], yy[idx], ref)
            j = int(np.argmax(errs))
            worst[h] = max(worst[h], (errs[j], k, j))
    print("%s, %d rows, worst node: %s" % (name, rows, "; ".join("%s %.3e (flow index %d, node %d)" % ((h,) + worst[h]) for h in ("fused", "generic"))))
    for h in ("generic", "fused"):
        assert worst[h][0] <= TOL, (h, worst[h])


def test_shapes_reached(case, capfd):
    """(b) From the debug lines of one call per (net, batch size), each held to its design by check_launches:
    k_stage_prod ran every (MT1, MT2) at T = 1 and at T = 2, in the shapes 8 x 2, 4 x 2, 4 x 1 and the shrunk default; k_igsfa every
    (MS, MO) and K-block capacity at T = 1 and T = 2, in 12 x 2, 8 x 2, 4 x 2 chosen and the fallbacks 4 x 2, 2 x 2, 1 x 2, 1 x 1;
    k_igfold MO = 1 .. 4 at T = 1 and T = 2.  Every two-tile shape ran on an odd tile count (a wave whose second tile is absent); each
    of the three kernels ran with tile_groups > parts > 1 (a workgroup that walks more than one tile group: k_igfold's prefetch
    into the next one) and k_stage_prod with a short last node group."""
    ran = []
    for name in NAMES:
        c = case(name)
        # describe() names the tile widths of every product stage and the fold of every iGSFA stage as the cases file states them
        listed = c.flow.describe().splitlines()
        prod_listed = [l for l in listed if "table-driven expansion" in l]
        assert [l.split(", tiles ")[1].split(",")[0] for l in prod_listed] == ["%dx%d" % (s["mt1"], s["mt2"]) for s in stage_table(name) if s["kind"] == "prod"], name
        ig_listed = [l for l in listed if "fused iGSFA stage" in l]
        assert [("folded to one GEMM" in l) for l in ig_listed] == [s["folded"] for s in stage_table(name) if s["kind"] == "igsfa"], name
        assert [int(l.split("out tiles ")[1].split(",")[0]) for l in ig_listed] == [s["mo"] for s in stage_table(name) if s["kind"] == "igsfa"], name
        for rows in ROWS:
            y, got = run(capfd, c.flow, c.xd, rows)
            ran += check_launches(name, rows, got)
            assert y.shape[0] == rows
    prod = [r for r in ran if r["kind"] == "prod"]
    unf = [r for r in ran if r["kind"] == "igsfa" and not r["folded"]]
    fold = [r for r in ran if r["kind"] == "igsfa" and r["folded"]]
    # k_stage_prod
    assert {(r["widths"], r["shape"][1]) for r in prod} >= {(w, t) for w in cases.PROD_PAIRS for t in (1, 2)}
    assert {r["shape"] for r in prod} == {(8, 2), (4, 2), (4, 1), (2, 1), (1, 1)}
    for w in cases.PROD_PAIRS:      # every width in every shape of the 64-node layer
        assert {r["shape"] for r in prod if r["widths"] == w and r["nodes"] == 64} == set(cases.PROD_SHAPES_64.values()), w
    for sh in ((8, 2), (4, 2)):
        assert any(r["shape"] == sh and r["tiles"] % 2 for r in prod), sh
    assert any(r["tile_groups"] > r["parts"] > 1 for r in prod)
    assert any(r["shape"] == (8, 2) and r["tile_groups"] % r["parts"] for r in prod)
    assert any(r["nodes"] % r["npg"] and r["npg"] > 1 for r in prod)
    # prod_uneven layer 0: node groups of 2, 3 and 4 with the shape; 3 leaves a last group of one
    assert {(r["shape"], r["npg"]) for r in prod if r["name"] == "prod_uneven" and r["stage"] == 1} >= {((8, 2), 2), ((4, 2), 3), ((4, 1), 4)}
    # k_igsfa
    assert {(r["widths"], r["shape"][1]) for r in unf} >= {(w, t) for w in cases.IG_PAIRS for t in (1, 2)}
    assert {((r["kb1"] + 1) // 2 * 2, r["shape"][1]) for r in unf} == {(kbm, t) for kbm in (2, 4, 6, 8) for t in (1, 2)}
    assert {r["shape"] for r in unf if not r["fallback"]} == {(12, 2), (8, 2), (4, 2)}
    assert {r["shape"] for r in unf if r["fallback"]} == {(4, 2), (2, 2), (1, 2), (1, 1)}
    for sh in ((12, 2), (8, 2), (4, 2)):
        assert any(r["shape"] == sh and not r["fallback"] and r["tiles"] % 2 for r in unf), sh
    assert any(r["tile_groups"] > r["parts"] > 1 for r in unf)
    # k_igfold
    assert {(r["widths"][1], r["shape"][1]) for r in fold} == {(mo, t) for mo in (1, 2, 3, 4) for t in (1, 2)}
    assert {r["shape"] for r in fold if not r["fallback"]} == {(8, 2), (4, 2)}
    assert {r["shape"] for r in fold if r["fallback"]} >= {(2, 2), (1, 2), (1, 1)}
    for sh in ((8, 2), (4, 2)):
        assert any(r["shape"] == sh and not r["fallback"] and r["tiles"] % 2 for r in fold), sh
    for mo in (1, 2, 3, 4):      # the prefetch into the next tile group (has_next) at every width
        assert any(r["widths"][1] == mo and r["tile_groups"] > r["parts"] > 1 for r in fold), mo


def test_every_launch_of_a_call_is_reported(case, capfd, monkeypatch):
    """Under HIGSFA_DEBUG every launch of a call writes one line, so the lines of ONE call name every stage exactly once, in order
    (cases.covered_stages: "[front]" is layers 0 and 1, "... stage i] layers k" stages i .. i + k - 1); a launch that went unreported
    would leave its stages out.  mixed_net (ordinary from the caller's rows, product, folded iGSFA, ordinary top) at 1, 2 and 27
    tiles, and tests/pair_cases.three_pair_net with its summed links at the row count tests/test_pair_gpu.py reads them at.  The
    product / iGSFA / pair assertions of the other tests hold on the same captures."""
    from tests import pair_cases
    from tests.test_pair_gpu import PAIRED
    c = case("mixed")
    n_stages = c.flow.info().n_stages - 1      # (the last entry is the pass that writes the caller's rows)
    assert n_stages == len(cases.MIXED_KINDS)
    for rows in (1, 17, 425):
        capfd.readouterr()
        y = device_call(c.flow, c.xd, rows)
        err = capfd.readouterr().err
        assert cases.covered_stages(err) == list(range(n_stages)), (rows, err[-2000:])
        check_launches("mixed", rows, launches(err))
        assert np.array_equal(y, c.y[:rows])
    nodes = pair_cases.three_pair_net()
    for k, v in dict(PAIRED, HIGSFA_DEBUG="1").items():
        monkeypatch.setenv(k, v)
    flow = Flow(nodes, output_dtype=np.float32)
    n_stages = flow.info().n_stages - 1
    assert n_stages == 5
    xd = to_device(np.random.default_rng(950).normal(size=(130, nodes[0].input_dim)).astype(np.float32))
    capfd.readouterr()
    device_call(flow, xd, 130)
    err = capfd.readouterr().err
    flow.close()
    assert cases.covered_stages(err) == list(range(n_stages)), err[-2000:]
    assert "[pair stage 2]" in err and "[pair stage 3]" in err and "[pair stage 4]" not in err and "[pair stage 1]" not in err
    assert launches(err) == []


@pytest.mark.parametrize("name", NAMES)
def test_rows_bit_identical_across_batch_sizes(case, name):
    """(c) A row's features do not depend on the batch it came in: rows [:n] at every size equal those rows of ONE call of 1738
    rows, and a window from the middle equals its rows.  Every product and iGSFA kernel adds a tile's terms in an order that does not
    depend on T, the waves per workgroup, the node group or tile_parts; this pins it.  (Its limit: test_split_fold_line.)  Host rows,
    which the host pipeline cuts into passes of its own choosing, give the same bits once more."""
    c = case(name)
    for n in ROWS:
        assert np.array_equal(device_call(c.flow, c.xd, n), c.y[:n]), n
    assert np.array_equal(device_call(c.flow, c.xd, 130, first=300), c.y[300:430])
    assert np.array_equal(c.flow.execute(c.x), c.y)
    assert np.array_equal(c.flow.execute(c.x[300:430]), c.y[300:430])


def test_split_fold_line(native_lib, monkeypatch, capfd):
    """(d) A folded first layer of 8 nodes at 32768 rows (8 x 2048 tiles = 16384: k_igfold_split, no "[igsfa stage" line) and at 32784 rows
    (8 x 2049: k_igfold, one line): each against the oracle per node on 30 strided rows.  k_igfold_split adds function-major,
    k_igfold K-block-major, so the first 32768 rows need not keep their bits across the line: what they do is printed, not asserted
    (DESIGN.md §6.9 records it beside the batch-independence claim).  On either side of the line rows keep their bits.
    Measured on MI355X: the rows change bits across the line, by 6.93e-7 of max|y|; worst node against the oracle 5.23e-7 below the
    line, 4.87e-7 above it."""
    monkeypatch.setenv("HIGSFA_DEBUG", "1")
    nodes = cases.ig_split_line_net()
    n0, n1 = cases.SPLIT_LINE_ROWS
    x = cases.inputs(nodes, 7200, n1)
    xd = to_device(x)
    flow = Flow(nodes, output_dtype=np.float32)
    assert flow.info().plan_kind == _capi.HG_PLAN_FUSED
    y0, got0 = run(capfd, flow, xd, n0)
    y1, got1 = run(capfd, flow, xd, n1)
    assert got0 == []
    assert [(g["kind"], g["nodes"], g["kb1"], g["shape"]) for g in got1] == [("igsfa", 8, 5, (8, 2))]
    # below the line, and above it, a row's bits do not depend on its batch
    assert np.array_equal(run(capfd, flow, xd, 1738)[0], y0[:1738])
    y2, got2 = run(capfd, flow, xd, n0, first=16)      # 2048 tiles again, other rows: k_igfold_split
    assert got2 == [] and np.array_equal(y2[:1722], y0[16:1738])
    y3, got3 = run(capfd, flow, xd, n1 - 5, first=5)      # 2049 tiles, the last one partly filled: k_igfold
    assert len(got3) == 1 and np.array_equal(y3, y1[5:])
    flow.close()
    for y, n in ((y0, n0), (y1, n1)):
        idx = strided_rows(n)
        errs = per_node_errors(nodes[1], y[idx], oracle.execute_flow(nodes, x[idx]))
        print("split/fold line, %d rows: worst node %.3e of its max|ref|" % (n, max(errs)))
        assert max(errs) <= TOL, (n, errs)
    same = np.array_equal(y0, y1[:n0])
    d = np.abs(y0.astype(np.float64) - y1[:n0]).max() / np.abs(y0).max()
    print("split/fold line: rows [:%d] %s across the line (max|d| / max|y| = %.3e)" % (n0, "keep their bits" if same else "change bits", d))
    assert d <= TOL


@pytest.mark.parametrize("name", ("prod_uneven", "igfold2", "igfold3", "mixed"))
def test_n_cols_and_dtypes(case, name):
    """(e) execute(x, n_cols=k) is the first k columns of the full call, bit for bit, for k in (1, 5, 16, 17); integer-valued pixels
    give the same bits as uint8, float32 and float64 rows.  425 rows: the 4 x 2 / 8 x 2 shapes with an odd tile count."""
    c = case(name)
    n = 425
    full = device_call(c.flow, c.xd, n)
    assert np.array_equal(full, c.y[:n])
    ks = [k for k in (1, 5, 16, 17) if k <= full.shape[1]]
    assert len(ks) == 4
    for k in ks:
        assert np.array_equal(device_call(c.flow, c.xd, n, n_cols=k), full[:, :k]), k
        assert np.array_equal(c.flow.execute(c.x[:n], n_cols=k), full[:, :k]), k
    u8 = np.random.default_rng(7300).integers(0, 256, size=(n, c.nodes[0].input_dim), dtype=np.uint8)
    y8 = device_call(c.flow, to_device(u8), n)
    assert np.isfinite(y8).all()
    assert np.array_equal(device_call(c.flow, to_device(u8.astype(np.float32)), n), y8)
    assert np.array_equal(device_call(c.flow, to_device(u8.astype(np.float64)), n), y8)
    assert np.array_equal(device_call(c.flow, to_device(u8), n, n_cols=ks[-1]), y8[:, :ks[-1]])
    for dt in (np.uint8, np.float32, np.float64):      # and as host rows
        assert np.array_equal(c.flow.execute(u8.astype(dt)), y8), dt


@pytest.mark.parametrize("name", ("prod22", "igfold1", "igfold2"))
def test_nan_stays_in_its_row_at_two_tiles_per_wave(case, capfd, name):
    """(f) 425 rows are 27 tiles: in the T = 2 kernels the wave that takes tile 26 has no second tile, loads tile 26 again in its
    place and must not store it.  One NaN pixel in row 420 (tile 26): every other row is bit-identical to the clean run, row 420
    comes back non-finite."""
    c = case(name)
    n, row = 425, 420
    bad = c.x[:n].copy()
    bad[row, c.nodes[0].input_dim // 2 + 3] = np.nan
    y, got = run(capfd, c.flow, to_device(bad), n)
    first = check_launches(name, n, got)[0]
    assert first["shape"][1] == 2 and first["tiles"] == 27 and row // 16 == 26
    keep = np.ones(n, dtype=bool)
    keep[row] = False
    assert np.array_equal(y[keep], c.y[:n][keep])
    assert not np.isfinite(y[row]).all()
