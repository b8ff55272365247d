"""Flows for the hoisted-link tests (tests/test_hoist_plan_host.py on the CPU, tests/test_hoist_gpu.py on the device) and the
stand-alone driver that runs the planner's hoist pass without a device (tests/hoist_plan_driver.cpp).  Untrained: every weight is a
seeded draw (helpers.rand_pca / rand_sfa, or plan_cases.reseed where a digest or a float64 comparison depends on it)."""
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import helpers
from tests.plan_cases import CSRC, ROOT

FUNCS = [N.identity, N.unsigned_08expo]
FUZZ_SEED = 6      # a helpers.subtree_fuzz_net seed whose plan has a hoisted link (test_hoist_plan_host.py checks that it still has)


def _layer(rng, n, d_in, p, s):
    out = []
    for _ in range(n):
        ex = N.GeneralExpansionNode(FUNCS, p)
        out.append(N.FlowNode([helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, helpers.rand_sfa(rng, ex.output_dim, s)]))
    return N.Layer(out)


CHAIN_DIMS = [(13, 13), (20, 24), (24, 40), (40, 60), (60, 60), (60, 60), (60, 20)]


def chain_net(seed=0, dims=CHAIN_DIMS, side=32):
    """side x side input, 4x4 fields, then two-way merges down to one node.  With CHAIN_DIMS: link 0 -> 1 is not eligible (it leads
    into stage 1), links 1 -> 2 .. 5 -> 6 are (P of the parent == S of the child), with parents of 2, 3 and 4 tiles, chained, and a
    last layer whose 20 outputs fill a tile and a quarter."""
    rng = np.random.default_rng(4000 + seed)
    flow, c, w, h = [], 1, side, side
    for li, (p, s) in enumerate(dims):
        field = (4, 4) if li == 0 else ((2, 1) if (li % 2 == 1 and w > 1) or h == 1 else (1, 2))
        sb = N.Rectangular2dSwitchboard((w, h), field, field, c)
        flow += [sb, _layer(rng, sb.output_channels, sb.out_channel_dim, p, s)]
        w, h = sb.out_channels_xy
        c = s
    assert w * h == 1
    return flow


QUAD_DIMS = [(12, 24), (24, 30), (28, 36), (32, 40), (38, 10)]


def quad_net(seed=0):
    """64 x 32 input, 4x4 fields (128 nodes), three 2x2 merges (32, 8 and 2 nodes: four children per parent) and a pair merge.
    Links 1 -> 2, 2 -> 3 and 3 -> 4 are eligible; the parents of 28 and 32 columns are narrower than their children's 30 and 36."""
    rng = np.random.default_rng(4100 + seed)
    flow, c, w, h = [], 1, 64, 32
    for li, (p, s) in enumerate(QUAD_DIMS):
        field = (4, 4) if li == 0 else ((2, 2) if w > 1 and h > 1 else (2, 1))
        sb = N.Rectangular2dSwitchboard((w, h), field, field, c)
        flow += [sb, _layer(rng, sb.output_channels, sb.out_channel_dim, p, s)]
        w, h = sb.out_channels_xy
        c = s
    assert w * h == 1
    return flow


def small_net(seed=0):
    """The smallest net with a hoisted link and a permuting switchboard in front of the parents: 8 x 8 input, 16 + 4 nodes, then two
    parents that read their two children's columns through a PInvSwitchboard in a shuffled order."""
    rng = np.random.default_rng(4200 + seed)
    sb0 = N.Rectangular2dSwitchboard((8, 8), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((4, 4), (2, 2), (2, 2), 5)
    cols = []
    for pj in range(2):
        mine = np.arange(18 * pj, 18 * pj + 18)      # children 2 pj and 2 pj + 1, nine columns each
        cols.append(rng.permutation(mine))
    sb2 = N.PInvSwitchboard(36, np.concatenate(cols))
    return [sb0, _layer(rng, 16, 4, 4, 5), sb1, _layer(rng, 4, 20, 7, 9), sb2, _layer(rng, 2, 18, 6, 11)]


def igsfa_after_ordinary(seed=0):
    """An ordinary layer pair with an eligible link, but with iGSFA nodes on the parent side: not hoisted."""
    rng = np.random.default_rng(4300 + seed)
    sb0 = N.Rectangular2dSwitchboard((8, 8), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((4, 4), (2, 2), (2, 2), 6)
    sb2 = N.Rectangular2dSwitchboard((2, 2), (2, 1), (2, 1), 9)

    def ig(d_in, k, q):
        ex = N.GeneralExpansionNode(FUNCS, d_in)
        pca = helpers.rand_pca(rng, d_in, q)
        pca.avg = np.zeros_like(pca.avg)
        return N.iGSFANode(rng.normal(size=d_in), ex, helpers.rand_sfa(rng, ex.output_dim, k, N.GSFANode), rng.uniform(0.5, 2.0, size=k),
                           N.LinearRegressionNode(rng.normal(size=(k + 1, d_in)) / np.sqrt(k + 1)), pca, k)

    return [sb0, _layer(rng, 16, 4, 4, 6), sb1, _layer(rng, 4, 24, 8, 9), sb2, N.Layer([ig(18, 3, 4) for _ in range(2)])]


def build_driver(exe, extra_flags=()):
    """tests/hoist_plan_driver.cpp with plain g++ against hg_tree.cpp and hg_fused_plan.cpp only.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "hoist_plan_driver.cpp"), os.path.join(CSRC, "hg_tree.cpp"),
           os.path.join(CSRC, "hg_fused_plan.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
