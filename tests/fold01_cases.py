"""Flows for the tests of the folded link 0 -> 1 (tests/test_fold01_plan_host.py on the CPU, tests/test_fold01_gpu.py on the device)
and the stand-alone driver that plans them without a device (tests/fold01_plan_driver.cpp).  Untrained: every weight, mean and
bias is a seeded draw of its own (helpers.rand_pca / rand_sfa: nonzero means in both layers, and the SFA nodes' nonzero bias).

Every net starts as the front kernels need it (Planner::can_fuse01): 4 x 4 pixel fields, first-layer nodes of 13..16 outputs, and a
second layer whose node n reads first-layer nodes 2 n and 2 n + 1."""
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import helpers
from tests.plan_cases import CSRC, ROOT

FUNCS = [N.identity, N.unsigned_08expo]


def _layer(rng, n, d_in, p, s, funcs=None):
    out = []
    for _ in range(n):
        ex = N.GeneralExpansionNode(funcs or FUNCS, p)
        out.append(N.FlowNode([helpers.rand_pca(rng, d_in, p, N.WhiteningNode), ex, helpers.rand_sfa(rng, ex.output_dim, s)]))
    return N.Layer(out)


def fold_net(w0, p1, s1, side=(16, 16), upper=(), funcs1=None, seed=0):
    """side[0] x side[1] pixels, 4x4 fields with w0 outputs (both affines of layer 0), pairs of them merged by layer-1 nodes with
    affines of p1 and s1 outputs, then one two-way merge per (p, s) of `upper`.  A chunk of the first layer holds the nodes of 128
    columns of a sub-image: 16 x 16 pixels make 16 nodes in two chunks."""
    rng = np.random.default_rng(5000 + seed)
    w, h = side
    sb = N.Rectangular2dSwitchboard((w, h), (4, 4), (4, 4), 1)
    flow = [sb, _layer(rng, sb.output_channels, 16, w0, w0)]
    w, h = sb.out_channels_xy
    sb = N.Rectangular2dSwitchboard((w, h), (2, 1), (2, 1), w0)
    flow += [sb, _layer(rng, sb.output_channels, 2 * w0, p1, s1, funcs1)]
    w, h = sb.out_channels_xy
    c = s1
    for li, (p, s) in enumerate(upper):
        field = (1, 2) if (li % 2 == 0 and h > 1) or w == 1 else (2, 1)
        sb = N.Rectangular2dSwitchboard((w, h), field, field, c)
        flow += [sb, _layer(rng, sb.output_channels, sb.out_channel_dim, p, s)]
        w, h = sb.out_channels_xy
        c = s
    return flow


# the two ends of both ranges: layer-0 widths 13 and 16, layer-1 widths 17 and 20 (first and second affine crossed)
HOST_NETS = {"w13_p20_s17": lambda: fold_net(13, 20, 17), "w16_p17_s20": lambda: fold_net(16, 17, 20),
             "w13_p17_s17": lambda: fold_net(13, 17, 17, seed=1), "w16_p20_s20": lambda: fold_net(16, 20, 20, seed=2)}


def igsfa_layer1_net(seed=0):
    """Layer 1 of iGSFA nodes on the pairs (26 inputs each)."""
    rng = np.random.default_rng(5100 + seed)
    sb0 = N.Rectangular2dSwitchboard((16, 16), (4, 4), (4, 4), 1)
    sb1 = N.Rectangular2dSwitchboard((4, 4), (2, 1), (2, 1), 13)

    def ig(d_in, k, q):
        ex = N.GeneralExpansionNode(FUNCS, d_in)
        pca = helpers.rand_pca(rng, d_in, q)
        pca.avg = np.zeros_like(pca.avg)
        return N.iGSFANode(rng.normal(size=d_in), ex, helpers.rand_sfa(rng, ex.output_dim, k, N.GSFANode), rng.uniform(0.5, 2.0, size=k),
                           N.LinearRegressionNode(rng.normal(size=(k + 1, d_in)) / np.sqrt(k + 1)), pca, k)

    return [sb0, _layer(rng, 16, 16, 13, 13), sb1, N.Layer([ig(26, 6, 12) for _ in range(8)])]


# refused: (net, environment of the planner, words hg_flow_describe must use on stage 1's line)
REFUSED = {"p21": (lambda: fold_net(13, 21, 17), {}, "not 17..20"),
           "s21": (lambda: fold_net(13, 17, 21), {}, "not 17..20"),
           "no_rem4": (lambda: fold_net(13, 20, 17), {"HIGSFA_NO_REM4": "1"}, "HIGSFA_NO_REM4"),
           "signed_power": (lambda: fold_net(13, 20, 17, funcs1=[N.identity, N.signed_08expo]), {}, "(identity, |x|^p)"),
           "igsfa_layer1": (igsfa_layer1_net, {}, "iGSFA")}


def gpu_net(w0, p1, s1, seed=0):
    """For the device: 64 x 32 pixels, 128 + 64 nodes and a third layer of 32 (more than 16, so layer 1 stores packed remainder
    tiles and the default handle runs k_stage01d), then 16 nodes on top.  16 chunks of 8 first-layer nodes."""
    return fold_net(w0, p1, s1, side=(64, 32), upper=((24, 22), (22, 9)), seed=10 + seed)


GPU_NETS = {"w13_p20_s17": lambda: gpu_net(13, 20, 17), "w16_p17_s20": lambda: gpu_net(16, 17, 20, seed=1)}


def build_driver(exe, extra_flags=()):
    """tests/fold01_plan_driver.cpp with plain g++ against hg_tree.cpp and hg_fused_plan.cpp only.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "fold01_plan_driver.cpp"), os.path.join(CSRC, "hg_tree.cpp"),
           os.path.join(CSRC, "hg_fused_plan.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
