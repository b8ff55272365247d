"""Flows for the tests of the folded link's packed one-row k-steps (FusedOptions::fold01_pack; tests/test_fold01_pack_plan_host.py on the
CPU, tests/test_fold01_pack_gpu.py on the device) and the stand-alone driver that plans them without a device
(tests/fold01_pack_plan_driver.cpp).  The nets are those of tests/fold01_cases.py, whose layer-0 nodes of 13 outputs are packed and
whose nodes of 16 are not, and three of their own:

  * two_affine_net: layer 0's first affine is a chain of two (whitening 16 -> 14, PCA 14 -> 13 with a nonzero mean), so its composed
    first bias is NOT zero and the repeated bias entry of feature 12 can be told from padding;
  * probe_net: every row of the layer-0 second affines except the two of feature 12 (identity and power) is zero, hence every row of
    F_c except (c, function, 12): layer 1's first affine is its folded bias plus the packed k-step ALONE, and a lane-group or child
    mix-up there shows at the order of the node's output, not in its last bits;
  * widths 12 and 14, which are refused."""
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import fold01_cases, helpers, plan_cases
from tests.plan_cases import CSRC, ROOT

FUNCS = fold01_cases.FUNCS
GOLDEN = os.path.join(ROOT, "tests", "golden", "fold01_pack_off_digests.json")


def two_affine_net(seed=0):
    """fold_net(13, 20, 17) on 16 x 16 pixels with [whitening 16 -> 14, PCA 14 -> 13, expansion, SFA 26 -> 13] in layer 0."""
    flow = fold01_cases.fold_net(13, 20, 17, seed=20 + seed)
    rng = np.random.default_rng(5200 + seed)
    nodes = []
    for fn in flow[1].nodes:
        nodes.append(N.FlowNode([helpers.rand_pca(rng, 16, 14, N.WhiteningNode), helpers.rand_pca(rng, 14, 13)] + list(fn.flow[1:])))
    flow[1] = N.Layer(nodes)
    return flow


def probe_net(seed=0):
    """fold01_cases.gpu_net(13, 20, 17) with the layer-0 second affines zero outside the rows of feature 12 (rows 12 and 25 of 26);
    those two rows are scaled up so that layer 1 still sees inputs of order one."""
    flow = fold01_cases.gpu_net(13, 20, 17, seed=5 + seed)
    for fn in flow[1].nodes:
        sfa = fn.flow[-1]
        keep = np.zeros((26, 1))
        keep[[12, 25]] = 3.0
        sfa.sf = sfa.sf * keep      # (its bias stays as drawn: it goes into the folded bias)
    return flow


HOST_NETS = dict(fold01_cases.HOST_NETS)
HOST_NETS["two_affine"] = two_affine_net
PACKED = ("w13_p20_s17", "w13_p17_s17", "two_affine")      # layer 0 of 13 outputs; the w16 nets fold and do not pack

# refused: (net, driver options, environment, words the note must use)
REFUSED = {"w12": (lambda: fold01_cases.fold_net(12, 20, 17), (), {}, "link 0 -> 1 stays as it is"),
           "w14": (lambda: fold01_cases.fold_net(14, 20, 17), (), {}, "14 outputs, not 13"),
           "w16": (lambda: fold01_cases.fold_net(16, 17, 20), (), {}, "16 outputs, not 13"),
           "fold01_off": (lambda: fold01_cases.fold_net(13, 20, 17), ("--fold", "0"), {}, "fold01 is off"),
           "no_rem4": (lambda: fold01_cases.fold_net(13, 20, 17), (), {"HIGSFA_NO_REM4": "1"}, "link 0 -> 1 stays as it is")}

GPU_NETS = dict(fold01_cases.GPU_NETS)
GPU_NETS["probe"] = probe_net


def digest_flows():
    """{name: flow} whose plans with fold01 on and fold01_pack off are recorded in tests/golden/fold01_pack_off_digests.json: the four fold
    nets, every weight redrawn element by element (plan_cases.reseed: no BLAS result reaches a digest)."""
    return {name: plan_cases.reseed(make(), 300 + i) for i, (name, make) in enumerate(sorted(fold01_cases.HOST_NETS.items()))}


def build_driver(exe, extra_flags=(), csrc=CSRC):
    """tests/fold01_pack_plan_driver.cpp with plain g++ against hg_tree.cpp and hg_fused_plan.cpp only.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "fold01_pack_plan_driver.cpp"), os.path.join(csrc, "hg_tree.cpp"),
           os.path.join(csrc, "hg_fused_plan.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
