"""The net of the summed-link tests (tests/test_pair_plan_host.py on the CPU, tests/test_pair_gpu.py on the device) and the
stand-alone driver that prints the planner's pair tables without a device (tests/pair_plan_driver.cpp).  Untrained: every weight is
a seeded draw, as in tests/hoist_cases.py."""
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import hoist_cases
from tests.plan_cases import CSRC, ROOT

# children of the six nodes of layer 3 and of the three of layer 4, in first-read order: neither ascending nor adjacent, and
# descending inside some pairs
GROUPS_3 = [[7, 2], [0, 11], [5, 4], [9, 1], [3, 10], [6, 8]]
GROUPS_4 = [[4, 1], [0, 5], [3, 2]]


def three_pair_net(seed=0):
    """16 x 12 input; 48 nodes on 2x2 fields, 24 nodes of 60 outputs, then three layers of 60 -> 60 nodes with two children each:
    12 nodes on 1x2 merges (a hoisted layer that reads layer 1's partial tiles: the two-children input form), six nodes on
    GROUPS_3 and three on GROUPS_4 through permuting switchboards.  Fused stages 2, 3 and 4 are hoisted, all three of 4 x 4 tiles
    with the (identity, |x|^0.8) expansion; the links 2 -> 3 and 3 -> 4 can be stored summed — a summed link below a summed link,
    so stage 3 both reads and writes the summed form — and 1 -> 2 cannot (its producer multiplies)."""
    rng = np.random.default_rng(4800 + seed)
    sb0 = N.Rectangular2dSwitchboard((16, 12), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((8, 6), (2, 1), (2, 1), 6)
    sb2 = N.Rectangular2dSwitchboard((4, 6), (1, 2), (1, 2), 60)
    sb3 = hoist_cases.grouped_board(rng, [60] * 12, GROUPS_3)
    sb4 = hoist_cases.grouped_board(rng, [60] * 6, GROUPS_4)
    layer = hoist_cases._layer
    return [sb0, layer(rng, 48, 4, 4, 6), sb1, layer(rng, 24, 12, 30, 60), sb2, layer(rng, 12, 120, 60, 60), sb3, layer(rng, 6, 120, 60, 60),
            sb4, layer(rng, 3, 120, 60, 60)]


def build_driver(exe, extra_flags=()):
    """tests/pair_plan_driver.cpp with plain g++ against hg_tree.cpp and hg_fused_plan.cpp only.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "pair_plan_driver.cpp"), os.path.join(CSRC, "hg_tree.cpp"),
           os.path.join(CSRC, "hg_fused_plan.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
