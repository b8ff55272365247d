"""Nets, rows and planner switches of tests/test_visit_waits_gpu.py: the node-group sweep, whose k_stage visits no
longer wait for their own stores (packed35 runs both of its loop forms); the hoisted kernels k_stage_sum and k_stage_sum_pair, where
the same change measured slower and was not kept, run the other three nets.  Untrained: every weight is a seeded draw.

The sweep takes two tiles per wave (the instantiations the flagship runs, and the only ones in which a wave can hold a tile that does
not exist and store its first tile twice) only from 8 x 2 tiles per workgroup with 256 workgroups to fill: BIG gives, per net, an odd
tile count that reaches it, next to the small ROWS, which all run one tile per wave."""
import numpy as np

from pyfaceanalysis_amd import nodes as N
from tests import fold01_cases, hoist_cases, pair_cases

SWEEP_ONLY = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0"}
ROWS = (1, 16, 17, 33, 49, 81)          # 1, 1, 2, 3, 4 and 6 tiles
N_ALL = 81
SENTINEL = -12345.5


def packed35_net():
    """64 x 40 pixels: 160 + 80 front-kernel nodes (layer 1: 17 outputs, packed remainder rows), 40 nodes of 35 -> 35 on pairs of them
    (3 x 3 tiles with a remainder tile, three K-blocks of which the middle one is the children's shared packed block: the
    whole-visit-prefetch form of k_stage, packed remainder output because 20 > 16 nodes read it) and 20 nodes of 60 -> 60 (4 x 4
    tiles, the streaming form; a 35-wide child is not hoisted)."""
    return fold01_cases.fold_net(13, 20, 17, side=(64, 40), upper=((35, 35), (60, 60)), seed=20)


def _kids_net(field, seed):
    rng = np.random.default_rng(4900 + seed)
    sb0 = N.Rectangular2dSwitchboard((12, 12), (2, 2), (2, 2), 1)
    sb1 = N.Rectangular2dSwitchboard((6, 6), (2, 1), (2, 1), 6)
    sb2 = N.Rectangular2dSwitchboard((3, 6), field, field, 60)
    layer = hoist_cases._layer
    return [sb0, layer(rng, 36, 4, 4, 6), sb1, layer(rng, 18, 12, 30, 60), sb2,
            layer(rng, sb2.output_channels, sb2.out_channel_dim, 60, 60)]


def kids3_net():
    """12 x 12 input, 36 and 18 nodes, then six hoisted 60 -> 60 nodes of three children each (k_stage_sum with a child loop of two
    trips)."""
    return _kids_net((3, 1), 0)


def kids2_net():
    """The same with nine hoisted nodes of two children each."""
    return _kids_net((1, 2), 1)


# name -> (net, planner switches of the sweep handle, rows of the two-tiles-per-wave call: an odd tile count)
#   pairs: the three-pair net as tests/test_pair_gpu.py plans it (k_stage_sum_pair on both input forms, k_stage_sum on a summed input)
#   packed35: 209 tiles in 14 tile groups x 20 node groups (layers 2 and 3)
#   kids3: node groups of one (every visit wraps to the group's first node), 673 tiles in 43 tile groups x 6
#   kids2: node groups of two and a last one short, 833 tiles in 53 tile groups x 5
NETS = {"pairs": (pair_cases.three_pair_net, dict(SWEEP_ONLY, HIGSFA_SUM_LDS="128", HIGSFA_PAIR_WGS="1"), None),
        "packed35": (packed35_net, SWEEP_ONLY, 209 * 16 - 15),
        "kids3": (kids3_net, dict(SWEEP_ONLY, HIGSFA_SUM_LDS="32"), 673 * 16 - 15),
        "kids2": (kids2_net, dict(SWEEP_ONLY, HIGSFA_SUM_LDS="64"), 833 * 16 - 15)}
