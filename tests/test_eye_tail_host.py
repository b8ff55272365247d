"""CPU: what tests/test_eye_tail_gpu.py assumes about its cases (tests/eye_tail_cases.py), and a negative control for its reading of
k_eyes_glue's chunked compaction — a numpy model of it with two planted faults, on a keep pattern of the accept-all case's shape."""
import numpy as np

from tests import eye_tail_cases as TC
from tests import eyes_restate as ER


def test_window_counts_of_the_frames():
    assert TC.n_windows(TC.B_FRAME, TC.B_SF) == TC.B_WINDOWS and 1100 <= TC.B_WINDOWS <= 2500
    assert tuple(TC.n_windows(s, TC.B_SF) for s in TC.C_LIST) == TC.C_LIST_WINDOWS
    assert TC.C_LIST_WINDOWS[0] > TC.CHUNK and TC.C_LIST_WINDOWS[1] < TC.SMALL_ROWS < TC.C_LIST_WINDOWS[2]
    assert TC.n_windows(TC.D_FRAME, TC.D_SF) == TC.D_WINDOWS
    assert TC.A_SIZES == (1, TC.CHUNK - 1, TC.CHUNK, TC.CHUNK + 1, 2 * TC.CHUNK + 1, 4 * TC.CHUNK + 1) and TC.A_N == TC.A_SIZES[-1]
    # the stream set: more than one chunk of tracked windows in the pooled pass, less than one in every tracker of its own
    assert TC.CHUNK < 9 * TC.S_STREAMS * TC.S_FACES <= TC.MAX_STREAM_WINDOWS and 9 * TC.S_FACES < TC.CHUNK
    assert TC.n_windows(TC.S_FRAME, TC.S_SF) >= 4 * TC.S_FACES


def test_faces_of_the_locate_case_mix_every_kind_in_every_chunk():
    boxes, angles = TC.locate_faces()
    assert boxes.shape == (TC.A_N, 4) and angles.shape == (TC.A_N,)
    w = TC.A_FRAME[0]
    for lo in range(0, TC.A_N - 1, TC.CHUNK):
        b, a = boxes[lo:lo + TC.CHUNK], angles[lo:lo + TC.CHUNK]
        assert (b[:, 0] < 0).sum() >= 40 and (b[:, 2] > w).sum() >= 20, lo
        for v in (0.0, 90.0, -90.0, 180.0):
            assert (a == v).sum() >= 30, (lo, v)
        assert ((a != 0.0) & (np.abs(a) <= 22.5)).sum() >= 500, lo


def test_discard_labels_sit_on_the_tolerance():
    assert TC.JUST_INSIDE < TC.TOLERANCE and np.nextafter(TC.JUST_INSIDE, np.inf) == TC.TOLERANCE
    assert len(TC.D_CASES) == 8 and sum(far for _, _, far in TC.D_CASES) == 4
    for x, y, far in TC.D_CASES:
        reg = np.array([[x, x], [y, y]])
        got = ER.shift_eyes(ER.all_eye_boxes([[0.0, 0.0, 31.0, 31.0]], [0.0]), [0.0], reg, regression_size=TC.REG_SIZE)[1]
        assert bool(got[0]) is far and (max(abs(x), abs(y)) >= TC.TOLERANCE) is far


def test_crafted_patches_contain_the_four_kinds():
    """Per eye size and target pair, by the restatement: a patch of std 0 whose output is target_mean everywhere, one clipped at 0, one
    clipped at 255, an all-zero one; and the 24 x 20 size is no multiple of the contrast kernel's 256 threads."""
    frames = TC.contrast_frames()
    boxes, angles = TC.contrast_faces()
    assert (24 * 20) % 256 != 0 and (24, 20) in TC.E_EYE_SIZES
    for size in TC.E_EYE_SIZES:
        u8 = {name: TC.host_patches(f, boxes, angles, size) for name, f in frames.items()}
        for target in TC.E_TARGETS:
            kinds = np.sum([TC.patch_kinds(p, target) for p in u8.values()], axis=0)
            assert (kinds > 0).all(), (size, target, kinds)
        # what each crafted frame is there for
        assert TC.patch_kinds(u8["const255"], TC.CONTRAST)[0] > 0 and TC.patch_kinds(u8["const0"], TC.CONTRAST)[3] == len(u8["const0"])
        assert TC.patch_kinds(u8["black_dots"], TC.CONTRAST)[2] > 0 and TC.patch_kinds(u8["white_holes"], TC.CONTRAST)[1] > 0
        two = [p for p in u8["const128"] if len(np.unique(p)) == 2]
        assert len(two) > 0 and all(set(np.unique(p)) == {0, 128} for p in two)
        assert any(set(np.unique(p)) == {127, 128} for p in u8["split127_128"])
        assert any(p.min() >= 250 and len(np.unique(p)) > 2 for p in u8["noise250_256"])
        assert any(p.min() >= 100 and p.max() < 110 and len(np.unique(p)) > 2 for p in u8["noise100_110"])


def test_fixture_patches_are_small_and_distinct():
    for size in ((16, 16), (24, 20)):
        p = TC.fixture_patches(size)
        assert p.dtype == np.uint8 and p.shape[1] == size[0] * size[1] and 20 <= len(p) <= 400
        assert (np.sum([TC.patch_kinds(p, t) for t in TC.F_TARGETS], axis=0) > 0).all()
    assert TC.fixture_patches((64, 64)).shape == (2, 4096)


def test_chunked_compaction_model_and_its_planted_faults():
    """The model without a fault is numpy's boolean compaction at every chunk size.  With the base not carried, the second chunk's rows
    land on the first's; with the last partial chunk skipped, its rows are missing: both change the rows of a pattern of the accept-all
    case's shape, which keeps and discards faces on both sides of 1024.  Patterns that would let a fault through: one chunk only (no
    base to carry), nothing kept below 1024 (the carried base is 0 either way), nothing kept in the partial chunk (skipping it loses
    nothing) — so the GPU case asserts kept and discarded faces on both sides of the edge."""
    keep = TC.keep_pattern()
    n = len(keep)
    assert n == TC.B_WINDOWS and n % TC.CHUNK != 0 and n > 2 * TC.CHUNK
    assert (~keep[:TC.CHUNK]).any() and keep[:TC.CHUNK].any() and (~keep[TC.CHUNK:]).any() and keep[TC.CHUNK:].any()
    want = np.nonzero(keep)[0]
    src, count = TC.chunked_compaction(keep)
    assert count == len(want) and np.array_equal(src[:count], want) and (src[count:] == -1).all()
    for chunk in (1, 7, 64, n, n + 5):
        s, c = TC.chunked_compaction(keep, chunk)
        assert c == len(want) and np.array_equal(s[:c], want)
    for fault in ("base", "tail"):
        s, c = TC.chunked_compaction(keep, fault=fault)
        assert c != count and not np.array_equal(s[:count], want), fault

    def shows(pattern, fault):
        good, bad = TC.chunked_compaction(pattern), TC.chunked_compaction(pattern, fault=fault)
        return good[1] != bad[1] or not np.array_equal(good[0], bad[0])
    assert not shows(keep[:300], "base") and not shows(keep[:TC.CHUNK], "base") and not shows(keep[:TC.CHUNK], "tail")
    none_below = keep.copy()
    none_below[:TC.CHUNK] = False
    assert not shows(none_below[:TC.CHUNK + 500], "base") and shows(none_below, "base")      # the third chunk lands on the second's rows
    none_in_tail = keep.copy()
    none_in_tail[2 * TC.CHUNK:] = False
    assert not shows(none_in_tail, "tail") and shows(none_in_tail, "base")
