"""Shared by tests/test_stream_set_host.py and tests/test_stream_set_gpu.py: the numbers of a stream set's refusals, and the harness
that steps a ``tracking.StreamSetTracker`` beside its oracle — one ``tracking.FaceTracker`` per stream, on a cascade and an eye handle of
their own, fed the same frames — and compares every stream's dict with ``array_equal`` ("Tracking over a stream set": rows
are independent, the HIP path is bit-identical across batch sizes, every compaction keeps row order, the purge and the hand-over are per
stream — so no tolerance is needed)."""
import numpy as np

N_TRACKED = 9
MAX_STREAM_WINDOWS = 8192          # include/higsfa.h HG_MAX_STREAM_WINDOWS = 2 * kChunk
MAX_STACK_FRAMES = 1024
MAX_FACES_CAP = 64

# (n_streams, max_faces, rescan_every, the word of the message): refused by hg_stream_tracker_create before any handle is looked at
BAD_SETS = ((0, 1, 0, "n_streams"), (-1, 1, 0, "n_streams"), (MAX_STACK_FRAMES + 1, 1, 0, "n_streams"), (1, 0, 0, "max_faces"), (1, -2, 0, "max_faces"),
            (1, MAX_FACES_CAP + 1, 0, "max_faces"), (1 << 20, 1 << 20, 0, "n_streams"), (15, 61, 0, "windows"), (911, 1, 0, "windows"), (114, 8, 0, "windows"),
            (1, 1, -1, "rescan_every"), (16, 8, -7, "rescan_every"))
# in range: 9 * 910 * 1 = 8190 and 9 * 113 * 8 = 8136 are the last products under the bound for those face counts
GOOD_SETS = ((1, 1, 0), (16, 8, 2), (910, 1, 0), (14, 64, 0), (113, 8, 1), (128, 7, 0))

STEP_KEYS = ("faces", "tracked", "n_windows", "n_before_purge", "slots", "n_held")


def assert_cases_consistent():
    for b, k, r, word in BAD_SETS:
        numbers_bad = not 1 <= b <= MAX_STACK_FRAMES or not 1 <= k <= MAX_FACES_CAP
        assert numbers_bad or N_TRACKED * b * k > MAX_STREAM_WINDOWS or r < 0, (b, k, r)
        if word == "windows":
            assert not numbers_bad and N_TRACKED * b * k > MAX_STREAM_WINDOWS
    for b, k, r in GOOD_SETS:
        assert 1 <= b <= MAX_STACK_FRAMES and 1 <= k <= MAX_FACES_CAP and N_TRACKED * b * k <= MAX_STREAM_WINDOWS and r >= 0
    assert N_TRACKED * 910 * 1 <= MAX_STREAM_WINDOWS < N_TRACKED * 911 * 1 and N_TRACKED * 113 * 8 <= MAX_STREAM_WINDOWS < N_TRACKED * 114 * 8


class Pair(object):
    """A stream set on (dc, loc) and its oracle, one FaceTracker per stream on (odc, oloc)."""

    def __init__(self, dc, loc, odc, oloc, n_streams, smallest_face, **kw):
        from pyfaceanalysis_amd.tracking import FaceTracker, StreamSetTracker
        self.n = n_streams
        self.multi = kw.get("max_faces", 1) != 1 or kw.get("rescan_every", 0) != 0      # whether FaceTracker returns slots and n_held
        self.set = StreamSetTracker(dc, loc, n_streams, smallest_face=smallest_face, **kw)
        self.oracle = [FaceTracker(odc, oloc, smallest_face=smallest_face, **kw) for _ in range(n_streams)]
        self.log = []

    def step(self, frames, what, oracle_frames=None):
        """One step of the set on ``frames`` and of every oracle tracker on its frame (``oracle_frames``: the same pictures in another
        layout); every stream compared key for key.  Returns the set's result."""
        got = self.set.step(frames)
        want = [tr.step((frames if oracle_frames is None else oracle_frames)[s]) for s, tr in enumerate(self.oracle)]
        assert sorted(got) == ["n_grid", "n_tracked", "rows_executed", "streams"] and len(got["streams"]) == self.n, what
        for s, (g, w) in enumerate(zip(got["streams"], want)):
            assert sorted(g) == sorted(STEP_KEYS), (what, s)
            assert g["tracked"] is w["tracked"], (what, s, g["tracked"], w["tracked"])
            assert g["faces"].shape == w["faces"].shape and g["faces"].dtype == np.float64 and np.array_equal(g["faces"], w["faces"], equal_nan=True), (what, s)
            assert g["faces"].tobytes() == w["faces"].tobytes(), (what, s)
            assert g["n_windows"] == w["n_windows"] and g["n_before_purge"] == w["n_before_purge"], (what, s, g["n_windows"], w["n_windows"])
            held = self.oracle[s].tracked_faces
            assert np.array_equal(self.set.tracked_faces(s), held) and g["n_held"] == len(held), (what, s)
            assert g["slots"].dtype == np.int32 and g["slots"].shape == (len(g["faces"]),), (what, s)
            if self.multi:
                assert np.array_equal(g["slots"], w["slots"]) and g["n_held"] == w["n_held"], (what, s, g["slots"], w["slots"])
            else:      # max_faces = 1, rescan_every = 0: FaceTracker returns neither; one face held, so every tracked row's slot is 0
                assert "slots" not in w and (g["slots"] == (0 if g["tracked"] else -1)).all(), (what, s)
        assert got["n_tracked"] == sum(w["tracked"] for w in want) and got["n_grid"] == self.n - got["n_tracked"], what
        assert got["rows_executed"] == sum(w["rows_executed"] for w in want), (what, got["rows_executed"], [w["rows_executed"] for w in want])
        self.log.append(got)
        return got

    def reset(self, s=None):
        self.set.reset(s)
        for i, tr in enumerate(self.oracle):
            if s is None or i == s:
                tr.reset()
        for i in range(self.n):
            assert np.array_equal(self.set.tracked_faces(i), self.oracle[i].tracked_faces), i

    def flags(self):
        return [[st["tracked"] for st in g["streams"]] for g in self.log]

    def close(self):
        self.set.close()
        for tr in self.oracle:
            tr.close()
