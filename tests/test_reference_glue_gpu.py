"""GPU: the device glue against outputs of the reference's own functions (tests/golden/reference_glue.npz, written by
tests/golden/make_reference_glue.py), bit for bit: the single-step cascade update (hg_cascade_update_device, whose arithmetic is
the group launches' update_one) on random candidates and on rows that sit exactly on a discard threshold, among them rows where a
fused multiply-add would decide the other way; the compaction and row gather against a numpy boolean mask; the first-stage grid;
the purge."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from tests.test_reference_glue import STAGES, consts, grid_cases, load, update_case


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STAGES)
def test_single_step_update_equals_reference(native_lib, kind):
    import torch
    g = load()
    c = update_case(g, kind)
    k = _capi.HgCascadeConsts(*consts(g))
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    coords, angles = dev(c["coords"]), dev(c["angles"])
    reg, oidx = dev(c["reg"]), dev(c["oidx"], torch.int32)
    ocoords, oangles, olevel = dev(c["ocoords"]), dev(c["oangles"]), dev(c["olevel"])
    n = len(c["coords"])
    discard = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(native_lib.hg_cascade_update_device(0, _capi.HG_STAGE[kind], C.byref(k), n, _ptr(coords), _ptr(angles), _ptr(reg), _ptr(oidx),
                                                    _ptr(ocoords), _ptr(oangles), _ptr(olevel), _ptr(discard), st))
    torch.cuda.synchronize()
    got_c, got_a, got_w = coords.cpu().numpy(), angles.cpu().numpy(), discard.cpu().numpy()
    bad = np.nonzero((got_c != c["out_coords"]).any(axis=1) | (got_a != c["out_angles"]) | (got_w != c["out_wrong"]))[0]
    assert bad.size == 0, (kind, "rows differing from the reference", [(int(i), "edge" if c["edge"][i] else "random",
                                                                         "fma flip" if c["fma_flips"][i] else "") for i in bad[:12]])
    assert set(np.unique(got_w)) <= {0, 1}


def _keep_masks(n):
    m = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternate": np.arange(n) % 2 == 0, "last": np.zeros(n, bool)}
    if n:
        m["last"][-1] = True
    return m


@pytest.mark.gpu
def test_compact_and_gather_equal_boolean_mask(native_lib):
    """hg_cascade_compact_device (one workgroup of 1024 walking the flags in chunks) + hg_gather_rows_device against numpy's boolean
    mask: counts around the chunk size, four keep patterns, rows of 4 / 12 / 32 / 16388 bytes (16388: 256-thread rows, not a multiple
    of 16; 32: the 16-byte path).  The count is read from device memory; rows past it are left as they were."""
    import torch
    L = native_lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for n in (0, 1, 1023, 1024, 1025, 4097):
        for name, keep in _keep_masks(n).items():
            flags = torch.from_numpy((~keep).astype(np.uint8)).cuda()
            mp = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
            _capi.check(L.hg_cascade_compact_device(0, _ptr(flags) if n else None, n, _ptr(mp), _ptr(cnt), st))
            torch.cuda.synchronize()
            want_idx = np.nonzero(keep)[0]
            k = int(cnt.cpu().item())
            assert k == len(want_idx), (n, name)
            assert np.array_equal(mp.cpu().numpy()[:k], want_idx.astype(np.int32)), (n, name)
            for row_bytes in (4, 12, 32, 16388):
                src = rng.integers(-2 ** 31, 2 ** 31 - 1, (max(n, 1), row_bytes // 4), dtype=np.int64).astype(np.int32)
                s_dev = torch.from_numpy(src).cuda()
                d_dev = torch.full((max(n, 1), row_bytes // 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                _capi.check(L.hg_gather_rows_device(0, _ptr(s_dev), _ptr(d_dev), row_bytes, _ptr(mp), _ptr(cnt), n, st))
                torch.cuda.synchronize()
                d = d_dev.cpu().numpy()
                assert np.array_equal(d[:k], src[:n][keep]), (n, name, row_bytes)
                assert (d[k:] == 0x5A5A5A5A).all(), (n, name, row_bytes)


@pytest.mark.gpu
def test_device_grid_equals_reference_grid(native_lib):
    """hg_cascade_grid_device (numpy.linspace in closed form) against the reference's grid builders: boxes and the per-window
    max_Dx_diff / max_Dy_diff, eight frames, one of them with a single grid point on an axis."""
    import torch
    from pyfaceanalysis_amd.cascade import frame_levels
    for (fw, fh, sf, sub), boxes, level, counts in grid_cases(load()):
        levels, n_levels, n0 = frame_levels(fw, fh, sf, grid.FACE_PIPELINE, sub)
        assert n0 == len(boxes), (fw, fh)
        n = C.c_int64()
        b_dev = torch.empty((n0, 4), dtype=torch.float64, device="cuda")
        l_dev = torch.empty((n0, 3), dtype=torch.float64, device="cuda")
        _capi.check(native_lib.hg_cascade_grid_device(0, levels, n_levels, _ptr(b_dev), _ptr(l_dev), n0, C.byref(n),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert n.value == n0
        assert np.array_equal(b_dev.cpu().numpy(), boxes), (fw, fh, sf, sub)
        assert np.array_equal(l_dev.cpu().numpy()[:, :2], level), (fw, fh, sf, sub)


@pytest.mark.gpu
def test_device_purge_equals_reference(native_lib):
    from pyfaceanalysis_amd.eyes import purge_detections
    g = load()
    for name in g["purge_names"]:
        rows, want = g["purge_%s_in" % name], g["purge_%s_out" % name]
        got = purge_detections(rows)
        assert got.shape == want.shape, name
        if name == "ties":          # the reference's order among exact ties is its unstable sort's (tests/test_reference_glue.py)
            assert np.array_equal(np.unique(got, axis=0), np.unique(want, axis=0)), name
        else:
            assert np.array_equal(got, want, equal_nan=True), name
