"""GPU: pitched frames and ROI views (``ld != frame_w``) through every frame-reading entry — the patcher's device and host entries, the
cascade's four detect entries, the eye step and the tracker — and three neighbouring edges of the same kernels: more than 65535
boxes, an output row stride / output pointer that defeats the vector stores, frames narrower than one 8-byte load.

Pixels are compared with PIL called here (``array_equal``), the cascade with the host-composed loop on the contiguous numpy frame
(tests/test_filters_gpu.py ``Rig.composed_loop``).  On top of that every result must be the same, bit for bit, for the dense frame
and for the same frame seen through a pitched buffer or a crop of a larger one, whatever surrounds it, and the call must leave
the whole buffer as it was.  No tolerance anywhere.

Which kernel branch a case reaches (hg_extract.hip):

  k_extent_gather          NEAREST unrotated (37, 21) scalar, (48, 5) four pixels per thread with the table read entry by entry
                           ((w + h) & 3 != 0); every float output and every float32 frame; ``ldo = w*h + 1`` or an output pointer off by
                           3 bytes sends (16, 12) / (64, 64) here too, scalar; ``ldo = w*h + 4`` the four-pixel path with 16-byte table reads
  k_extent_gather_u8x16    (16, 12) one thread per row, (32, 12) two, (64, 64) four.  A window at most twice as wide as its output, inside
                           the frame in x and ending at least 8 pixels left of the frame's right edge, takes the 8-byte loads (the inside
                           boxes of FC.boxes() but those at the right edge, the boxes over the top / bottom edge, the magnified ones), at
                           every row alignment the layouts give; the boxes over the left / right edge, the outside boxes and the 8 x
                           shrinking boxes take the byte branch (``takes_8_byte_loads`` restates the choice and the tests assert that
                           both happen).  The narrow frames decide ``x0 + 8 <= fw`` at fw = 7, 8 and 9
  k_extent_gather_rot      (16, 12) and (64, 64) sixteen pixels per thread (180 degrees: PIL's scaling branch, four pixels); (16, 7) table
                           rows not 16-byte aligned; (37, 21) scalar; float output scalar; ``ldo = w*h + 4`` sixteen-pixel rows for even
                           boxes and four-pixel rows for odd ones
  k_filter_gather          BILINEAR / BICUBIC unrotated (64, 64)
  k_filter_gather_rot      corner boxes: the staged tile; boxes 20 and 23 of FC.boxes() (8 x shrunk): tap by tap; (20, 12) has partial
                           tiles, (64, 64) sixteen tiles per window; 65568 boxes: the barrier loop takes a second trip in 33 rows of
                           workgroups only
"""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from tests import eyes_restate as ER
from tests import filters_cases as FC
from tests.test_filters_gpu import CONTRAST, FORMATS, SF, SUB, Rig, assert_same_detection, composed_faces

pytestmark = pytest.mark.gpu

DT = {np.uint8: _capi.HG_U8, np.float32: _capi.HG_F32, np.float64: _capi.HG_F64}
FILLS = (9101, 9102)                                  # two different surroundings for every non-dense layout
LAYOUTS = ("dense", "pad1", "pad_al", "roi")


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def layout_geometry(name, H, W):
    """(buffer shape, row offset, column offset) of a layout whose view [y0:y0 + H, x0:x0 + W] is the frame."""
    if name == "dense":
        return (H, W), 0, 0
    if name == "pad1":                                # odd pitch for the frames used here: rows at every byte alignment
        return (H, W + 1), 0, 0
    if name == "pad_al":                              # aligned rows, long padding
        return (H, ((W + 8) // 64 + 1) * 64), 0, 0
    if name == "roi":                                 # foreign bytes on all four sides; the view starts 3 * (W + 24) + 13 bytes in
        return (H + 5, W + 24), 3, 13
    raise KeyError(name)


def host_layout(f, name, seed):
    """(buffer, view) on the host: the buffer is seeded noise, never 0 (0 is the kernels' own fill for pixels outside the frame), the view
    holds ``f``."""
    H, W = f.shape
    shape, y0, x0 = layout_geometry(name, H, W)
    noise = np.random.default_rng(seed).integers(1, 256, shape)
    buf = noise.astype(np.uint8) if f.dtype == np.uint8 else (noise.astype(np.float32) * np.float32(0.75))
    assert buf.dtype == f.dtype and buf.min() > 0 and (buf.size < 16 or len(np.unique(buf)) > 1)
    buf[y0:y0 + H, x0:x0 + W] = f
    return buf, buf[y0:y0 + H, x0:x0 + W]


class DevLayout(object):
    def __init__(self, f, name, seed):
        import torch
        self.name, self.seed = name, seed
        self.buf, hview = host_layout(f, name, seed)
        self.dev = torch.from_numpy(self.buf).cuda()
        H, W = f.shape
        _, y0, x0 = layout_geometry(name, H, W)
        self.view = self.dev[y0:y0 + H, x0:x0 + W]
        self.f = f
        assert self.view.stride(1) == 1 and self.view.stride(0) == self.buf.shape[1] and tuple(self.view.shape) == f.shape

    def assert_untouched(self):
        """The view still holds the frame and the bytes outside it are what they were."""
        after = self.dev.cpu().numpy()
        assert np.array_equal(self.view.cpu().numpy(), self.f), (self.name, "the frame changed")
        assert np.array_equal(after, self.buf), (self.name, "bytes outside the view changed")

    def __repr__(self):
        return "%s/%d" % (self.name, self.seed)


def layouts(f, names=LAYOUTS):
    """dense first, then every other layout with both fills."""
    return [DevLayout(f, n, s) for n in names for s in (FILLS if n != "dense" else FILLS[:1])]


def assert_layout_invariant(lays, run, equal=np.array_equal):
    """run(view) on every layout: the dense result is returned; every other one equals it, and no buffer was written to."""
    assert lays[0].name == "dense"
    first = run(lays[0].view)
    lays[0].assert_untouched()
    for lay in lays[1:]:
        got = run(lay.view)
        assert equal(got, first), (lay, "differs from the dense frame's result")
        lay.assert_untouched()
    return first


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pt(native_lib):
    from pyfaceanalysis_amd.patches import Patcher
    p = Patcher()
    yield p
    p.close()


@pytest.fixture(scope="module")
def rig(native_lib, nets, pt):
    r = Rig(nets, pt)
    yield r
    r.close()


@pytest.fixture(scope="module")
def small(native_lib):
    """The 53 x 37 frame in every layout, uint8 and float32 (x 0.5: values no uint8 holds), made once."""
    f8 = FC.frame()
    f32 = f8.astype(np.float32) * np.float32(0.5)
    return {np.uint8: layouts(f8), np.float32: layouts(f32)}


_PIL = {}


def pil_ref(boxes, angs, size, filt):
    """FC.pil_windows of FC.frame(), computed once per case and shared (read only)."""
    key = (boxes.tobytes(), angs.tobytes(), size, filt)
    if key not in _PIL:
        _PIL[key] = FC.pil_windows(FC.frame(), boxes, angs, size, filt)
        _PIL[key].setflags(write=False)
    return _PIL[key]


def cut(pt, view, boxes, size, out_dt=np.uint8, angs=None, filt=0):
    """Patcher.extract_device on a frame view with its own row stride; the output is pre-filled, so a pixel never written shows."""
    import torch
    w, h = size
    n = len(boxes)
    fdt = np.uint8 if view.dtype == torch.uint8 else np.float32
    bdev = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float64)).cuda()
    adev = None if angs is None else torch.from_numpy(np.ascontiguousarray(angs, dtype=np.float64)).cuda()
    odev = torch.full((n, w * h), 7, dtype=getattr(torch, np.dtype(out_dt).name), device="cuda")
    pt.extract_device(view.data_ptr(), fdt, view.shape[0], view.shape[1], view.stride(0), bdev.data_ptr(), n, size, odev.data_ptr(), out_dt, w * h,
                      stream=torch.cuda.current_stream().cuda_stream, delta_angs_ptr=None if adev is None else adev.data_ptr(), interpolation=filt)
    torch.cuda.synchronize()
    return odev.cpu().numpy()


def takes_8_byte_loads(box, w, fw):
    """The choice k_extent_gather_u8x16 makes for a window (for all its waves: every group of four columns qualifies): the four source
    columns of a group inside the frame, ascending within 8 bytes of the first, and the 8 bytes end inside the row.  Only used to
    assert that a case reaches the branch it is there for."""
    a = (box[2] - box[0]) / w
    o, xs = box[0] + a * 0.5, []
    for _ in range(w):
        v = -1 if o < 0 else int(o)
        xs.append(v if v < fw else -1)
        o += a
    return all(g[0] >= 0 and all(g[0] <= x < g[0] + 8 for x in g[1:]) and g[0] + 8 <= fw for g in (xs[i:i + 4] for i in range(0, w, 4)))


def all_boxes():
    return np.concatenate([FC.boxes(), FC.corner_boxes()])


def over_angles(boxes, angles=FC.ANGLES):
    return np.repeat(boxes, len(angles), axis=0), np.tile(np.array(angles, dtype=np.float64), len(boxes))


# ---- 1. patcher, device entry, against PIL -------------------------------------------------------------------------------------
def test_layouts_are_what_they_claim(small):
    lays = {(l.name, l.seed): l for l in small[np.uint8]}
    assert [l.name for l in small[np.uint8]] == ["dense", "pad1", "pad1", "pad_al", "pad_al", "roi", "roi"]
    assert lays["pad1", FILLS[0]].view.stride(0) == 54 and lays["pad_al", FILLS[0]].view.stride(0) == 64 and lays["roi", FILLS[0]].view.stride(0) == 77
    assert lays["pad_al", FILLS[0]].view.data_ptr() % 64 == 0
    roi = lays["roi", FILLS[0]]
    assert roi.view.data_ptr() - roi.dev.data_ptr() == 3 * 77 + 13 and roi.view.data_ptr() % 8 != 0
    # the 160-pixel frame's crop starts at an odd address; an odd pitch walks the rows through every alignment of an 8-byte load
    assert (3 * (160 + 24) + 13) % 2 == 1 and {(r * 77) % 8 for r in range(37)} == set(range(8))
    for a, b in ((lays["pad1", FILLS[0]], lays["pad1", FILLS[1]]), (lays["roi", FILLS[0]], lays["roi", FILLS[1]])):
        assert not np.array_equal(a.buf, b.buf) and np.array_equal(a.view.cpu().numpy(), b.view.cpu().numpy())


@pytest.mark.parametrize("size", [(16, 12), (32, 12), (64, 64), (37, 21), (48, 5)])
def test_nearest_unrotated_windows(pt, small, size):
    """(16, 12), (32, 12), (64, 64): k_extent_gather_u8x16 with one, two and four threads per row.  The "inside" boxes of FC.boxes() are
    at most 22 pixels wide, so the four columns of a group lie within 8 bytes: they take the 8-byte-load branch unless they end within 8
    pixels of the right edge (so do the boxes over the top / bottom edge and the magnified ones); the boxes over the left / right edge,
    the outside boxes and the 8 x shrinking boxes take the byte branch.  (37, 21) is k_extent_gather's scalar path, (48, 5) its
    four-pixel path with an unaligned table row.  Float outputs: k_extent_gather."""
    boxes = all_boxes()
    want = pil_ref(boxes, np.zeros(len(boxes)), size, 0)
    assert want[:14].any(axis=1).all() and not want[14:16].any()
    if size[0] % 16 == 0 and size != (48, 5):
        wide = [i for i, b in enumerate(boxes) if takes_8_byte_loads(b, size[0], FC.FRAME_W)]
        assert {0, 2, 4, 5} <= set(wide) and not set(wide) & {6, 7, 8, 9, 14, 15, 20, 21, 22, 23}, wide
    for dt in ((np.uint8, np.float32, np.float64) if size in ((16, 12), (37, 21)) else (np.uint8,)):
        got = assert_layout_invariant(small[np.uint8], lambda v: cut(pt, v, boxes, size, dt))
        assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (size, dt, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("size", [(16, 12), (37, 21)])
def test_nearest_from_a_float32_frame(pt, small, size):
    boxes = all_boxes()
    want = pil_ref(boxes, np.zeros(len(boxes)), size, 0)
    for dt in (np.float32, np.float64):
        got = assert_layout_invariant(small[np.float32], lambda v: cut(pt, v, boxes, size, dt))
        assert got.dtype == dt and np.array_equal(got, want.astype(dt) * 0.5) and (got % 1 == 0.5).any()


@pytest.mark.parametrize("size", [(16, 12), (64, 64), (16, 7), (37, 21)])
def test_nearest_rotated_windows(pt, small, size):
    """(16, 12), (64, 64): the sixteen-pixel path of k_extent_gather_rot (``off = ys * ld + xs``); 180 degrees is PIL's scaling branch
    and takes the four-pixel path; (16, 7): table rows of 23 entries, not 16-byte aligned; (37, 21): scalar."""
    bb, aa = over_angles(all_boxes())
    want = pil_ref(bb, aa, size, 0)
    got = assert_layout_invariant(small[np.uint8], lambda v: cut(pt, v, bb, size, np.uint8, angs=aa))
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (size, len(bad), [(bb[i], aa[i], j) for i, j in bad[:3]])
    assert want.any() and (want == 0).sum() > 500             # the rotation's zero fill is in there
    if size == (16, 12):                                      # one float64 case from the float32 frame
        gotf = assert_layout_invariant(small[np.float32], lambda v: cut(pt, v, bb, size, np.float64, angs=aa))
        assert gotf.dtype == np.float64 and np.array_equal(gotf, want.astype(np.float64) * 0.5)


@pytest.mark.parametrize("size", [(20, 12), (64, 64)])
@pytest.mark.parametrize("filt", FC.FILTERS)
def test_filtered_rotated_windows(pt, small, filt, size):
    """The boxes and angles of test_filters_gpu.test_rotated_windows_equal_pil: corner boxes (staged tiles; the rotation's zero fill is in
    the taps) and boxes [0, 7, 17, 20, 23] (20 and 23 shrink about 8 x: tap by tap)."""
    boxes = np.concatenate([FC.corner_boxes(), FC.boxes()[[0, 7, 17, 20, 23]]])
    bb, aa = over_angles(boxes, FC.ANGLES if size != (64, 64) else (17.0, -135.0))
    want = pil_ref(bb, aa, size, filt)
    got = assert_layout_invariant(small[np.uint8], lambda v: cut(pt, v, bb, size, np.uint8, angs=aa, filt=filt))
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (size, filt, len(bad), [(bb[i], aa[i], j) for i, j in bad[:3]])
    assert want.any() and (want == 0).any()


@pytest.mark.parametrize("filt", FC.FILTERS)
def test_filtered_unrotated_windows_64(pt, small, filt):
    boxes = all_boxes()
    want = pil_ref(boxes, np.zeros(len(boxes)), (64, 64), filt)
    got = assert_layout_invariant(small[np.uint8], lambda v: cut(pt, v, boxes, (64, 64), np.uint8, filt=filt))
    assert np.array_equal(got, want) and want[:14].any(axis=1).all()


# ---- 2. patcher, host entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pad1", "roi"])
def test_host_entry_reads_pitched_numpy_views(pt, name):
    """hg_patcher_extract_rotate / hg_patcher_extract_filter with ``ld = view.strides[0]`` (Patcher.extract makes the frame contiguous and
    cannot reach this): the pitched upload of the host entry."""
    L = _capi.lib()
    bb, aa = over_angles(np.concatenate([FC.corner_boxes(), FC.boxes()[[0, 7, 17, 20, 23]]]))
    size = (20, 12)
    for seed in FILLS:
        buf, view = host_layout(FC.frame(), name, seed)
        before = buf.copy()
        assert view.strides == (buf.shape[1], 1) and not view.flags["C_CONTIGUOUS"]
        for filt in (0, 3):
            out = np.full((len(bb), 240), 7, dtype=np.uint8)
            if filt == 0:
                rc = L.hg_patcher_extract_rotate(pt._handle(), view.ctypes.data, _capi.HG_U8, FC.FRAME_H, FC.FRAME_W, view.strides[0], bb.ctypes.data,
                                                 aa.ctypes.data, len(bb), size[0], size[1], out.ctypes.data, _capi.HG_U8, 240)
            else:
                rc = L.hg_patcher_extract_filter(pt._handle(), filt, view.ctypes.data, _capi.HG_U8, FC.FRAME_H, FC.FRAME_W, view.strides[0], bb.ctypes.data,
                                                 aa.ctypes.data, len(bb), size[0], size[1], out.ctypes.data, _capi.HG_U8, 240)
            assert rc == _capi.HG_OK and np.array_equal(out, pil_ref(bb, aa, size, filt)), (name, seed, filt)
        assert np.array_equal(buf, before)


# ---- 3. output stride and unaligned output, NEAREST ----------------------------------------------------------------------------
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("size", [(16, 12), (64, 64)])
def test_output_stride_and_unaligned_output(pt, small, size, rotated):
    """``ldo`` = w*h (the vector stores), w*h + 1 (nothing aligned: scalar stores), w*h + 16 (rows stay 16-byte aligned), and w*h + 4
    (4-byte aligned only: k_extent_gather's packed path; in k_extent_gather_rot every other box falls from the sixteen-pixel to the
    four-pixel path); the output pointer 0 and 3 bytes into a filled buffer.  The windows are PIL's and every other byte keeps its fill."""
    import torch
    w, h = size
    boxes = all_boxes()
    if rotated:
        bb, aa = over_angles(boxes, (17.0, 180.0, -135.0))
    else:
        bb, aa = boxes, np.zeros(len(boxes))
    want = pil_ref(bb, aa, size, 0)
    n = len(bb)
    frame = small[np.uint8][0]
    bdev = torch.from_numpy(bb).cuda()
    adev = torch.from_numpy(aa).cuda() if rotated else None
    st = torch.cuda.current_stream().cuda_stream
    for out_dt, cases in ((np.uint8, [(ldo, off) for ldo in (w * h, w * h + 1, w * h + 4, w * h + 16) for off in (0, 3)]), (np.float32, [(w * h + 1, 0)])):
        for ldo, off in cases:
            fill = np.random.default_rng(9300 + ldo + off).integers(1, 256, off + n * ldo + 64).astype(out_dt)
            big = torch.from_numpy(fill).cuda()
            assert big.data_ptr() % 256 == 0
            pt.extract_device(frame.view.data_ptr(), np.uint8, FC.FRAME_H, FC.FRAME_W, FC.FRAME_W, bdev.data_ptr(), n, size,
                              big.data_ptr() + off * fill.itemsize, out_dt, ldo, stream=st, delta_angs_ptr=adev.data_ptr() if rotated else None)
            torch.cuda.synchronize()
            after = big.cpu().numpy()
            rows = after[off:off + n * ldo].reshape(n, ldo)
            assert np.array_equal(rows[:, :w * h], want.astype(out_dt)), (out_dt, ldo, off, np.argwhere(rows[:, :w * h] != want)[:4])
            expect = fill.copy()
            expect[off:off + n * ldo].reshape(n, ldo)[:, :w * h] = want
            assert np.array_equal(after, expect), (out_dt, ldo, off, "bytes outside the windows changed")
    frame.assert_untouched()


# ---- 4. more than 65535 boxes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nearest", "nearest_rotated", "bicubic_rotated"])
def test_more_boxes_than_grid_rows(pt, small, case):
    """65568 boxes = 2732 copies of FC.boxes(): the launches have 65535 rows of workgroups and 33 of them take a second trip through
    ``for (b = blockIdx.y; b < n; b += gridDim.y)`` — in k_filter_gather_rot with its barriers.  FC.ANGLES cycles with period 8, which
    divides 24: the result is the 24-box result (PIL's), tiled."""
    import torch
    copies, size = 2732, (16, 12)
    b24 = FC.boxes()
    a24 = np.resize(np.array(FC.ANGLES), 24) if case != "nearest" else np.zeros(24)
    filt = 3 if case == "bicubic_rotated" else 0
    want = torch.from_numpy(np.array(pil_ref(b24, a24, size, filt))).cuda()
    boxes, angs = np.tile(b24, (copies, 1)), np.tile(a24, copies)
    n = len(boxes)
    assert n == 65568 and n > 65535
    bdev, adev = torch.from_numpy(boxes).cuda(), torch.from_numpy(angs).cuda()
    for lay in [l for l in small[np.uint8] if l.name in ("dense", "roi") and l.seed == FILLS[0]]:
        odev = torch.full((n, 192), 7, dtype=torch.uint8, device="cuda")
        pt.extract_device(lay.view.data_ptr(), np.uint8, FC.FRAME_H, FC.FRAME_W, lay.view.stride(0), bdev.data_ptr(), n, size, odev.data_ptr(), np.uint8, 192,
                          stream=torch.cuda.current_stream().cuda_stream, delta_angs_ptr=None if case == "nearest" else adev.data_ptr(), interpolation=filt)
        torch.cuda.synchronize()
        got = odev.view(copies, 24, 192)
        same = (got == want[None]).all(dim=2)                  # (copies, 24)
        assert bool(same.all()), (case, lay, torch.nonzero(~same)[:4].tolist())
        assert bool(want.any()) and torch.equal(got[-1], want)      # the last copy: boxes 65544 .. 65567, all on the second trip
        lay.assert_untouched()


# ---- 5. narrow frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fw", [1, 7, 8, 9, 15])
def test_narrow_frames(pt, fw):
    """Frames narrower than, as wide as and just wider than one 8-byte load, (16, 12) windows (k_extent_gather_u8x16): below 8 pixels the
    8-byte branch must never be chosen, at 8 only a group that starts at column 0 qualifies, at 9 columns 0 and 1.  Boxes: the whole
    frame, its left half, one hanging over the right edge, and slivers inside pixel 0, pixel 1 and the last pixel (all sixteen columns
    read one source pixel: the groups that do qualify)."""
    for fh in (1, 5):
        f = np.random.default_rng(9500 + 16 * fw + fh).integers(1, 256, (fh, fw), dtype=np.uint8)
        boxes = np.array([[0.0, 0.0, fw, fh], [0.0, 0.0, fw / 2.0, fh], [fw * 0.5, 0.0, fw * 1.5, fh],
                          [0.1, 0.0, 0.9, fh], [min(1, fw - 1) + 0.1, 0.0, min(1, fw - 1) + 0.9, fh], [fw - 0.9, 0.0, fw - 0.1, fh]])
        want = FC.pil_windows(f, boxes, np.zeros(len(boxes)), (16, 12), 0)
        sliver = want[3].reshape(12, 16)
        assert (sliver == sliver[:, :1]).all() and sliver[0, 0] == f[0, 0] and want[5, 0] == f[0, fw - 1]
        assert want[:2].all() and (want[2] == 0).any() and want[2].any()
        wide = [i for i, b in enumerate(boxes) if takes_8_byte_loads(b, 16, fw)]
        assert wide == {1: [], 7: [], 8: [3], 9: [3, 4], 15: [1, 3, 4]}[fw], wide
        lays = layouts(f, ("dense", "pad1"))
        got = assert_layout_invariant(lays, lambda v: cut(pt, v, boxes, (16, 12)))
        assert np.array_equal(got, want), (fw, fh, np.argwhere(got != want)[:4])


# ---- 6. cascade, eye step, tracker -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig_lays(rig):
    """The rig's 160 x 120 frame in every layout (pitches 160, 161, 192, 184)."""
    lays = layouts(rig.frame)
    assert [l.view.stride(0) for l in lays] == [160, 161, 161, 192, 192, 184, 184]
    return lays


@pytest.fixture(scope="module")
def refs(rig):
    """The host-composed loops the cascade tests share (they read the contiguous numpy frame), computed once."""
    out = {}
    for name, formats in (("filters", FORMATS), ("nearest", None), ("bicubic", [3] * 10)):
        out[name] = rig.composed_loop(formats)
    return out


def same_detection(a, b):
    try:
        assert_same_detection(a, b, "layouts")
    except AssertionError:
        return False
    return a["counts"] == b["counts"] and a["rows_executed"] == b["rows_executed"] and a["n_windows"] == b["n_windows"]


def assert_detection_is(got, ref, rig, what):
    assert_same_detection(got, ref, what)
    known = [i for i, c in enumerate(got["counts"]) if c >= 0]
    assert [i for i in known if rig.stages[i].type == "Disc"] == [i for i, s in enumerate(rig.stages) if s.type == "Disc"]
    assert [got["counts"][i] for i in known] == [ref["counts"][i] for i in known], (what, got["counts"], ref["counts"])


@pytest.mark.parametrize("which", ["filters", "nearest"])
def test_cascade_detect_on_every_layout(rig, rig_lays, refs, which):
    """160 x 120 needs no prescale: the stage loop itself (first stage keyed, later stages rotated, BILINEAR / BICUBIC or all NEAREST) reads
    the pitched frame."""
    ref, seen = refs[which]
    print("extracting stages (stage, filter, rows, rotated rows):", seen, "counts:", ref["counts"])
    if which == "filters":      # the rig's own guards: survivors, a non-zero angle among them, a BICUBIC stage with rotated rows
        assert len(ref["coords"]) >= 1 and np.abs(ref["angles"]).max() > 0
        assert seen[0][:2] == (0, 2) and seen[0][2] == len(rig.boxes)
        assert [(k, f, n, nz) for k, f, n, nz in seen[1:] if f == 3 and nz >= 3 and ref["counts"][k] >= 3], seen
    else:
        # all NEAREST, the host loop ends with no survivor on this frame (counts ... 37, 9, 2, 0): what is compared is the count after
        # every Disc stage, and rotated windows must have survived one of them
        assert all(f == 0 for _, f, _, _ in seen) and [k for k, _, _, nz in seen[1:] if nz >= 3 and ref["counts"][k] >= 1], seen
    dc = rig.cascade(FORMATS if which == "filters" else None)
    got = assert_layout_invariant(rig_lays, lambda v: dc.detect(v, smallest_face=SF), equal=same_detection)
    assert_detection_is(got, ref, rig, which)
    # windows from the host: the unkeyed first stage
    explicit = assert_layout_invariant(rig_lays, lambda v: dc.detect(v, smallest_face=SF, windows=(rig.boxes, rig.level)), equal=same_detection)
    assert_detection_is(explicit, ref, rig, which + ", windows from the host")


def test_one_cascade_over_alternating_layouts(rig, rig_lays, refs):
    """The keyed first-stage tables belong to the frame's shape, not to its pitch: dense, pad1, roi, pad_al, dense through one cascade."""
    dc = rig.cascade(FORMATS)
    by_name = {}
    for l in rig_lays:
        by_name.setdefault(l.name, l)
    for i, name in enumerate(("dense", "pad1", "roi", "pad_al", "dense")):
        assert_detection_is(dc.detect(by_name[name].view, smallest_face=SF), refs["filters"][0], rig, "call %d on %s" % (i, name))
        by_name[name].assert_untouched()


def test_detect_frame_and_detect_faces_on_every_layout(rig, rig_lays, refs):
    dc, loc = rig.cascade(FORMATS), rig.locator(3)
    ref = refs["filters"][0]
    det = assert_layout_invariant(rig_lays, lambda v: dc.detect_frame(v, smallest_face=SF), equal=same_detection)
    assert_detection_is(det, ref, rig, "detect_frame")
    for l in rig_lays:
        assert dc.prescale(l.view) is l.view                   # no prescale: the stage loop read the view itself
    want, n_before = composed_faces(dc, loc, rig.fdev, ref)      # the eye step, the discard and the purge on the host loop's survivors
    assert len(want) >= 1

    def same_faces(a, b):
        return all(np.array_equal(a[k], b[k]) if k == "faces" else a[k] == b[k] for k in a) and a.keys() == b.keys()
    got = assert_layout_invariant(rig_lays, lambda v: dc.detect_faces(v, loc, smallest_face=SF), equal=same_faces)
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want)
    assert got["n_before_purge"] == n_before and got["counts"] == det["counts"]


@pytest.mark.parametrize("filt", [3, 0])
def test_eye_step_on_every_layout(rig, rig_lays, filt):
    loc = rig.locator(filt)
    nz = np.flatnonzero(np.abs(rig.face_angles) > 1.0)[:4]
    boxes, angles = rig.face_boxes[nz], rig.face_angles[nz]
    assert len(nz) == 4
    eb = loc.eye_boxes(boxes, angles)
    dang = -np.concatenate([angles, angles])
    want = ER.contrast(FC.pil_windows(rig.frame, eb, dang, SUB, filt), *CONTRAST)

    def same(a, b):
        return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    out = assert_layout_invariant(rig_lays, lambda v: loc.locate(v, boxes, angles, return_patches=True), equal=same)
    assert out["patches"].shape == (8, 256) and np.array_equal(out["patches"], want)
    assert set(out) == {"eye_coords", "too_far", "reg", "patches"} and np.isfinite(out["reg"]).all()


def test_tracker_on_roi_views(rig, refs):
    """Two steps on crops of two different larger frames: a full-grid frame, then a tracked one (nine windows), against the composed
    answers of test_filters_gpu.test_detect_faces_and_tracked_frame_bicubic (here rooted in the host loop)."""
    from pyfaceanalysis_amd.cascade import tracked_windows
    from pyfaceanalysis_amd.tracking import FaceTracker
    dc, loc = rig.cascade([3] * 10), rig.locator(3)
    det = dc.detect_frame(rig.fdev, smallest_face=SF)
    assert_detection_is(det, refs["bicubic"][0], rig, "all BICUBIC")
    want, n_before = composed_faces(dc, loc, rig.fdev, refs["bicubic"][0])
    det9 = dc.detect(rig.fdev, windows=tracked_windows(want[0, :4], rig.pipe, SUB))
    want9, n9 = composed_faces(dc, loc, rig.fdev, det9)
    assert len(want) >= 1
    roi0, roi1 = DevLayout(rig.frame, "roi", FILLS[0]), DevLayout(rig.frame, "roi", FILLS[1])
    tr = FaceTracker(dc, loc, smallest_face=SF)
    try:
        r0 = tr.step(roi0.view)
        assert r0["tracked"] is False and r0["n_windows"] == len(rig.boxes) and np.array_equal(r0["faces"], want) and r0["n_before_purge"] == n_before
        r1 = tr.step(roi1.view)
        assert r1["tracked"] is True and r1["n_windows"] == 9
        assert r1["faces"].shape == want9.shape and np.array_equal(r1["faces"], want9) and r1["n_before_purge"] == n9
    finally:
        tr.close()
    roi0.assert_untouched()
    roi1.assert_untouched()


def test_prescale_reads_the_pitch(rig, rig_lays):
    """On a large frame the prescale is the only reader of the caller's pitch.  1280 x 720 -> 1000 x 562 against PIL's NEAREST resize; on the
    rig's frame ``prescale_size=120`` gives a 120 x 90 frame, and the detection on it is the detection on PIL's resized frame (107
    windows, 7 survivors)."""
    import torch
    from PIL import Image
    dc = rig.cascade(FORMATS)
    f = np.random.default_rng(9601).integers(1, 256, (720, 1280), dtype=np.uint8)
    assert grid.prescaled_size(1280, 720, 1000) == (1000, 562)
    want = np.asarray(Image.fromarray(f).resize((1000, 562), Image.NEAREST))
    for lay in layouts(f, ("roi", "pad1")):
        small_t = dc.prescale(lay.view, 1000)
        assert small_t.shape == (562, 1000) and small_t.is_contiguous() and np.array_equal(small_t.cpu().numpy(), want), lay
        small_t.zero_()                                        # the tensor lives with the cascade: the next layout must write it again
        lay.assert_untouched()
    assert grid.prescaled_size(160, 120, 120) == (120, 90)
    small_f = np.asarray(Image.fromarray(rig.frame).resize((120, 90), Image.NEAREST))
    want_det = dc.detect(torch.from_numpy(small_f.copy()).cuda(), smallest_face=SF)
    for lay in rig_lays:
        assert np.array_equal(dc.prescale(lay.view, 120).cpu().numpy(), small_f), lay
    got = assert_layout_invariant(rig_lays, lambda v: dc.detect_frame(v, smallest_face=SF, prescale_size=120), equal=same_detection)
    print("prescaled to 120 x 90: %d windows, counts %s, %d survivors" % (got["n_windows"], got["counts"], len(got["coords"])))
    assert got["n_windows"] > 0 and got["n_windows"] == want_det["n_windows"]
    assert_detection_is(got, want_det, rig, "prescale 120")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_row_stride_below_the_width_is_refused(rig, refs):
    """A broadcast view has ``stride(0) == 0`` and ``stride(1) == 1``: the Python checks let it through, every entry of the library must
    refuse it as a bad argument (ValueError) before it writes anything, and stay usable."""
    import torch
    from pyfaceanalysis_amd.cascade import frame_levels
    from pyfaceanalysis_amd.tracking import FaceTracker
    L = _capi.lib()
    dc, loc = rig.cascade(FORMATS), rig.locator(3)
    bad = torch.zeros(1, 160, dtype=torch.uint8, device="cuda").expand(120, 160)
    assert bad.stride(0) == 0 and bad.stride(1) == 1 and bad.shape == rig.fdev.shape
    ref = refs["filters"][0]
    nz = np.flatnonzero(np.abs(rig.face_angles) > 1.0)[:4]
    boxes, angles = rig.face_boxes[nz], rig.face_angles[nz]
    good_det = dc.detect(rig.fdev, smallest_face=SF)
    good_frame = dc.detect_frame(rig.fdev, smallest_face=SF)
    good_faces = dc.detect_faces(rig.fdev, loc, smallest_face=SF)
    good_eyes = loc.locate(rig.fdev, boxes, angles, return_patches=True)
    good_small = dc.prescale(rig.fdev, 120).clone()
    assert_detection_is(good_det, ref, rig, "before")
    st = torch.cuda.current_stream().cuda_stream

    # detect: through the wrapper, and through the C entry with outputs of our own, which stay as they were
    with pytest.raises(ValueError):
        dc.detect(bad, smallest_face=SF)
    with pytest.raises(ValueError):
        dc.detect(bad, smallest_face=SF, windows=(rig.boxes, rig.level))
    levels, n_levels, n0 = frame_levels(160, 120, SF, rig.pipe, SUB)
    coords, angs, conf = np.full((n0, 4), -7.0), np.full(n0, -7.0), np.full(n0, -7.0)
    oidx, counts = np.full(n0, -7, dtype=np.int32), np.full(len(rig.stages), -7, dtype=np.int32)
    n_out, rows = C.c_int64(-7), C.c_int64(-7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for ld in (0, 159, -160):
        rc = L.hg_cascade_detect_levels_device(dc._handle(), C.c_void_p(rig.fdev.data_ptr()), 120, 160, ld, levels, n_levels, vp(coords), vp(angs), vp(oidx),
                                               vp(conf), n0, C.byref(n_out), vp(counts), C.byref(rows), C.c_void_p(st))
        assert rc == _capi.HG_ERR_ARG, ld
        rc = L.hg_cascade_detect_device(dc._handle(), C.c_void_p(rig.fdev.data_ptr()), 120, 160, ld, vp(rig.boxes), vp(rig.level), len(rig.boxes), vp(coords),
                                        vp(angs), vp(oidx), vp(conf), n0, C.byref(n_out), vp(counts), C.byref(rows), C.c_void_p(st))
        assert rc == _capi.HG_ERR_ARG, ld
    assert (coords == -7).all() and (angs == -7).all() and (conf == -7).all() and (oidx == -7).all() and (counts == -7).all()
    assert n_out.value == -7 and rows.value == -7
    assert_detection_is(dc.detect(rig.fdev, smallest_face=SF), ref, rig, "detect after the refusal")

    # detect_frame / detect_faces: their per-shape plans hold the result buffers
    frame_plan = dc._frames[(160, 120, float(SF), grid.PRESCALE_SIZE)]
    faces_plan = dc._frames[("faces", 160, 120, float(SF), grid.PRESCALE_SIZE)]
    for b in frame_plan[4]:
        b[...] = -7
    faces_plan[4][...] = -7.0
    with pytest.raises(ValueError):
        dc.detect_frame(bad, smallest_face=SF)
    with pytest.raises(ValueError):
        dc.detect_frame(bad, smallest_face=SF, prescale_size=120)
    with pytest.raises(ValueError):
        dc.detect_faces(bad, loc, smallest_face=SF)
    assert all((b == -7).all() for b in frame_plan[4]) and (faces_plan[4] == -7.0).all()
    assert same_detection(dc.detect_frame(rig.fdev, smallest_face=SF), good_frame)
    again = dc.detect_faces(rig.fdev, loc, smallest_face=SF)
    assert np.array_equal(again["faces"], good_faces["faces"]) and again["counts"] == good_faces["counts"]

    # prescale: the prescaled tensor that lives with the cascade is not written
    kept = dc._prescale[(160, 120, 120, 90)][1]
    kept.fill_(201)
    with pytest.raises(ValueError):
        dc.prescale(bad, 120)
    torch.cuda.synchronize()
    assert bool((kept == 201).all())
    assert torch.equal(dc.prescale(rig.fdev, 120), good_small)

    # locate: the wrapper, and the C entry with outputs of our own
    with pytest.raises(ValueError):
        loc.locate(bad, boxes, angles, return_patches=True)
    bdev, adev = torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(angles.copy()).cuda()
    ec = torch.full((4, 4), -7.0, dtype=torch.float64, device="cuda")
    tf = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    patches = torch.full((8, 256), -7.0, dtype=torch.float32, device="cuda")
    reg = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    rc = L.hg_eyes_locate_device(loc._handle(), bad.data_ptr(), 120, 160, bad.stride(0), bdev.data_ptr(), adev.data_ptr(), 4, ec.data_ptr(), tf.data_ptr(),
                                 patches.data_ptr(), reg.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == _capi.HG_ERR_ARG
    assert bool((ec == -7).all()) and bool((tf == 7).all()) and bool((patches == -7).all()) and bool((reg == -7).all())
    again = loc.locate(rig.fdev, boxes, angles, return_patches=True)
    assert all(np.array_equal(again[k], good_eyes[k]) for k in good_eyes)

    # the tracker: refused on a full-grid step and on a tracked step; its plan's rows stay; it is reset and finds the face again
    tr = FaceTracker(dc, loc, smallest_face=SF)
    try:
        with pytest.raises(ValueError):
            tr.step(bad)
        r0 = tr.step(rig.fdev)
        assert r0["tracked"] is False and np.array_equal(r0["faces"], good_faces["faces"]) and tr.tracked_face is not None
        plan_rows = tr._plans[(160, 120)][4]
        plan_rows[...] = -7.0
        with pytest.raises(ValueError):
            tr.step(bad)                                        # would have been a tracked frame
        assert (plan_rows == -7.0).all() and tr.tracked_face is None
        r1 = tr.step(rig.fdev)
        assert r1["tracked"] is False and np.array_equal(r1["faces"], good_faces["faces"])      # reset: the full grid again
        r2 = tr.step(rig.fdev)
        assert r2["tracked"] is True and r2["n_windows"] == 9
    finally:
        tr.close()
