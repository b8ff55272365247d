"""GPU: pose-normalised face crops on the device (hg_patcher_normalize_device, csrc/hg_normalize.hip) against PIL itself composed as
the reference composes it (tests/normalize_cases.py::pil_normalize) driven by the host geometry, ``array_equal``: both device paths and
the default choice between them, batches with refused faces, pitched frames and crop views, pitched outputs, the host twin, and the
rows of the synthetic cascade of tests/test_eyes_gpu.py normalised with the "age" preset."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, normalize as N
from tests import normalize_cases as NC
from tests.test_eyes_gpu import setup      # noqa: F401  (the synthetic frame, cascade and eye locator, built as that module builds them)

CASES = NC.gpu_cases()
_WANT = {}


def expected(case):
    """(geoms, PIL's image) of a case, computed once."""
    name, fs, e, size, method = case
    if name not in _WANT:
        g = N.geometry([e], fs, size, method)
        _WANT[name] = (g, NC.pil_normalize(NC.noise_frame(*fs), g[0], size))
    return _WANT[name]


@pytest.fixture(scope="module")
def dev(native_lib):
    import torch
    frames = {fs: torch.from_numpy(NC.noise_frame(*fs)).cuda() for fs in NC.FRAME_SIZES[:2] + [NC.SQUARE_FRAME]}
    norm = {(size, method): N.FaceNormalizer(0, preset="pose", out_size=size, method=method) for size, method in NC.OUT_SIZES}
    yield dict(torch=torch, frames=frames, norm=norm)
    torch.cuda.synchronize()
    for n in norm.values():
        n.close()


def method_name(method):
    return "eyes_inferred-mouth_areaZ" if method == NC.AREAZ else "eyes_inferred-mouth_area"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_pil_on_both_paths_and_the_host_twin(dev, case):
    name, fs, e, size, method = case
    g, want = expected(case)
    fn = dev["norm"][(size, method)]
    frame = dev["frames"][fs]
    for flags in (0, 1, 2):      # the default choice, every face staged, every face tap by tap
        img, status = fn.normalize(frame, [e], flags=flags)
        assert img.shape == (1, size[1], size[0]) and img.dtype == dev["torch"].uint8 and status.dtype == np.int32 and status[0] == 0
        assert np.array_equal(img[0].cpu().numpy(), want), (name, flags)
    host = N.normalize_host(NC.noise_frame(*fs), [e], size, method_name(method))[0][0]
    assert np.array_equal(host, want)


@pytest.mark.gpu
def test_cases_cover_both_default_paths(dev):
    taps = {c[0] for c in CASES if int(expected(c)[0][0]["rect"][2]) * int(expected(c)[0][0]["rect"][3]) > 16 * c[3][0] * c[3][1]}
    assert {"97x61-wider-17x13", "160x120-wider-32x24", "160x120-wider-17x13", "65x65-wider-17x13"} <= taps and len(taps) < len(CASES) // 2, taps
    assert NC.AT_THE_BOUND[0] not in taps
    unrotated = [c[0] for c in CASES if not expected(c)[0][0]["rotated"]]
    square = [c[0] for c in CASES if abs(expected(c)[0][0]["angle"]) == 90.0 and expected(c)[0][0]["W"] == expected(c)[0][0]["H"]]
    assert len(unrotated) >= 4 and len(square) >= 4


def batch_eyes(fs):
    """70 faces of mixed geometry, the four kinds of refused face in the middle."""
    refused = [(5.0, 5.0, 4.0, 5.0), (np.nan, 1.0, 2.0, 3.0), (7.0, 7.0, 7.0, 7.0), (-1e9, -1.135e9, 1e9, -1.135e9 + 3e6)]
    good = [e for _, e in NC.eye_sets(*fs)] + [tuple(r) for r in NC.random_eyes(80, fs, seed=9)]
    eyes = good[:30] + refused[:2] + good[30:45] + refused[2:] + good[45:]
    return np.array(eyes[:70], dtype=np.float64), [30, 31, 47, 48], [1, 2, 3, 4]


@pytest.mark.gpu
@pytest.mark.parametrize("size,method", NC.SMALL_OUT_SIZES)
def test_batches_of_0_1_and_70_faces(dev, size, method):
    fs = (97, 61)
    fn, frame, host_frame = dev["norm"][(size, method)], dev["frames"][fs], NC.noise_frame(*fs)
    eyes, where, codes = batch_eyes(fs)
    img0, st0 = fn.normalize(frame, np.zeros((0, 4)))
    assert tuple(img0.shape) == (0, size[1], size[0]) and st0.shape == (0,)
    g = fn.geometry(eyes, fs)
    want = np.stack([NC.pil_normalize(host_frame, gi, size) for gi in g])
    n_taps = sum(int(gi["rect"][2]) * int(gi["rect"][3]) > 16 * size[0] * size[1] for gi in g)
    assert 0 < n_taps < 60      # the batch mixes both paths
    for flags in (0, 1, 2):
        img, status = fn.normalize(frame, eyes, flags=flags)
        got = img.cpu().numpy()
        assert list(status[where]) == codes and np.count_nonzero(status) == 4
        assert not got[where].any()
        assert np.array_equal(got, want), flags
    got = fn.normalize(frame, eyes)[0].cpu().numpy()
    for i in range(len(eyes)):      # neighbours of refused faces, and everyone else: the bytes of a call of their own
        one, st = fn.normalize(frame, eyes[i:i + 1])
        assert st[0] == (codes[where.index(i)] if i in where else 0)
        assert np.array_equal(one[0].cpu().numpy(), got[i]), i


@pytest.mark.gpu
def test_pitched_frames_crop_views_and_pitched_outputs(dev):
    t = dev["torch"]
    fs, (size, method) = (160, 120), NC.SMALL_OUT_SIZES[0]
    fn = dev["norm"][(size, method)]
    host_frame = NC.noise_frame(*fs)
    eyes = np.array([e for _, e in NC.eye_sets(*fs)])
    want = fn.normalize(dev["frames"][fs], eyes)[0].cpu().numpy()
    assert np.array_equal(want, np.stack([NC.pil_normalize(host_frame, gi, size) for gi in fn.geometry(eyes, fs)]))
    for view in (NC.pitched(host_frame), NC.crop_view(host_frame)):
        base = t.from_numpy(np.ascontiguousarray(view.base)).cuda()
        off = (view.__array_interface__["data"][0] - view.base.__array_interface__["data"][0])
        y0, x0 = divmod(off, view.base.shape[1])
        dview = base[y0:y0 + fs[1], x0:x0 + fs[0]]
        assert not dview.is_contiguous() and np.array_equal(dview.cpu().numpy(), host_frame)
        for flags in (0, 1, 2):
            assert np.array_equal(fn.normalize(dview, eyes, flags=flags)[0].cpu().numpy(), want)
    # images farther apart than their size: the gap bytes are untouched
    n, px, gap = len(eyes), size[0] * size[1], 13
    buf = t.full((n, px + gap), 0xA5, dtype=t.uint8, device="cuda")
    out = buf[:, :px].view(n, size[1], size[0])
    got, _ = fn.normalize(dev["frames"][fs], eyes, out=out)
    assert got.data_ptr() == buf.data_ptr()
    b = buf.cpu().numpy()
    assert np.array_equal(b[:, :px].reshape(n, size[1], size[0]), want) and np.all(b[:, px:] == 0xA5)


@pytest.mark.gpu
def test_device_entry_refuses_bad_arguments(dev):
    t = dev["torch"]
    fs, (size, method) = (97, 61), NC.SMALL_OUT_SIZES[0]
    fn, frame = dev["norm"][(size, method)], dev["frames"][fs]
    g = fn.geometry([NC.eye_sets(*fs)[1][1]], fs)
    px = size[0] * size[1]
    out = t.full((1, px), 7, dtype=t.uint8, device="cuda")
    L = _capi.lib()
    h = fn._patcher._handle()
    gp = g.ctypes.data_as(C.c_void_p)
    base = dict(p=h, flags=0, frame=frame.data_ptr(), fh=61, fw=97, ld=97, g=gp, n=1, ow=size[0], oh=size[1], out=out.data_ptr(), ldo=px, st=None)
    call = lambda **kw: L.hg_patcher_normalize_device(*[dict(base, **kw)[k] for k in ("p", "flags", "frame", "fh", "fw", "ld", "g", "n", "ow", "oh", "out", "ldo", "st")])
    for kw in (dict(p=None), dict(frame=None), dict(g=None), dict(out=None), dict(fh=0), dict(fw=-1), dict(ld=96), dict(ldo=px - 1), dict(ow=0), dict(oh=4097),
               dict(n=-1), dict(flags=3), dict(flags=4), dict(fw=150, ld=150)):
        assert call(**kw) == _capi.HG_ERR_ARG, kw
    t.cuda.synchronize()
    assert bool((out == 7).all())      # nothing was launched
    assert call(n=0) == _capi.HG_OK
    t.cuda.synchronize()
    assert bool((out == 7).all())
    assert call() == _capi.HG_OK
    t.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(size[1], size[0]), NC.pil_normalize(NC.noise_frame(*fs), g[0], size))
    with pytest.raises(ValueError, match="float"):
        fn.normalize(frame.float(), [NC.eye_sets(*fs)[0][1]])
    with pytest.raises(ValueError):
        fn.normalize(frame.cpu(), [NC.eye_sets(*fs)[0][1]])
    with pytest.raises(ValueError):      # a colour frame goes through frames.to_gray first
        fn.normalize(frame[:, :, None].expand(61, 97, 3).contiguous(), [NC.eye_sets(*fs)[0][1]])


@pytest.mark.gpu
def test_cascade_rows_normalised_with_the_age_preset(setup):      # noqa: F811
    """detect_faces rows -> FaceNormalizer("age") on the prescaled frame the rows refer to -> PIL on the same rows; the images are frames:
    the patcher cuts a window from one."""
    import torch
    from pyfaceanalysis_amd.patches import Patcher
    s = setup
    faces = s["dc"].detect_faces(s["fdev"], s["loc"], smallest_face=0.1)["faces"]
    assert len(faces) > 0
    small = s["dc"].prescale(s["fdev"])
    fn = N.FaceNormalizer(0, preset="age")
    img, status = fn.normalize(small, faces[:, 5:9])
    assert tuple(img.shape) == (len(faces), 260, 256) and np.any(status == 0)
    g = fn.geometry(faces[:, 5:9], (small.shape[1], small.shape[0]))
    host_small = small.cpu().numpy()
    got = img.cpu().numpy()
    for i in range(len(faces)):
        assert np.array_equal(got[i], NC.pil_normalize(host_small, g[i], (256, 260))), i
    i = int(np.flatnonzero(status == 0)[0])
    pt = Patcher()
    boxes = torch.tensor([[64.0, 70.0, 192.0, 198.0], [-10.0, 100.0, 118.0, 228.0]], dtype=torch.float64, device="cuda")
    win = torch.empty((2, 64 * 64), dtype=torch.uint8, device="cuda")
    pt.extract_device(img[i].data_ptr(), np.uint8, 260, 256, 256, boxes.data_ptr(), 2, (64, 64), win.data_ptr(), np.uint8, 64 * 64,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    from PIL import Image
    pil = Image.fromarray(got[i])
    want = np.stack([np.asarray(pil.transform((64, 64), Image.EXTENT, tuple(b), Image.NEAREST)).reshape(-1) for b in boxes.cpu().numpy()])
    assert np.array_equal(win.cpu().numpy(), want) and want.any()
    pt.close()
    fn.close()
