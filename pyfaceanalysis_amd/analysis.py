"""Age, race and gender of the detected faces, on the device: ``estimate_age_race_gender`` (face_analysis.py:1170-1306; called from
FaceDetectUpdated.py:1186-1187), the reference's last step per image (include/higsfa.h, "Age, race and gender estimation").

Per purged face the reference makes the 256 x 260 pose-normalised crop (``normalize.FaceNormalizer(preset="age")``), cuts ONE 96 x 96
sub-image from it with a contrast step, runs the age network on it and evaluates three classifiers on the same features: age (with its
std), race and gender — the Race and Gender stages have no network of their own (Pipelines/Pipeline_experimental.txt:62-70).
``FaceAnalyzer.estimate`` enqueues that whole chain for all faces of a frame and reads back one (4, n) block.

The sub-image is cut by cuicuilco's ``load_image_data_monoprocessor``, which is not available.  The build owns three rules
(DESIGN.md §1.1), each pinned against PIL in tests/test_analysis_gpu.py:

box       ``age_patch_box()``: the reference's visible expressions (:1182-1197) in their order, under the stated reading of
          ``trans_sampled``.  A plain parameter: a caller who knows better passes ``box=``.
cut       ``crop.transform((pw, ph), EXTENT, box, F)``, F = ``interpolation`` (NEAREST by default).
contrast  the eye step's rule (``eyes.EyeLocator``): exact integer sums, ``p' = (p - mean) / (std / target_std + 1e-8) + target_mean``,
          float32.  The targets have no default.  ``clip=True`` clips to [0, 255] (face_analysis.py:327, the only rule the reference
          shows); ``clip=False`` does not — the reference's ``obj_avgs = 0.0`` makes sense only unclipped.

EYE COORDINATES ARE IN THE COORDINATES OF THE FRAME PASSED IN, as for ``normalize``: the rows of ``detect_faces`` / ``FaceTracker`` refer
to the frame the cascade read, so ``estimate_faces`` takes that frame (``DeviceCascade.prescale(frame)``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import normalize as _normalize

FILTERS = {"NEAREST": _capi.HG_FILTER_NEAREST, "BILINEAR": _capi.HG_FILTER_BILINEAR, "BICUBIC": _capi.HG_FILTER_BICUBIC}
FLAG_COMPOSED, FLAG_FUSED = 1, 2          # hg_estimator_*_device flags: force the composed patch path / the fused kernel (tests, A/B runs)


def age_patch_box(out_size=(256, 260), patch_size=(96, 96), base_scale=1.14, reduction=160.0 / 96, translation=(0.0, -6.0), trans_sampled=True):
    """The box (x0, y0, x1, y1), in the coordinates of the ``out_size`` crop, of the ``patch_size`` sub-image the reference hands to
    ``load_image_data_monoprocessor`` (face_analysis.py:1182-1197, :1231-1247): sampling ``base_scale * reduction``, the sub-image
    centred, the translation ``translation / reduction`` — in sampled pixels when ``trans_sampled``, which this build reads as "times
    the sampling".  Python floats in the reference's operation order; about (36.8, 31.96, 219.2, 214.36) by default."""
    ow, oh = out_size
    pw, ph = patch_size
    s = base_scale * reduction
    first_col = ow / 2.0 - pw * s / 2.0
    first_row = oh / 2.0 - ph * s / 2.0
    tx = translation[0] / reduction
    ty = translation[1] / reduction
    if trans_sampled:
        tx = tx * s
        ty = ty * s
    return (first_col + tx, first_row + ty, first_col + tx + pw * s, first_row + ty + ph * s)


def _strings(labels, bound, low, high, long_text):
    out = []
    for label in np.asarray(labels, dtype=np.float64).reshape(-1):
        if label < -bound or label > bound:
            raise ValueError("Unrecognized label: " + str(label))
        name = low if label <= 0 else high
        out.append(name if long_text else name[0])
    return out


def gender_strings(labels, long_text=True):
    """``map_real_gender_labels_to_strings`` (face_analysis.py:333-351): label <= 0 "Male" / "M", else "Female" / "F"; a label beyond
    +-1.000001 raises ValueError("Unrecognized label: ...")."""
    return _strings(labels, 1.000001, "Male", "Female", long_text)


def race_strings(labels, long_text=True):
    """``map_real_race_labels_to_strings`` (face_analysis.py:354-371): label <= 0 "Black" / "B", else "White" / "W"; beyond +-2.000001
    raises ValueError("Unrecognized label: ...")."""
    return _strings(labels, 2.000001, "Black", "White", long_text)


def gender_confidence(labels):
    """face_analysis.py:1294."""
    return np.abs(np.asarray(labels, dtype=np.float64))


def race_confidence(labels):
    """face_analysis.py:1295."""
    return np.abs(np.asarray(labels, dtype=np.float64)) / 2.0


def _filter(interpolation):
    if isinstance(interpolation, str):
        if interpolation not in FILTERS:
            raise ValueError("unknown interpolation filter %r (NEAREST, BILINEAR, BICUBIC)" % (interpolation,))
        return FILTERS[interpolation]
    return _capi.filter_code(interpolation)


class FaceAnalyzer(object):
    """``flow``: the age network, a ``flow.Flow`` on ``device`` with ``output_dtype=float32`` whose input is a ``patch_size`` sub-image.
    ``age`` / ``race`` / ``gender``: ``classifier.GaussianClassifier`` with ``avg_labels``, each optional, at least one.  ``contrast``:
    (target_mean, target_std) in pixel units, required.  ``box``: None = ``age_patch_box`` for the preset's crop and ``patch_size``.
    ``n_features``: feature columns computed (None: the widest classifier's ``input_dim``).  ``patcher``: a ``patches.Patcher`` to share
    (one stream per patcher); None: its own.  ``crop_size``: another (width, height) than the preset's for the normalised crop."""

    def __init__(self, flow, age=None, race=None, gender=None, *, contrast, clip=True, patch_size=(96, 96), box=None, interpolation="NEAREST",
                 n_features=None, normalizer_preset="age", patcher=None, device=0, crop_size=None):
        self.flow, self.age, self.race, self.gender = flow, age, race, gender
        self.filter = _filter(interpolation)
        self.contrast = (float(contrast[0]), float(contrast[1]))
        if not (self.contrast[1] > 0.0 and np.isfinite(self.contrast[1]) and np.isfinite(self.contrast[0])):
            raise ValueError("contrast must be (target_mean, target_std) with target_std > 0, got %r" % (contrast,))
        self.clip = bool(clip)
        self.patch_size = (int(patch_size[0]), int(patch_size[1]))
        self.device = int(device)
        clfs = [(n, c) for n, c in (("age", age), ("race", race), ("gender", gender)) if c is not None]
        if not clfs:
            raise ValueError("at least one classifier (age, race, gender) must be given")
        self.k = int(max(c.input_dim for _, c in clfs) if n_features is None else n_features)
        if flow.device != self.device or flow.output_dtype != np.float32:
            raise ValueError("flow must live on device %d with output_dtype float32" % self.device)
        if flow.input_dim != self.patch_size[0] * self.patch_size[1]:
            raise ValueError("flow reads %d columns, patches have %d x %d" % (flow.input_dim, self.patch_size[0], self.patch_size[1]))
        if flow.output_dim < self.k:
            raise ValueError("flow gives %d features, %d kept" % (flow.output_dim, self.k))
        for name, c in clfs:
            if c.input_dim > self.k:
                raise ValueError("%s reads %d features, %d kept" % (name, c.input_dim, self.k))
            if c.avg_labels is None:
                raise ValueError("%s needs avg_labels" % name)
        self._norm = _normalize.FaceNormalizer(self.device, preset=normalizer_preset, out_size=crop_size, patcher=patcher)
        self.crop_size = self._norm.out_size
        self.box = tuple(float(v) for v in (age_patch_box(self.crop_size, self.patch_size) if box is None else box))
        if len(self.box) != 4 or not all(np.isfinite(self.box)):
            raise ValueError("box must be four finite numbers (x0, y0, x1, y1), got %r" % (box,))
        self._h = None

    def consts(self):
        c = _capi.HgEstimatorConsts()
        c.crop_w, c.crop_h = self.crop_size
        nc = _normalize._consts(self.crop_size, self._norm.method, self._norm.rotate)
        c.method, c.rotate = nc.method, nc.rotate
        c.patch_w, c.patch_h = self.patch_size
        c.filter, c.clip = self.filter, 1 if self.clip else 0
        c.box[:] = self.box
        c.target_mean, c.target_std = self.contrast
        c.n_features, c.reserved = self.k, 0
        return c

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            cc = self.consts()
            clf = [None if c is None else c._handle(c.avg_labels) for c in (self.age, self.race, self.gender)]
            _capi.check(_capi.lib().hg_estimator_create(self.flow._handle().h, clf[0], clf[1], clf[2], C.byref(cc), self._norm._patcher._handle(), self.device,
                                                        C.byref(h)))
            self._h = h
        return self._h

    def patches(self, crops, out=None, flags=0):
        """The patch step alone (hg_estimator_patches_device): ``crops`` an (n, crop_h, crop_w) uint8 device tensor, each image contiguous,
        ``stride(0) >= crop_w * crop_h`` -> an (n, patch_w * patch_h) float32 device tensor (``out`` if given: that shape, contiguous rows,
        any row stride).  Enqueued on the current stream, no host wait."""
        import torch as t
        cw, ch = self.crop_size
        npix = self.patch_size[0] * self.patch_size[1]
        if (not isinstance(crops, t.Tensor) or not crops.is_cuda or crops.dtype != t.uint8 or crops.dim() != 3 or tuple(crops.shape[1:]) != (ch, cw)
                or (cw > 1 and crops.stride(2) != 1) or (ch > 1 and crops.stride(1) != cw) or (crops.shape[0] > 1 and crops.stride(0) < cw * ch)
                or (crops.device.index or 0) != self.device):
            raise ValueError("crops must be an (n, %d, %d) uint8 tensor on device %d whose images are contiguous" % (ch, cw, self.device))
        n = int(crops.shape[0])
        if out is None:
            out = t.empty((n, npix), dtype=t.float32, device=crops.device)
        elif (not isinstance(out, t.Tensor) or out.dtype != t.float32 or out.device != crops.device or tuple(out.shape) != (n, npix)
              or (npix > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < npix)):
            raise ValueError("out must be an (%d, %d) float32 tensor on %s with contiguous rows" % (n, npix, crops.device))
        if n:
            _capi.check(_capi.lib().hg_estimator_patches_device(self._handle(), int(flags), crops.data_ptr(), crops.stride(0) if n > 1 else cw * ch, n,
                                                                out.data_ptr(), out.stride(0) if n > 1 else npix,
                                                                t.cuda.current_stream(crops.device).cuda_stream))
        return out

    def estimate(self, frame, eyes=None, geoms=None, return_intermediates=False, flags=0):
        """``frame``: an (H, W) grey uint8 device tensor with contiguous rows, any row pitch; ``eyes``: (n, 4) located eyes in that frame's
        coordinates (or ``geoms`` from ``normalize.geometry`` for that frame size and this analyzer's crop).  Returns a dict, with only the
        keys of the classifiers given: ``age``, ``age_std``, ``race``, ``gender`` float64 arrays (one device-to-host copy of the (4, n)
        block, the call's only wait); ``race_confidence`` = |race| / 2, ``gender_confidence`` = |gender|; ``race_label`` /
        ``gender_label`` lists of strings; ``status`` (``normalize.STATUS``).  A refused face (status != 0) has NaN values and ``None``
        labels.  ``return_intermediates``: also ``patches`` (n, patch_w * patch_h) and ``features`` (n, n_features), float32.  ``flags`` is
        for tests and A/B runs (``FLAG_COMPOSED`` / ``FLAG_FUSED``: the patch path; same bits)."""
        import torch as t
        from .eyes import check_frame
        if not isinstance(frame, t.Tensor) or not frame.is_cuda:
            raise ValueError("estimate takes a device tensor")
        if frame.dtype != t.uint8:
            raise ValueError("frame must be grey uint8 (a float frame is not offered; a colour frame goes through frames.to_gray first)")
        check_frame(t, frame, frame.device)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        if h == 0 or w == 0:
            raise ValueError("frame must not be empty")
        if (frame.device.index or 0) != self.device:
            raise ValueError("frame is on %s, the analyzer on device %d" % (frame.device, self.device))
        g = self._norm.geometry(eyes, (w, h)) if geoms is None else _normalize._check_geoms(geoms)
        n = int(g.shape[0])
        npix = self.patch_size[0] * self.patch_size[1]
        out = t.empty((4, n), dtype=t.float64, device=frame.device)
        pt = t.empty((n, npix), dtype=t.float32, device=frame.device) if return_intermediates else None
        ft = t.empty((n, self.k), dtype=t.float32, device=frame.device) if return_intermediates else None
        if n:
            _capi.check(_capi.lib().hg_estimator_estimate_device(
                self._handle(), int(flags), frame.data_ptr(), h, w, frame.stride(0) if h > 1 else w, g.ctypes.data_as(C.c_void_p), n, out.data_ptr(), n,
                None if pt is None else pt.data_ptr(), None if ft is None else ft.data_ptr(), t.cuda.current_stream(frame.device).cuda_stream))
        return self._result(out.cpu().numpy(), g["status"].astype(np.int32), pt, ft)

    def _result(self, block, status, pt, ft):
        """The dict of ``estimate`` from the (4, n) host block, the status per face and the intermediates (device tensors or None)."""
        ok = status == 0
        res = dict(status=status)
        if self.age is not None:
            res["age"], res["age_std"] = block[0], block[1]
        for key, row, conf, strings in (("race", 2, race_confidence, race_strings), ("gender", 3, gender_confidence, gender_strings)):
            if getattr(self, key) is None:
                continue
            v = block[row]
            res[key] = v
            res[key + "_confidence"] = conf(v)
            names = iter(strings(v[ok]))
            res[key + "_label"] = [next(names) if o else None for o in ok]
        if pt is not None:
            res["patches"], res["features"] = (a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in (pt, ft))
        return res

    def estimate_frames(self, stack, eyes=None, face_frame=None, geoms=None, return_intermediates=False, flags=0):
        """``estimate`` for faces spread over a stack of B same-size frames as ONE pooled chain (hg_estimator_estimate_frames_device: one
        normalise, one patch step, one network call and the regressions on all n rows).  ``stack``: a (B, H, W) grey uint8 device tensor
        (``normalize.check_grey_stack``) — for the rows of ``detect_faces_frames`` the prescaled stack the cascade read,
        ``DeviceCascade.prescale_frames(stack)``; ``eyes`` (n, 4) in each face's own frame (or ``geoms``); ``face_frame`` (n,) integers,
        the frame of every face, in any order.  Returns the dict of ``estimate`` over all n faces — face i's values are, bit for bit,
        those of ``estimate(stack[face_frame[i]], eyes[i:i + 1])`` — with one device-to-host copy of the (4, n) block, the call's only
        wait.  A face whose frame index is outside [0, B) has status ``normalize.STATUS_FRAME_RANGE``, NaN values and ``None`` labels, like
        a refused face.  An empty stack or n = 0 touches no library entry."""
        import torch as t
        stack = _normalize.check_grey_stack(t, stack, None, "estimate_frames")      # layout first, then the faces, then the device
        if geoms is not None:
            g = _normalize._check_geoms(geoms)
        else:
            e = _normalize._eyes(eyes)
            g = (self._norm.geometry(e, (int(stack.shape[2]), int(stack.shape[1]))) if stack is not None and len(e)
                 else np.zeros(len(e), dtype=_capi.NORM_GEOM_DTYPE))
        n = int(g.shape[0])
        ff = _normalize.check_face_frame(face_frame, n)
        _normalize.check_stack_device(stack, self.device, "estimate_frames")
        b = 0 if stack is None else int(stack.shape[0])
        status = np.where((ff < 0) | (ff >= b), _normalize.STATUS_FRAME_RANGE, g["status"]).astype(np.int32)
        npix = self.patch_size[0] * self.patch_size[1]
        if n == 0 or b == 0:
            inter = (np.zeros((n, npix), dtype=np.float32), np.zeros((n, self.k), dtype=np.float32)) if return_intermediates else (None, None)
            return self._result(np.full((4, n), np.nan), status, *inter)
        out = t.empty((4, n), dtype=t.float64, device=stack.device)
        pt = t.empty((n, npix), dtype=t.float32, device=stack.device) if return_intermediates else None
        ft = t.empty((n, self.k), dtype=t.float32, device=stack.device) if return_intermediates else None
        b, h, w, ld, stride = _normalize.stack_layout(stack)
        _capi.check(_capi.lib().hg_estimator_estimate_frames_device(
            self._handle(), int(flags), stack.data_ptr(), b, stride, h, w, ld, g.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), n, out.data_ptr(), n,
            None if pt is None else pt.data_ptr(), None if ft is None else ft.data_ptr(), t.cuda.current_stream(stack.device).cuda_stream))
        return self._result(out.cpu().numpy(), status, pt, ft)

    def estimate_faces_frames(self, stack, faces, **kw):
        """The list of B (m_b, 10) arrays ``DeviceCascade.detect_faces_frames`` returns, on the stack the cascade read
        (``DeviceCascade.prescale_frames(stack)``), through ONE ``estimate_frames``.  Returns a list of B dicts, each, key for key, what
        ``estimate_faces(stack[b], faces[b])`` returns; a frame without faces gets the dict of ``estimate`` with n = 0.  A list whose
        length is not B raises ValueError."""
        import torch as t
        stack = _normalize.check_grey_stack(t, stack, None, "estimate_faces_frames")
        b = 0 if stack is None else int(stack.shape[0])
        if isinstance(faces, np.ndarray) or not hasattr(faces, "__len__") or len(faces) != b:
            raise ValueError("faces must be the list of %d (m, 10) arrays detect_faces_frames returns, one per frame" % b)
        rows = [np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in faces]
        first = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        eyes = np.concatenate([r[:, 5:9] for r in rows]) if rows else np.zeros((0, 4))
        face_frame = np.repeat(np.arange(b, dtype=np.int32), [len(r) for r in rows]) if rows else np.zeros(0, dtype=np.int32)
        res = self.estimate_frames([] if stack is None else stack, eyes, face_frame, **kw)
        return [{k: v[int(first[f]):int(first[f + 1])] for k, v in res.items()} for f in range(b)]

    def estimate_frame_list(self, frame_list, eyes=None, face_frame=None, geoms=None, return_intermediates=False, flags=0):
        """``estimate`` for faces spread over a list of B frames of DIFFERENT sizes as ONE pooled chain
        (hg_estimator_estimate_frame_list_device: the chain of ``estimate_frames`` with every face normalised from its own frame).
        ``frame_list``: a list of (H, W) grey uint8 device tensors (``normalize.check_grey_list``) — for the rows of
        ``detect_faces_frame_list`` the prescaled frames the cascade read, ``DeviceCascade.prescale_frame_list(frame_list)``; ``eyes``
        (n, 4) in each face's own frame (or ``geoms``, record i for the size of face i's OWN frame); ``face_frame`` (n,) integers, the
        frame of every face, in any order.  Returns the dict of ``estimate_frames`` — face i's values are, bit for bit, those of
        ``estimate(frame_list[face_frame[i]], eyes[i:i + 1])`` — with one device-to-host copy of the (4, n) block, the call's only wait.
        A face whose frame index is outside [0, B) has status ``normalize.STATUS_FRAME_RANGE``, NaN values and ``None`` labels.  An
        empty list or n = 0 touches no library entry."""
        import torch as t
        frame_list = _normalize.check_grey_list(t, frame_list, "estimate_frame_list")      # layout first, then the faces, then the device
        b = 0 if frame_list is None else len(frame_list)
        if geoms is not None:
            g = _normalize._check_geoms(geoms)
            ff = _normalize.check_face_frame(face_frame, int(g.shape[0]))
        else:
            g, ff = self._norm.list_geometry(_normalize.list_sizes(frame_list), eyes, face_frame)
        n = int(g.shape[0])
        _normalize.check_list_device(frame_list, self.device, "estimate_frame_list")
        status = np.where((ff < 0) | (ff >= b), _normalize.STATUS_FRAME_RANGE, g["status"]).astype(np.int32)
        npix = self.patch_size[0] * self.patch_size[1]
        if n == 0 or b == 0:
            inter = (np.zeros((n, npix), dtype=np.float32), np.zeros((n, self.k), dtype=np.float32)) if return_intermediates else (None, None)
            return self._result(np.full((4, n), np.nan), status, *inter)
        dev = frame_list[0].device
        out = t.empty((4, n), dtype=t.float64, device=dev)
        pt = t.empty((n, npix), dtype=t.float32, device=dev) if return_intermediates else None
        ft = t.empty((n, self.k), dtype=t.float32, device=dev) if return_intermediates else None
        refs = _normalize.list_refs(frame_list)
        _capi.check(_capi.lib().hg_estimator_estimate_frame_list_device(
            self._handle(), int(flags), refs, b, g.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), n, out.data_ptr(), n,
            None if pt is None else pt.data_ptr(), None if ft is None else ft.data_ptr(), t.cuda.current_stream(dev).cuda_stream))
        return self._result(out.cpu().numpy(), status, pt, ft)

    def estimate_faces_frame_list(self, frame_list, faces, **kw):
        """The list of B (m_b, 10) arrays ``DeviceCascade.detect_faces_frame_list`` returns, on the frames the cascade read
        (``DeviceCascade.prescale_frame_list(frame_list)``), through ONE ``estimate_frame_list``.  Returns a list of B dicts, each, key
        for key, what ``estimate_faces(frame_list[b], faces[b])`` returns; a frame without faces gets the dict of ``estimate`` with n = 0.
        A list whose length is not B raises ValueError."""
        import torch as t
        frame_list = _normalize.check_grey_list(t, frame_list, "estimate_faces_frame_list")
        b = 0 if frame_list is None else len(frame_list)
        if isinstance(faces, np.ndarray) or not hasattr(faces, "__len__") or len(faces) != b:
            raise ValueError("faces must be the list of %d (m, 10) arrays detect_faces_frame_list returns, one per frame" % b)
        rows = [np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in faces]
        first = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        eyes = np.concatenate([r[:, 5:9] for r in rows]) if rows else np.zeros((0, 4))
        face_frame = np.repeat(np.arange(b, dtype=np.int32), [len(r) for r in rows]) if rows else np.zeros(0, dtype=np.int32)
        res = self.estimate_frame_list([] if frame_list is None else frame_list, eyes, face_frame, **kw)
        return [{k: v[int(first[f]):int(first[f + 1])] for k, v in res.items()} for f in range(b)]

    def estimate_faces(self, frame, faces, **kw):
        """The (n, 10) rows of ``detect_faces`` / ``FaceTracker`` (x0, y0, x1, y1, angle, eyeL_x, eyeL_y, eyeR_x, eyeR_y, confidence) on
        the frame the cascade read: ``estimate(frame, faces[:, 5:9])``."""
        f = np.asarray(faces, dtype=np.float64).reshape(-1, 10)
        return self.estimate(frame, f[:, 5:9], **kw)

    def close(self):
        """Frees the estimator and the patcher it owns; the caller makes sure the device has finished with them.  The flow and the
        classifiers stay the caller's."""
        if self._h is not None:
            _capi.lib().hg_estimator_free(self._h)
            self._h = None
        if self._norm is not None:
            self._norm.close()
            self._norm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
