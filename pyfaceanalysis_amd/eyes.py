"""Eye localisation and the purge of repeated detections, after the face cascade, on one GPU.

What the reference does per image once the face stages are done (FaceDetectUpdated.py:947-1041, :1180):

    eye boxes = compute_approximate_eye_boxes_coordinates(box, 0.825, 2.3719, rot_angle=angle)   :947-950 (face_analysis.py:61-135)
    find_Left_eyes / find_Right_eyes: 64x64 patches -> EyeLX / EyeLY networks -> regression     :992-1004 (face_analysis.py:1018-1109)
    discard of the faces whose eyes moved too far, eye centres                                   :1006-1017
    rows (x0, y0, x1, y1, angle, eyeL_x, eyeL_y, eyeR_x, eyeR_y, confidence)                      :1036-1041
    purgue_detected_faces_angles_eyes_confidence                                                   :1180 (face_analysis.py:186-221)

``EyeLocator`` holds the two eye stages (include/higsfa.h ``hg_eyes_create``); ``locate`` runs the eye step on given faces and returns
what it found BEFORE the discard; ``purge_detections`` runs the purge on the device; ``DeviceCascade.detect_faces`` does all of it
after the cascade in one host call.  The contrast targets have no default: how the reference's obj_avg = 0.11 / obj_std = 0.15 map to
pixel units is not known.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

FACE_SAMPLING = 0.825          # FaceDetectUpdated.py:948
EYE_SAMPLING = 2.3719          # FaceDetectUpdated.py:948, face_analysis.py:1080
TOLERANCE_XY_EYE = 9.0         # face_analysis.py:1018


class EyeLocator(object):
    def __init__(self, flow_x, clf_x, flow_y, clf_y, *, contrast, eye_size=(64, 64), regression_size=(64, 64), tolerance=TOLERANCE_XY_EYE,
                 n_features=None, device=0, interpolation=0):
        """interpolation: the filter of the eye patches (PIL's codes 0 / 2 / 3) — the reference passes what its stage loop's last
        iteration left in interpolation_format (FaceDetectUpdated.py:671, :994)."""
        import torch
        self.interpolation = _capi.filter_code(interpolation)
        self.torch = torch
        self.flow_x, self.clf_x, self.flow_y, self.clf_y = flow_x, clf_x, flow_y, clf_y
        self.contrast = (float(contrast[0]), float(contrast[1]))
        self.w, self.h = int(eye_size[0]), int(eye_size[1])
        self.regression_size = (float(regression_size[0]), float(regression_size[1]))
        self.tolerance = float(tolerance)
        self.k = int(max(clf_x.input_dim, clf_y.input_dim) if n_features is None else n_features)
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        for name, f in (("flow_x", flow_x), ("flow_y", flow_y)):
            if f.device != self.device or f.output_dtype != np.float32:
                raise ValueError("%s must live on device %d with output_dtype float32" % (name, self.device))
            if f.input_dim != self.w * self.h:
                raise ValueError("%s reads %d columns, eye patches have %d x %d" % (name, f.input_dim, self.w, self.h))
            if f.output_dim < self.k:
                raise ValueError("%s gives %d features, %d kept" % (name, f.output_dim, self.k))
        for name, c in (("clf_x", clf_x), ("clf_y", clf_y)):
            if c.input_dim > self.k:
                raise ValueError("%s reads %d features, %d kept" % (name, c.input_dim, self.k))
            if c.avg_labels is None:
                raise ValueError("%s needs avg_labels" % name)
        self._h = None
        self._gray = None        # locate(frame_format=...): the converted frame, reused while the frame size stays

    def consts(self):
        c = _capi.HgEyeConsts()
        c.eye_regression_width, c.eye_regression_height = self.regression_size
        c.face_sampling, c.eye_sampling, c.tolerance = FACE_SAMPLING, EYE_SAMPLING, self.tolerance
        c.target_mean, c.target_std = self.contrast
        c.eye_w, c.eye_h, c.n_features, c.reserved = self.w, self.h, self.k, 0
        return c

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            cc = self.consts()
            _capi.check(_capi.lib().hg_eyes_create(self.flow_x._handle().h, self.clf_x._handle(self.clf_x.avg_labels), self.flow_y._handle().h,
                                                   self.clf_y._handle(self.clf_y.avg_labels), C.byref(cc), self.device, C.byref(h)))
            self._h = h
            if self.interpolation != _capi.HG_FILTER_NEAREST:
                _capi.check(_capi.lib().hg_eyes_set_interpolation(h, self.interpolation))
        return self._h

    def _faces(self, boxes, angles):
        t = self.torch
        b = t.as_tensor(np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4), device=self.dev)
        a = t.as_tensor(np.ascontiguousarray(angles, dtype=np.float64).reshape(-1), device=self.dev)
        if a.shape[0] != b.shape[0]:
            raise ValueError("one angle per box")
        return b, a

    def eye_boxes(self, boxes, angles):
        """The eye boxes (2n, 4) of n faces, left boxes then right boxes (hg_eyes_boxes_device)."""
        t = self.torch
        b, a = self._faces(boxes, angles)
        n = b.shape[0]
        out = t.empty((2 * n, 4), dtype=t.float64, device=self.dev)
        _capi.check(_capi.lib().hg_eyes_boxes_device(self._handle(), b.data_ptr(), a.data_ptr(), n, out.data_ptr(), None,
                                                     t.cuda.current_stream(self.dev).cuda_stream))
        return out.cpu().numpy()

    def locate(self, frame, boxes, angles, return_patches=False, frame_format="L"):
        """The eye step for n faces on ``frame`` ((H, W) uint8 tensor on this device, contiguous rows), BEFORE the discard.  Host
        arrays: eye_coords (n, 4) = (eyeL_x, eyeL_y, eyeR_x, eyeR_y), too_far (n) bool, reg (2, 2n) — EyeLX / EyeLY regressions, left
        eyes then right eyes — and with return_patches the contrast-normalised patches (2n, w*h) float32.  frame_format: a colour
        frame (frames.py) is first converted as PIL's ``convert("L")`` does, into a buffer that lives with the locator."""
        from . import frames
        t = self.torch
        if frames.check_color_frame(t, frame, frame_format, self.dev) != _capi.HG_FRAME_L:
            if self._gray is None or tuple(self._gray.shape) != tuple(frame.shape[:2]):
                self._gray = t.empty(tuple(frame.shape[:2]), dtype=t.uint8, device=self.dev)
            frame = frames.to_gray(frame, frame_format, out=self._gray)
        b, a = self._faces(boxes, angles)
        n = b.shape[0]
        ec = t.empty((n, 4), dtype=t.float64, device=self.dev)
        tf = t.empty(n, dtype=t.uint8, device=self.dev)
        reg = t.empty((2, 2 * n), dtype=t.float64, device=self.dev)
        pt = t.empty((2 * n, self.w * self.h), dtype=t.float32, device=self.dev) if return_patches else None
        _capi.check(_capi.lib().hg_eyes_locate_device(
            self._handle(), frame.data_ptr(), int(frame.shape[0]), int(frame.shape[1]), frame.stride(0), b.data_ptr(), a.data_ptr(), n,
            ec.data_ptr(), tf.data_ptr(), None if pt is None else pt.data_ptr(), reg.data_ptr(), t.cuda.current_stream(self.dev).cuda_stream))
        out = dict(eye_coords=ec.cpu().numpy(), too_far=tf.cpu().numpy().astype(bool), reg=reg.cpu().numpy())
        if pt is not None:
            out["patches"] = pt.cpu().numpy()
        return out

    def close(self):
        if self._h is not None:
            _capi.lib().hg_eyes_free(self._h)
            self._h = None


def check_frame(t, frame, dev):
    if not isinstance(frame, t.Tensor) or frame.dim() != 2 or frame.dtype != t.uint8 or frame.device != dev or frame.stride(1) != 1:
        raise ValueError("frame must be a 2-d uint8 tensor on %s with contiguous rows" % (dev,))


def assemble_rows(coords, angles, confidence, eye_coords, too_far):
    """The discard of the too-far faces, order kept (FaceDetectUpdated.py:1010-1017), and one row per face (:1036-1041)."""
    keep = ~np.asarray(too_far, dtype=bool)
    return np.concatenate([np.asarray(coords)[keep], np.asarray(angles)[keep, None], np.asarray(eye_coords)[keep],
                           np.asarray(confidence)[keep, None]], axis=1).reshape(-1, 10)


def purge_detections(rows, device=0):
    """purgue_detected_faces_angles_eyes_confidence (face_analysis.py:186-221) on the device (hg_purge_detections_device): rows (n, 10)
    -> the kept rows, in the order of numpy.argsort(w, kind="stable")[::-1]."""
    import torch
    dev = torch.device("cuda", int(device))
    r = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 10), device=dev)
    n = r.shape[0]
    out = torch.empty((n + 1, 10), dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(_capi.lib().hg_purge_detections_device(int(device), r.data_ptr(), n, out.data_ptr(), cnt.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream))
    return out[:int(cnt.item())].cpu().numpy()
