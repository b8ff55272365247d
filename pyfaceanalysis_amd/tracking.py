"""Tracking one face across a stream of frames: the reference's ``track_single_face`` mode on the device.

Once a frame has produced a face, its first purged detection is carried over (FaceDetectUpdated.py:1189-1195); the next frame then
searches nine windows around that box instead of the whole pyramid — one sampling value from the box's size (face_analysis.py:576-585),
the box and one separation step to either side (:611-623).  When a tracked frame finds nothing, the following frame returns to the full
grid.  ``FaceTracker`` holds that state in the library (include/higsfa.h ``hg_tracker``): the tracked box never leaves the device — the
purge writes it, the next frame's grid kernel reads it — and a tracked frame is enqueued as a whole, every launch sized by the bound 9,
with one host wait at the end.  ``grid.tracked_boxes`` / ``cascade.tracked_windows`` are the host restatement of the
nine windows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, grid
from .cascade import frame_levels

N_TRACKED = 9          # windows of a tracked frame: 3 posX values x 3 (equal) posY values


class FaceTracker(object):
    """One face followed through a stream of frames, on ``cascade`` (a ``DeviceCascade``) and ``eyes`` (an ``EyeLocator``) of one device.
    Both stay owned by the caller and must outlive the tracker; while the tracker is in use they serve one stream at a time (a
    ``detect_faces`` between two steps is fine, one in flight during a step is not)."""

    def __init__(self, cascade, eyes, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        if eyes.device != cascade.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, cascade.device))
        self.cascade, self.eyes = cascade, eyes
        self.smallest_face, self.prescale_size = float(smallest_face), int(prescale_size or 0)
        self.torch = cascade.torch
        self._plans = {}       # frame size -> everything a step needs that depends on the size alone
        self._box = None
        self._h = None
        p = cascade.pipeline
        tc = _capi.HgTrackedConsts()
        tc.subimage_width, tc.subimage_height = cascade.w, cascade.h
        tc.regression_width, tc.regression_height = p["regression_width"], p["regression_height"]
        tc.net_Dx, tc.net_Dy = p["net_Dx"], p["net_Dy"]
        h = C.c_void_p()
        _capi.check(_capi.lib().hg_tracker_create(cascade._handle(), eyes._handle(), C.byref(tc), C.byref(h)))
        self._h = h

    @property
    def tracked_face(self):
        """Host copy of the tracked box (x0, y0, x1, y1), in the coordinates of the prescaled frame it was found on, or None."""
        return None if self._box is None else self._box.copy()

    def step(self, frame):
        """One frame of the stream ((H, W) uint8 tensor on the device, contiguous rows — or a colour frame of the cascade's
        ``frame_format``; checked on every call).  Returns faces (m, 10)
        as ``DeviceCascade.detect_faces``, tracked (this frame used the nine-window grid), n_windows (9 then, else the grid's count),
        n_before_purge, counts (-1 throughout on a tracked frame: no count left the device) and rows_executed."""
        if self._h is None:
            raise RuntimeError("tracker is closed")
        t, L, dc = self.torch, _capi.lib(), self.cascade
        dc._check_frame(frame)
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        plan = self._plans.get((fw, fh))
        if plan is None:
            pw, ph = grid.prescaled_size(fw, fh, self.prescale_size) if self.prescale_size else (fw, fh)
            pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
            levels, n_levels, n0 = frame_levels(pw, ph, self.smallest_face, dc.pipeline, (dc.w, dc.h))
            rows, counts = np.empty((max(n0, N_TRACKED) + 1, 10)), np.zeros(len(dc.stages), dtype=np.int32)      # the purge may keep n + 1 rows
            plan = self._plans[(fw, fh)] = (pre, levels, n_levels, n0, rows, counts)
        pre, levels, n_levels, n0, rows, counts = plan
        n_out, n_before, n_rows, used = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        try:
            _capi.check(L.hg_tracker_step_frame_device(
                self._h, frame.data_ptr(), fh, fw, frame.stride(0), pre[0], pre[1], levels, n_levels, rows.ctypes.data_as(C.c_void_p), len(rows),
                C.byref(n_out), C.byref(n_before), counts.ctypes.data_as(C.c_void_p), C.byref(n_rows), C.byref(used),
                t.cuda.current_stream(dc.dev).cuda_stream))
        except Exception:
            self.reset()
            raise
        faces = rows[:n_out.value].copy()
        # the library's rule (hg_tracker_step_frame_device): row 0's box is carried if there is a row and the box is finite
        self._box = faces[0, :4].copy() if len(faces) and np.isfinite(faces[0, :4]).all() else None
        tracked = bool(used.value)
        return dict(faces=faces, tracked=tracked, n_windows=N_TRACKED if tracked else n0, n_before_purge=n_before.value,
                    counts=counts.tolist(), rows_executed=n_rows.value)

    def reset(self):
        """Forget the tracked face: the next step searches the full grid."""
        if self._h is not None:
            _capi.check(_capi.lib().hg_tracker_reset(self._h))
        self._box = None

    def close(self):
        if self._h is not None:
            _capi.lib().hg_tracker_free(self._h)
            self._h = None
        self._box = None
