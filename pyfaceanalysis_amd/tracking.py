"""Tracking faces across a stream of frames: the reference's ``track_single_face`` mode on the device, and the same for several faces.

Once a frame has produced a face, its first purged detection is carried over (FaceDetectUpdated.py:1189-1195); the next frame then
searches nine windows around that box instead of the whole pyramid — one sampling value from the box's size (face_analysis.py:576-585),
the box and one separation step to either side (:611-623).  When a tracked frame finds nothing, the following frame returns to the full
grid.  ``FaceTracker`` holds that state in the library (include/higsfa.h ``hg_tracker``): the tracked box never leaves the device — the
purge writes it, the next frame's grid kernel reads it — and a tracked frame is enqueued as a whole, every launch sized by the bound 9,
with one host wait at the end.  ``grid.tracked_boxes`` / ``cascade.tracked_windows`` are the host restatement of the
nine windows.

Several faces (``max_faces`` > 1): the first ``max_faces`` purged detections with a finite box are carried, in purge order, and a
tracked frame searches the nine windows of EVERY held face in one pooled pass — 9 K windows under the bound 9 K, one purge over the
union of their rows, one host wait.  Every returned row names the held face it came from (``slots``).  ``rescan_every`` = R sends
every R-th + 1 step back to the full grid, where new faces can enter (include/higsfa.h ``hg_tracker_create_multi``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, grid
from . import frames as frames_mod
from .cascade import frame_levels

N_TRACKED = 9          # windows of a tracked frame per held face: 3 posX values x 3 (equal) posY values
MAX_FACES = 64         # the library's cap (hg_tracker_create_multi)


def tracked_consts(cascade):
    """``hg_tracked_consts`` of a ``DeviceCascade``: its sub-image size and its pipeline's regression size and separations."""
    p = cascade.pipeline
    tc = _capi.HgTrackedConsts()
    tc.subimage_width, tc.subimage_height = cascade.w, cascade.h
    tc.regression_width, tc.regression_height = p["regression_width"], p["regression_height"]
    tc.net_Dx, tc.net_Dy = p["net_Dx"], p["net_Dy"]
    return tc


class FaceTracker(object):
    """Up to ``max_faces`` faces (1..64) followed through a stream of frames, on ``cascade`` (a ``DeviceCascade``) and ``eyes`` (an
    ``EyeLocator``) of one device.  Both stay owned by the caller and must outlive the tracker; while the tracker is in use they serve
    one stream at a time (a ``detect_faces`` between two steps is fine, one in flight during a step is not).  ``rescan_every`` = R > 0:
    after R consecutive tracked steps the next step searches the full grid again (0: only when every face is lost, as the reference)."""

    def __init__(self, cascade, eyes, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE, max_faces=1, rescan_every=0):
        self.max_faces, self.rescan_every = int(max_faces), int(rescan_every)
        self._multi = self.max_faces != 1 or self.rescan_every != 0      # the defaults: hg_tracker_create and today's dict
        if eyes.device != cascade.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, cascade.device))
        self.cascade, self.eyes = cascade, eyes
        self.smallest_face, self.prescale_size = float(smallest_face), int(prescale_size or 0)
        self.torch = cascade.torch
        self._plans = {}       # frame size -> everything a step needs that depends on the size alone
        self._boxes = np.zeros((0, 4))
        self._h = None
        tc = tracked_consts(cascade)
        h = C.c_void_p()
        if self._multi:
            _capi.check(_capi.lib().hg_tracker_create_multi(cascade._handle(), eyes._handle(), C.byref(tc), self.max_faces, self.rescan_every, C.byref(h)))
        else:
            _capi.check(_capi.lib().hg_tracker_create(cascade._handle(), eyes._handle(), C.byref(tc), C.byref(h)))
        self._h = h

    @property
    def tracked_face(self):
        """Host copy of the first tracked box (x0, y0, x1, y1), in the coordinates of the prescaled frame it was found on, or None."""
        return self._boxes[0].copy() if len(self._boxes) else None

    @property
    def tracked_faces(self):
        """Host copy of the held boxes, (n_held, 4) in carried order — the order ``slots`` of the next step refers to — or (0, 4)."""
        return self._boxes.copy()

    def step(self, frame):
        """One frame of the stream ((H, W) uint8 tensor on the device, contiguous rows — or a colour frame of the cascade's
        ``frame_format``; checked on every call).  Returns faces (m, 10)
        as ``DeviceCascade.detect_faces``, tracked (this frame used the nine-window grid), n_windows (9 per held face then, else the
        grid's count), n_before_purge, counts (-1 throughout on a tracked frame: no count left the device) and rows_executed.  With
        ``max_faces`` > 1 or ``rescan_every`` > 0 also slots (int32, one per face row: the held face — index into ``tracked_faces``
        as it was BEFORE this step — whose windows produced the row; -1 on a full-grid step) and n_held (faces carried to the next step)."""
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
            n_rows_max = max(n0, N_TRACKED * self.max_faces) + 1      # the purge may keep n + 1 rows
            rows, counts = np.empty((n_rows_max, 10)), np.zeros(len(dc.stages), dtype=np.int32)
            plan = self._plans[(fw, fh)] = (pre, levels, n_levels, n0, rows, counts, np.empty(n_rows_max, dtype=np.int32))
        pre, levels, n_levels, n0, rows, counts, slots = plan
        n_out, n_before, n_rows, used, n_held = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        held_before = len(self._boxes)
        head = (self._h, frame.data_ptr(), fh, fw, frame.stride(0), pre[0], pre[1], levels, n_levels, rows.ctypes.data_as(C.c_void_p), len(rows),
                C.byref(n_out), C.byref(n_before), counts.ctypes.data_as(C.c_void_p), C.byref(n_rows), C.byref(used))
        stream = t.cuda.current_stream(dc.dev).cuda_stream
        try:
            if self._multi:
                _capi.check(L.hg_tracker_step_frame_multi_device(*(head + (slots.ctypes.data_as(C.c_void_p), C.byref(n_held), stream))))
            else:
                _capi.check(L.hg_tracker_step_frame_device(*(head + (stream,))))
        except Exception:
            self.reset()
            raise
        faces = rows[:n_out.value].copy()
        # the library's rule (k_tracker_handover): of the first max_faces rows those with a finite box are carried, in order
        cand = faces[:self.max_faces, :4]
        self._boxes = cand[np.isfinite(cand).all(axis=1)].copy()
        tracked = bool(used.value)
        res = dict(faces=faces, tracked=tracked, n_windows=N_TRACKED * held_before if tracked else n0, n_before_purge=n_before.value,
                   counts=counts.tolist(), rows_executed=n_rows.value)
        if self._multi:
            if n_held.value != len(self._boxes):
                raise RuntimeError("tracker holds %d faces, the rows say %d" % (n_held.value, len(self._boxes)))
            res["slots"], res["n_held"] = slots[:n_out.value].copy(), n_held.value
        return res

    def reset(self):
        """Forget the tracked face: the next step searches the full grid."""
        if self._h is not None:
            _capi.check(_capi.lib().hg_tracker_reset(self._h))
        self._boxes = np.zeros((0, 4))

    def close(self):
        if self._h is not None:
            _capi.lib().hg_tracker_free(self._h)
            self._h = None
        self._boxes = np.zeros((0, 4))


class StreamSetTracker(object):
    """``n_streams`` frame streams tracked in ONE pooled step per frame time (include/higsfa.h ``hg_stream_tracker``).
    Stream ``s`` behaves exactly as a ``FaceTracker(cascade, eyes, smallest_face, prescale_size, max_faces, rescan_every)`` of its own that
    is fed ``frames[s]`` step after step: the same boxes in the same carried order, the same path rule (the full grid when the stream
    holds nothing, or after ``rescan_every`` tracked steps in a row, counted per stream), the same hand-over rule; when the prescaled
    size changes, every stream drops its boxes.  The streams on the tracked path share one pass — the nine windows of every held face
    of every such stream under one bound, the eye step as one batch, the purge per stream, one host wait — and the others one full-grid
    pass (``detect_faces_frames`` on their frames).  ``cascade`` and ``eyes`` stay owned by the caller and serve one call at a time.
    9 * n_streams * max_faces may not exceed 8192 (``_capi.HG_MAX_STREAM_WINDOWS``: the bounded stage loop's single-workgroup path)."""

    def __init__(self, cascade, eyes, n_streams, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE, max_faces=1, rescan_every=0):
        self.n_streams, self.max_faces, self.rescan_every = int(n_streams), int(max_faces), int(rescan_every)
        # the library's own refusals (hg_stream_tracker_create), stated here as well: the handle is created at the first step
        if not 1 <= self.n_streams <= _capi.HG_MAX_STACK_FRAMES:
            raise ValueError("n_streams %d outside 1..%d" % (self.n_streams, _capi.HG_MAX_STACK_FRAMES))
        if not 1 <= self.max_faces <= MAX_FACES:
            raise ValueError("max_faces %d outside 1..%d" % (self.max_faces, MAX_FACES))
        if N_TRACKED * self.n_streams * self.max_faces > _capi.HG_MAX_STREAM_WINDOWS:
            raise ValueError("%d streams of %d faces: %d tracked windows, at most %d" %
                             (self.n_streams, self.max_faces, N_TRACKED * self.n_streams * self.max_faces, _capi.HG_MAX_STREAM_WINDOWS))
        if self.rescan_every < 0:
            raise ValueError("negative rescan_every %d" % self.rescan_every)
        if eyes.device != cascade.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, cascade.device))
        self.cascade, self.eyes = cascade, eyes
        self.smallest_face, self.prescale_size = float(smallest_face), int(prescale_size or 0)
        self.torch = cascade.torch
        self._plans = {}       # frame size -> everything a step needs that depends on the size alone
        self._boxes = [np.zeros((0, 4)) for _ in range(self.n_streams)]
        self._h = None
        self._closed = False

    def _handle(self):
        if self._closed:
            raise RuntimeError("tracker is closed")
        if self._h is None:
            tc, h = tracked_consts(self.cascade), C.c_void_p()
            _capi.check(_capi.lib().hg_stream_tracker_create(self.cascade._handle(), self.eyes._handle(), C.byref(tc), self.n_streams, self.max_faces,
                                                             self.rescan_every, C.byref(h)))
            self._h = h
        return self._h

    def tracked_faces(self, s):
        """Host copy of stream ``s``'s held boxes, (n_held, 4) in carried order — the order ``slots`` of its next step refers to."""
        return self._boxes[range(self.n_streams)[s]].copy()

    def step(self, frames):
        """One frame per stream: a (n_streams, H, W) uint8 tensor on the cascade's device with unit pixel stride — rows and frames may be
        pitched, as for ``detect_frames`` — or a colour stack of the cascade's ``frame_format``, or a list of such frames; checked on
        every call.  Returns streams (a list of n_streams dicts: faces (m, 10), tracked, n_windows — 9 per face held before the step,
        else the grid's count — n_before_purge, slots (int32, one per row: index into ``tracked_faces(s)`` as it was BEFORE this step;
        -1 on a full-grid step) and n_held, each as in ``FaceTracker.step``), rows_executed, and n_tracked / n_grid, the streams that
        took each path.  If the step raises, every stream is reset."""
        if self._closed:
            raise RuntimeError("tracker is closed")
        t, dc = self.torch, self.cascade
        n_given = len(frames) if isinstance(frames, (list, tuple)) else (int(frames.shape[0]) if isinstance(frames, t.Tensor) and frames.dim() else -1)
        if n_given >= 0 and n_given != self.n_streams:      # the length before the device, like every other property of the stack
            raise ValueError("%d frames for a set of %d streams" % (n_given, self.n_streams))
        stack = dc._check_stack(frames)
        if stack is None or int(stack.shape[0]) != self.n_streams:
            raise ValueError("%d frames for a set of %d streams" % (0 if stack is None else int(stack.shape[0]), self.n_streams))
        b, fh, fw = self.n_streams, int(stack.shape[1]), int(stack.shape[2])
        plan = self._plans.get((fw, fh))
        if plan is None:
            pw, ph = grid.prescaled_size(fw, fh, self.prescale_size) if self.prescale_size else (fw, fh)
            pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
            levels, n_levels, n0 = frame_levels(pw, ph, self.smallest_face, dc.pipeline, (dc.w, dc.h))
            n_rows_max = b * (max(n0, N_TRACKED * self.max_faces) + 1)      # the purge may keep n + 1 rows of every stream
            ints = lambda n: np.zeros(n, dtype=np.int32)
            plan = self._plans[(fw, fh)] = (pre, levels, n_levels, n0, np.empty((n_rows_max, 10)), ints(n_rows_max), ints(b + 1), ints(b), ints(b), ints(b))
        pre, levels, n_levels, n0, rows, slots, first, before, used, held = plan
        c = frames_mod.CHANNELS[dc.frame_format]
        ld = stack.stride(1) if fh > 1 else fw * c
        stride = stack.stride(0) if b > 1 else (fh - 1) * ld + fw * c
        held_before = [len(x) for x in self._boxes]
        n_rows = C.c_int64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        try:
            _capi.check(_capi.lib().hg_stream_tracker_step_frames_device(
                self._handle(), stack.data_ptr(), b, stride, fh, fw, ld, pre[0], pre[1], levels, n_levels, vp(rows), len(rows), vp(first), vp(before), vp(used),
                vp(held), vp(slots), C.byref(n_rows), t.cuda.current_stream(dc.dev).cuda_stream))
        except Exception:
            self.reset()
            raise
        streams = []
        for s in range(b):
            lo, hi = int(first[s]), int(first[s + 1])
            faces = rows[lo:hi].copy()
            # the library's rule (k_stream_handover): of the first max_faces rows those with a finite box are carried, in order
            cand = faces[:self.max_faces, :4]
            self._boxes[s] = cand[np.isfinite(cand).all(axis=1)].copy()
            if int(held[s]) != len(self._boxes[s]):
                self.reset()
                raise RuntimeError("stream %d holds %d faces, the rows say %d" % (s, int(held[s]), len(self._boxes[s])))
            tracked = bool(used[s])
            streams.append(dict(faces=faces, tracked=tracked, n_windows=N_TRACKED * held_before[s] if tracked else n0, n_before_purge=int(before[s]),
                                slots=slots[lo:hi].copy(), n_held=int(held[s])))
        n_tracked = sum(x["tracked"] for x in streams)
        return dict(streams=streams, rows_executed=n_rows.value, n_tracked=n_tracked, n_grid=b - n_tracked)

    def reset(self, s=None):
        """Forget the faces of stream ``s`` (its next step searches the full grid), or of every stream (``None``)."""
        if s is None:
            if self._h is not None:
                _capi.check(_capi.lib().hg_stream_tracker_reset(self._h, -1))
            self._boxes = [np.zeros((0, 4)) for _ in range(self.n_streams)]
            return
        s = range(self.n_streams)[s]
        if self._h is not None:
            _capi.check(_capi.lib().hg_stream_tracker_reset(self._h, s))
        self._boxes[s] = np.zeros((0, 4))

    def close(self):
        if self._h is not None:
            _capi.lib().hg_stream_tracker_free(self._h)
            self._h = None
        self._closed = True
        self._boxes = [np.zeros((0, 4)) for _ in range(self.n_streams)]
