"""numpy restatement of the eye step and the purge that follow the face cascade (test infrastructure, float64, the reference's
operation order).  The reference is Python 2 over mdp / cuicuilco; what is restated here is its own arithmetic, line by line.
Extraction, networks and regression are injected as callables, as oracle/cascade_restate.py does for the stage loop."""
from __future__ import annotations

import numpy as np


def eye_boxes(box, angle, face_sampling=0.825, eye_sampling=2.3719):
    """compute_approximate_eye_boxes_coordinates(box, face_sampling=0.825, eye_sampling=2.3719, rot_angle=angle), face_analysis.py:61-135
    (its body writes 0.825 and 2.3719 as literals; the arguments equal them).  Returns (eye coordinates, left box, right box)."""
    x0, y0, x1, y1 = (np.float64(v) for v in box)
    fc_x = (x0 + x1) / 2.0                                                       # :89
    fc_y = (y0 + y1) / 2.0                                                       # :90
    mirroring_factor = 1                                                         # :92-93
    rot_angle = np.float64(angle)
    eye_dx = (37.0 / 2.0) * (np.abs(x1 - x0) / 64.0) / (2 * face_sampling)      # :104
    eye_dy = (42.0 / 2.0) * (np.abs(y1 - y0) / 64.0) / (2 * face_sampling)      # :105
    box_width = (np.abs(x1 - x0) / (64.0 * 2 * face_sampling)) * (64 * eye_sampling / 2)   # :109
    box_height = box_width + 0.0                                                 # :111
    rad = rot_angle * np.pi / 180                                                # :115
    eye_right_dx_rotated = eye_dx * np.cos(rad) - eye_dy * np.sin(rad)           # :117
    eye_right_dy_rotated = eye_dy * np.cos(rad) + eye_dx * np.sin(rad)           # :118
    eye_left_dx_rotated = (-1 * eye_dx) * np.cos(rad) - eye_dy * np.sin(rad)     # :119
    eye_left_dy_rotated = eye_dy * np.cos(rad) + (-1 * eye_dx) * np.sin(rad)     # :120
    eye_left_x = fc_x + mirroring_factor * eye_left_dx_rotated                   # :122
    eye_right_x = fc_x + mirroring_factor * eye_right_dx_rotated                 # :123
    eye_left_y = fc_y - eye_left_dy_rotated                                      # :124
    eye_right_y = fc_y - eye_right_dy_rotated                                    # :125
    left = np.array([eye_left_x - box_width / 2.0, eye_left_y - box_height / 2.0, eye_left_x + box_width / 2.0, eye_left_y + box_height / 2.0])
    right = np.array([eye_right_x - box_width / 2.0, eye_right_y - box_height / 2.0, eye_right_x + box_width / 2.0,
                      eye_right_y + box_height / 2.0])                           # :126-133
    return np.array([eye_left_x, eye_left_y, eye_right_x, eye_right_y]), left, right


def all_eye_boxes(boxes, angles):
    """FaceDetectUpdated.py:947-950 for every face: (2n, 4), left boxes then right boxes."""
    L, R = [], []
    for b, a in zip(np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(angles, dtype=np.float64).reshape(-1)):
        _, l, r = eye_boxes(b, a)
        L.append(l)
        R.append(r)
    return np.array(L + R, dtype=np.float64).reshape(-1, 4)


def contrast_stats(patch):
    """The build's exact statistics: N, S1 = sum p, S2 = sum p^2 as integers; mean = S1 / N; std = sqrt((N S2 - S1^2) / (N N))."""
    p = np.asarray(patch).astype(np.int64).reshape(-1)
    n = p.size
    s1, s2 = int(p.sum()), int((p * p).sum())
    return s1 / n, float(np.sqrt((n * s2 - s1 * s1) / (n * n)))


def contrast(patches_u8, target_mean, target_std):
    """image_array_contrast_normalize_avg_std (face_analysis.py:318-327) per patch with the exact statistics above; clipped to [0, 255],
    float32, no re-quantisation."""
    p = np.asarray(patches_u8)
    out = np.empty(p.shape, dtype=np.float32)
    for i in range(len(p)):
        mean, std = contrast_stats(p[i])
        x = p[i].astype(np.float64)
        x -= mean                                                                # :320
        x /= (std / target_std) + 0.00000001                                     # :321-322
        x += target_mean                                                         # :324
        np.clip(x, 0.0, 255.0, x)                                                # :326
        out[i] = x.astype(np.float32)
    return out


def shift_eyes(eye_boxes_lr, angles, reg, eye_sampling=2.3719, regression_size=(64.0, 64.0), tolerance=9.0):
    """find_Left_Right_eyes after its networks (face_analysis.py:1073-1104, left_eye = 1 for both eyes — find_Right_eyes passes the
    unswapped box, :1022-1033) and the eye centres (FaceDetectUpdated.py:1008-1009).  eye_boxes_lr (2n, 4); reg (2, 2n) EyeLX / EyeLY.
    Returns (eye coordinates (n, 4), too_far (n))."""
    n = len(angles)
    angles = np.asarray(angles, dtype=np.float64)
    reg = np.asarray(reg, dtype=np.float64)
    centres, far = [], np.zeros(n, dtype=bool)
    for side in (0, 1):
        box = np.array(eye_boxes_lr[side * n:(side + 1) * n], dtype=np.float64).reshape(-1, 4)
        rx, ry = reg[0, side * n:(side + 1) * n], reg[1, side * n:(side + 1) * n]
        far |= np.abs(rx) >= tolerance                                           # :1073
        far |= np.abs(ry) >= tolerance
        reg_out_x = (rx / eye_sampling) * np.abs(box[:, 2] - box[:, 0]) / regression_size[0]    # :1079-1080
        reg_out_y = (ry / eye_sampling) * np.abs(box[:, 3] - box[:, 1]) / regression_size[1]    # :1084-1085
        factor = 1
        rot = -1 * factor * angles * np.pi / 180                                 # :1096
        dx = reg_out_x * np.cos(rot) - reg_out_y * np.sin(rot)                   # :1097
        dy = reg_out_y * np.cos(rot) + reg_out_x * np.sin(rot)                   # :1098
        box[:, 0] = box[:, 0] - factor * dx                                      # :1100
        box[:, 2] = box[:, 2] - factor * dx                                      # :1101
        box[:, 1] = box[:, 1] - dy                                               # :1103
        box[:, 3] = box[:, 3] - dy                                               # :1104
        centres.append((box[:, 0:2] + box[:, 2:4]) / 2.0)                        # FaceDetectUpdated.py:1008-1009
    return np.concatenate(centres, axis=1), far


def eye_step(frame, coords, angles, extract, execute, regress, contrast_targets):
    """FaceDetectUpdated.py:947-1009 for the survivors of a frame: extract(frame, eye_boxes (2n, 4), delta_angs (2n)) -> uint8 patches;
    execute(patches float32) -> features; regress(s, features) -> regression of classifier s (0 EyeLX, 1 EyeLY).  The two stages share
    one flow in the reference's pipeline, so one execute over the 2n rows stands for its four (rows are independent)."""
    n = len(angles)
    eb = all_eye_boxes(coords, angles)
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0, dtype=bool), eb, np.zeros((2, 0))
    dang = -1 * np.concatenate([angles, angles]).astype(np.float64)             # face_analysis.py:1042
    patches = contrast(extract(frame, eb, dang), *contrast_targets)
    sl = execute(patches)
    reg = np.stack([regress(0, sl), regress(1, sl)])
    ec, far = shift_eyes(eb, angles, reg)
    return ec, far, eb, reg


def assemble_rows(coords, angles, confidence, eye_coords, too_far):
    """FaceDetectUpdated.py:1010-1017 (discard, order kept) and :1036-1041 (one row per face)."""
    keep = ~np.asarray(too_far, dtype=bool)
    rows = [np.array([b[0], b[1], b[2], b[3], a, e[0], e[1], e[2], e[3], c]) for b, a, e, c in
            zip(np.asarray(coords)[keep], np.asarray(angles)[keep], np.asarray(eye_coords)[keep], np.asarray(confidence)[keep])]
    return np.array(rows, dtype=np.float64).reshape(-1, 10)


def relative_error_detection(app_eye_coords, eye_coords):
    """face_analysis.py:158-165 (Python's max() on numpy scalars, numpy's division by zero)."""
    dist_left = eye_coords[0:2] - app_eye_coords[0:2]
    dist_left = np.sqrt((dist_left ** 2).sum())
    dist_right = eye_coords[2:4] - app_eye_coords[2:4]
    dist_right = np.sqrt((dist_right ** 2).sum())
    dist_eyes = eye_coords[0:2] - eye_coords[2:4]
    dist_eyes = np.sqrt((dist_eyes ** 2).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(dist_left, dist_right) / dist_eyes


def literal_min_error(app, kept):
    """face_analysis.py:213-217 as written: min_d starts at 10000 and moves on error < min_d only (a NaN error never moves it)."""
    min_d = 10000
    for k in kept:
        error = relative_error_detection(app, k)
        if error < min_d:
            min_d = error
    return min_d


def min_error(app, kept):
    """The same over all kept rows at once, element for element the same operations (a two-element .sum() is one addition; Python's
    max(a, b) is b only where b > a); tests/test_eyes_host.py checks it against literal_min_error."""
    with np.errstate(divide="ignore", invalid="ignore"):
        l0, l1 = kept[:, 0] - app[0], kept[:, 1] - app[1]
        r0, r1 = kept[:, 2] - app[2], kept[:, 3] - app[3]
        e0, e1 = kept[:, 0] - kept[:, 2], kept[:, 1] - kept[:, 3]
        dl, dr, de = np.sqrt(l0 ** 2 + l1 ** 2), np.sqrt(r0 ** 2 + r1 ** 2), np.sqrt(e0 ** 2 + e1 ** 2)
        err = np.where(dr > dl, dr, dl) / de
    err = err[err < 10000]
    return err.min() if len(err) else 10000


def purge(rows, literal=False):
    """purgue_detected_faces_angles_eyes_confidence (face_analysis.py:186-221), weight_confidences_by_area=True, with the build's tie
    rule: numpy.argsort(w, kind="stable")[::-1] (the reference's default argsort is not stable)."""
    d = np.array(rows, dtype=np.float64).reshape(-1, 10)
    if len(d) > 1:                                                               # :191
        conf = d[:, -1]                                                          # :192
        with np.errstate(divide="ignore", invalid="ignore"):
            areas = ((d[:, 7] - d[:, 5]) ** 2 + (d[:, 8] - d[:, 6]) ** 2) ** 0.5  # :195-196
            w = (1.0 - conf) * areas                                             # :197
            w = w / w.max()                                                      # :198
        order = np.argsort(w, kind="stable")[::-1]                              # :201 (tie rule pinned)
        d = d[order, :]                                                          # :203
        unique = np.empty((len(d) + 1, 10))
        unique[0] = d[0]                                                         # :210-211
        nk = 1
        for row in d:                                                            # :212
            min_d = min_error(row[5:9], unique[:nk, 5:9]) if literal is False else literal_min_error(row[5:9], unique[:nk, 5:9])
            if min_d > 0.25:                                                     # :218
                unique[nk] = row
                nk += 1
        return unique[:nk].copy()
    return d.copy()                                                              # :220-221
