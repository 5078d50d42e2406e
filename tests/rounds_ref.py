"""Restatement of the detection rounds of include/lfdmi.h ("detection rounds"): a round is a detector called on the frame with
the bands of the lines so far set to +0 (tests/mask_ref.py's membership, cap = +inf), ``dup_of`` is the trail masks' step-3 u of
a record's end points against an earlier record's segment.  The detector is a parameter: ``oracle_detect`` wraps the oracle's
``detect_frame``; the hand-made cases of test_rounds_ref.py pass scripted ones."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as MR  # noqa: E402

RESULT_DTYPE = np.dtype([("status", "<i4"), ("found", "<i4"), ("rho", "<f4"), ("theta", "<f4"),
                         ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"),
                         ("n_lines_equ", "<i4"), ("n_lines_box", "<i4"), ("detection", "<i4"),
                         ("rejected_by_theta", "<i4")])
MAX_TRAILS = 8
DEFAULTS = {"max_trails": 4, "half": 10.0, "dup_dist": 20.0}


def found(r):
    return int(r["status"]) == 0 and int(r["found"]) != 0


def record(**kw):
    r = np.zeros(1, RESULT_DTYPE)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def band_segment(r, half):
    """the trail masks' segment of a record: its end points as doubles, cap = +inf"""
    return MR.segment(0, float(r["x1"]), float(r["y1"]), float(r["x2"]), float(r["y2"]), half=half, cap=np.inf)


def band(r, half, h, w):
    """bool [h, w], buffer rows: the pixels of record r's band (all False for a segment the masks call bad)"""
    m = MR.inside(band_segment(r, half), h, w)
    return np.zeros((h, w), bool) if m is None else m


def blotted(frame, recs, half):
    """step 3: the native float32 frame with the band of every record in recs set to +0"""
    out = np.array(frame, dtype=np.float32, copy=True)
    for r in recs:
        out[band(r, half, *out.shape)] = np.float32(0.0)
    return out


def dup_of(recs, k, dup_dist):
    """step 4 for record k of one frame's records"""
    if k == 0 or not found(recs[k]):
        return -1
    ends = ((np.float64(recs[k]["x1"]), np.float64(recs[k]["y1"])), (np.float64(recs[k]["x2"]), np.float64(recs[k]["y2"])))
    for j in range(k):
        g = MR.geometry(band_segment(recs[j], 0.0))
        if g is None:
            continue
        x1, y1, ex, ey, nx, ny = g[:6]
        if all(abs((px - x1) * nx + (py - y1) * ny) <= dup_dist for px, py in ends):
            return j
    return -1


def rounds(frame, detect, max_trails=4, half=10.0, dup_dist=20.0):
    """One frame.  detect(native float32 frame, round) -> a record (anything with RESULT_DTYPE's fields); round 0 gets the frame
    itself.  Returns (records [max_trails], n_found, dup_of [max_trails])."""
    assert 1 <= max_trails <= MAX_TRAILS and np.isfinite(half) and half >= 0 and np.isfinite(dup_dist) and dup_dist >= 0
    recs = np.zeros(max_trails, RESULT_DTYPE)
    dups = np.full(max_trails, -1, np.int32)
    n_found = 0
    for k in range(max_trails):
        r = detect(frame if k == 0 else blotted(frame, recs[:k], half), k)
        for name in RESULT_DTYPE.names:
            recs[k][name] = r[name]
        dups[k] = dup_of(recs, k, dup_dist)
        if not found(recs[k]):
            break
        n_found = k + 1
    return recs, n_found, dups


def oracle_detect(O, params_bright, params_dim, cat=None, rs=None):
    """the oracle's detect_frame as a ``detect`` of ``rounds`` (it blots its own copy with the catalogue every round)"""
    def detect(frame, k):
        return O.detect_frame(np.ascontiguousarray(frame, np.float32).copy(), params_bright, params_dim, cat, rs)
    return detect
