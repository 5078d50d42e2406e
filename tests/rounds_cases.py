"""Frames for the detection rounds' tests: the star field and catalogue of a streakless ``synth.make_portable_frame`` frame
(512 x 768; integer draws and IEEE + - * / sqrt only, so every machine builds the same bits) with 0 .. 3 streaks well apart
in angle (normals at 135, 173 and 99 degrees), each a triangle profile of 3 px half-base.  The detector takes the top lines of
a whole frame at once, so streaks of equal strength spoil each other's line sets and nothing passes; the peaks differ (one for
the bright pass's eye, one weaker, one for the dim pass) so that every round has one strongest streak.  HALF is the band that
covers such a streak after the passes' dilation; the default half of 10 px leaves its wings standing."""
import math

import numpy as np

from lfd_amd import synth

SHAPE = (512, 768)
# (x0, buffer row r0, a, b): the pixels with (x - x0) a - (r - r0) b = 0
STREAKS = ((384, 256, 1, -1), (300, 200, 8, -1), (450, 300, 3, -19))
PEAKS = (2.0, 1.0, 0.2)
WIDTH = 3.0
HALF = 16.0
# which streaks frame i of ``frames()`` carries
LAYOUT = ((), (0,), (0, 1), (0, 1, 2), (1,), (1, 2), (), (2,))
# hand-placed bright streaks for the gather's geometry: name -> (streak, half, theta of the record in degrees).  Each is drawn on
# field 0 with peak PEAKS[0], beside the dim streak 2; the detector finds it in round 0 (tests/test_rounds_model.py checks that on
# the oracle), so round 1 gathers with its band.  The detector finds no streak at theta = 0 exactly: 4 degrees is its nearest.
BANDS = {"near_vertical": ((384, 256, 19, 1), HALF, 4), "horizontal": ((384, 150, 0, 1), HALF, 90),
         "two_corners": ((0, 0, 2, 3), HALF, 57), "top_right_corner": ((767, 0, 1, -1), HALF, 135),
         "half_zero": ((0, 511, 1, -1), 0.0, 135), "wider_than_a_tile": ((767, 0, 1, -1), 150.0, 135)}


def band_frame(name):
    """(frame, catalogue, half) of a BANDS case"""
    streak, half, _ = BANDS[name]
    img, cat = field(0)
    add_streak(img, *streak, PEAKS[0])
    add_streak(img, *STREAKS[2], PEAKS[2])
    return img, cat, half


def field(k, shape=SHAPE):
    """(frame, catalogue) of the k-th streakless portable frame"""
    img, cat, truth = synth.make_portable_frame(3 * k + 2, shape)
    assert truth["streak"] == "none"
    return img, cat


def add_streak(img, x0, r0, a, b, peak, width=WIDTH):
    h, w = img.shape
    yy = np.arange(h, dtype=np.int64)[:, None]
    xx = np.arange(w, dtype=np.int64)[None, :]
    num = np.abs((xx - x0) * a - (yy - r0) * b).astype(np.float64)
    dist = num / np.sqrt(float(a * a + b * b))
    img += (np.maximum(0.0, 1.0 - dist / width) * peak).astype(np.float32)
    return img


def line_of(streak, h):
    """(rho, theta) of a streak in the records' coordinates (flipped rows), theta in [0, pi)"""
    x0, r0, a, b = streak
    y0 = h - 1 - r0                            # (x - x0) a + (y - y0) b = 0
    n = math.hypot(a, b)
    nx, ny = a / n, b / n
    if ny < 0 or (ny == 0 and nx < 0):
        nx, ny = -nx, -ny
    return x0 * nx + y0 * ny, math.atan2(ny, nx)


def same_cell(rec, streak, h, rho_res=20.0, theta_res=math.pi / 180):
    """is the record's line within one Hough cell of the streak's?"""
    rho, theta = line_of(streak, h)
    r, t = float(rec["rho"]), float(rec["theta"])
    if abs(t - theta) > math.pi / 2:           # the same line seen from the other side of theta = 0 / pi
        r, t = -r, t - math.pi if t > theta else t + math.pi
    return abs(r - rho) <= rho_res and abs(t - theta) <= theta_res


def frame(i, which, shape=SHAPE):
    """(frame, catalogue) of field i with the streaks ``which`` of STREAKS"""
    img, cat = field(i, shape)
    for s in which:
        add_streak(img, *STREAKS[s], PEAKS[s])
    return img, cat


def frames(layout=LAYOUT, shape=SHAPE):
    """([n, h, w] float32, [catalogue]) for a layout"""
    pairs = [frame(i, which, shape) for i, which in enumerate(layout)]
    return np.stack([p[0] for p in pairs]), [p[1] for p in pairs]
