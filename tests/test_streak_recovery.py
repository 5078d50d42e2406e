"""The matching rule of ``python -m lfd_amd.recovery --detector streak`` on hand-made records, without a GPU: a found streak
matches when both its ends lie within L b / 2 px of the injected segment's line and its midpoint lies inside the injected
extent."""
import math

import numpy as np
import pytest

from lfd_amd import recovery, streaks

SHAPE = (200, 300)
REACH = 32.0                                                          # L b / 2 at the defaults


def plan(theta_deg, x0, y0, half_len, frame=0):
    """a trail through (x0, y0) with its normal at theta, half_len px either side"""
    th = math.radians(theta_deg)
    c, s = math.cos(th), math.sin(th)
    t = -x0 * s + y0 * c
    tr = np.zeros(1, recovery.PLAN_DTYPE)
    tr[0] = (frame, 0.05, x0 * c + y0 * s, th, t - half_len, t + half_len)
    return tr


def record(x1, y1, x2, y2, found=1):
    r = np.zeros((), streaks.STREAK_DTYPE)
    r["found"], r["x1"], r["y1"], r["x2"], r["y2"] = found, x1, y1, x2, y2
    th = math.atan2(-(x2 - x1), y2 - y1) % math.pi
    r["theta"], r["rho"] = th, x1 * math.cos(th) + y1 * math.sin(th)
    return r


def frames_of(*per_frame):
    k = max(1, max(len(f) for f in per_frame))
    recs = np.zeros((len(per_frame), k), streaks.STREAK_DTYPE)
    for i, f in enumerate(per_frame):
        for j, r in enumerate(f):
            recs[i, j] = r
    return recs, np.array([sum(int(r["found"]) for r in f) for f in per_frame], np.int32)


def test_a_streak_on_the_trail_matches():
    tr = plan(90.0, 150.0, 100.0, 32.0)                               # along x at y = 100, x = 118 .. 182
    recs, ns = frames_of([record(120.0, 101.0, 182.0, 99.0)])
    m, d_rho, d_theta, length, found = recovery.match_streaks(recs, ns, tr, SHAPE, REACH)
    assert m.tolist() == [True] and found.tolist() == [1] and length[0] == 64.0
    assert abs(d_rho[0]) < 1e-9 and abs(d_theta[0]) < math.radians(2.0)
    rows = recovery.streak_rows(recs, ns, tr, SHAPE, REACH)
    assert rows["matched"].tolist() == [1] and rows["found"].tolist() == [1] and np.isnan(rows["fwhm"][0])


def test_an_end_beyond_the_reach_does_not_match():
    tr = plan(90.0, 150.0, 100.0, 32.0)
    recs, ns = frames_of([record(120.0, 100.0, 182.0, 100.0 + REACH)])                # exactly at the reach: taken
    assert recovery.match_streaks(recs, ns, tr, SHAPE, REACH)[0].tolist() == [True]
    recs, ns = frames_of([record(120.0, 100.0, 182.0, 100.5 + REACH)])
    m, d_rho, _, _, found = recovery.match_streaks(recs, ns, tr, SHAPE, REACH)
    assert m.tolist() == [False] and found.tolist() == [1] and np.isfinite(d_rho[0])


def test_the_midpoint_must_lie_inside_the_extent():
    tr = plan(90.0, 150.0, 100.0, 32.0)                               # t runs against x here: the extent is x = 118 .. 182
    on_line_outside = record(190.0, 100.0, 252.0, 100.0)              # midpoint x = 221
    recs, ns = frames_of([on_line_outside])
    assert recovery.match_streaks(recs, ns, tr, SHAPE, REACH)[0].tolist() == [False]
    recs, ns = frames_of([record(152.0, 100.0, 212.0, 100.0)])        # midpoint x = 182: the extent's end, taken
    assert recovery.match_streaks(recs, ns, tr, SHAPE, REACH)[0].tolist() == [True]
    recs, ns = frames_of([record(153.0, 100.0, 213.0, 100.0)])
    assert recovery.match_streaks(recs, ns, tr, SHAPE, REACH)[0].tolist() == [False]


def test_later_records_and_other_frames():
    tr = np.concatenate([plan(90.0, 150.0, 100.0, 32.0, frame=0), plan(45.0, 100.0, 100.0, 40.0, frame=1),
                         plan(90.0, 150.0, 100.0, 32.0, frame=2)])
    far = record(10.0, 10.0, 70.0, 12.0)
    good = record(120.0, 100.0, 182.0, 100.0)
    stopped = record(120.0, 100.0, 182.0, 100.0, found=0)             # a stopping record is no detection
    recs, ns = frames_of([far, good], [far], [stopped])
    m, d_rho, _, _, found = recovery.match_streaks(recs, ns, tr, SHAPE, REACH)
    assert m.tolist() == [True, False, False] and found.tolist() == [2, 1, 0]
    assert abs(d_rho[0]) < 1e-9 and np.isfinite(d_rho[1]) and np.isnan(d_rho[2])


def test_a_trail_off_the_frame_never_matches():
    tr = plan(90.0, 150.0, 400.0, 32.0)                               # y = 400 on a frame of 200 rows
    recs, ns = frames_of([record(120.0, 199.0, 182.0, 199.0)])
    m, _, _, length, _ = recovery.match_streaks(recs, ns, tr, SHAPE, 1000.0)
    assert m.tolist() == [False] and length[0] == 0.0


def test_the_detector_is_offered():
    with pytest.raises(ValueError):
        recovery.run(None, np.zeros((1, 8, 8), np.float32), None, None, tr := plan(90.0, 4.0, 4.0, 2.0), None, 1.0, detector="streaks")
    with pytest.raises(ValueError):
        recovery.run(None, np.zeros((1, 8, 8), np.float32), None, None, tr, None, 1.0, detector="streak", null=4)
    with pytest.raises(SystemExit):
        recovery.main(["--synth", "0:1", "--peaks", "0.05", "--out", "x", "--detector", "streak", "--null", "4"])
