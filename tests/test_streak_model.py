"""The short-streak search on the CPU, on the restatement (tests/streak_ref.py): the noise ceiling and the rule the default
threshold follows, sixteen 64 px streaks on the sixteen 372 x 512 noise crops of tests/test_radon_model.py, the short search of
the faint-trail unit on the same frames for comparison, and what remove_stars leaves behind on synthetic frames (recorded).
Each bound is the measured extreme with a stated margin."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import streak_ref as S  # noqa: E402
import test_radon_model as TM  # noqa: E402

# the noise-only peaks of the sixteen crops at the defaults (bin 2, L 32), as include/lfdmi.h step 5 lists them
NOISE_PEAKS = (5.18, 5.05, 5.08, 4.85, 4.58, 5.41, 4.86, 4.98, 5.30, 4.97, 4.84, 5.03, 4.87, 5.02, 5.19, 5.12)
NOISE_MAX = 5.413
MARGIN = 1.4                     # the margin the short search keeps
STREAK_LEN = 64.0                # px
STREAK_SIGMA = 1.5               # px
PEAKS = (0.03, 0.04, 0.05, 0.06)
# the smallest of PEAKS at which all sixteen streaks are found: already 0.03 finds them all (scores 9.4 - 13.3; 0.04: 12.4 -
# 17.1, 0.05: 15.3 - 20.9, 0.06: 18.2 - 24.7)
RECOVERY_PEAK = 0.03
# the smallest score of the sixteen at RECOVERY_PEAK is 9.4; 0.9 of it for another seed still clears the threshold
RECOVERY_MIN_SNR = 0.9 * 9.4
# angles of the line's direction in degrees, four per octant pair, none on the grid's own directions
ANGLES = (5, 17, 29, 41, 52, 64, 76, 88, 97, 109, 121, 133, 142, 154, 166, 178)


def half_reach(p=S.DEFAULTS):
    return p["length"] * p["bin"] / 2.0


@functools.lru_cache(maxsize=None)
def noise_records():
    return tuple(S.search(f, TM.SET_SIGMA) for f in TM.noise_frames())


@functools.lru_cache(maxsize=None)
def streak_plan(peak):
    """INJECT records of one 64 px streak per crop, its middle near the frame's"""
    h, w = TM.SET_SHAPE
    tr = np.zeros(TM.SET_SIZE, IR.TRAIL_DTYPE)
    for i, deg in enumerate(ANGLES):
        a = math.radians(deg)                                         # the direction; the normal's angle is theta
        th = (a + math.pi / 2) % math.pi
        x0, y0 = w / 2 + 11 * (i % 4) - 20, h / 2 - 9 * (i % 3) + 7
        c, s = math.cos(th), math.sin(th)
        t_mid = -x0 * s + y0 * c
        tr[i] = (i, 0, x0 * c + y0 * s, th, t_mid - STREAK_LEN / 2, t_mid + STREAK_LEN / 2, peak)
    return tr


@functools.lru_cache(maxsize=None)
def streak_frames(peak):
    from lfd_amd import inject as I
    table, step = I.gaussian_table(STREAK_SIGMA)
    f = IR.inject(TM.noise_frames().copy(), streak_plan(peak), I.normalise_peak(table).astype(np.float32), step)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def streak_records(peak):
    return tuple(S.search(f, TM.SET_SIGMA) for f in streak_frames(peak))


def end_errors(rec, tr):
    """(distance of either end from the truth line, the midpoint's place along it relative to the extent)"""
    c, s = math.cos(tr["theta"]), math.sin(tr["theta"])
    d = [abs(x * c + y * s - tr["rho"]) for x, y in ((rec["x1"], rec["y1"]), (rec["x2"], rec["y2"]))]
    mx, my = 0.5 * (rec["x1"] + rec["x2"]), 0.5 * (rec["y1"] + rec["y2"])
    t = -mx * s + my * c
    return max(d), tr["t0"] <= t <= tr["t1"]


def test_noise_ceiling_and_the_default_threshold_rule():
    snr = [float(r["snr"]) for r in noise_records()]
    print("noise-only streak peaks", ["%.2f" % v for v in snr])
    assert ["%.2f" % v for v in snr] == ["%.2f" % v for v in NOISE_PEAKS]
    assert all(r["status"] == S.OK and r["found"] == 0 and r["n_pix"] == 128 for r in noise_records())
    assert abs(max(snr) - NOISE_MAX) < 1e-3
    rule = math.ceil(MARGIN * max(snr) * 2.0) / 2.0                   # rounded up to the next 0.5
    assert rule == S.DEFAULTS["threshold"] == 8.0
    from lfd_amd import streaks
    assert streaks.default_params()["threshold"] == rule


def test_recovery_peak_is_the_smallest_that_finds_all_sixteen():
    found = {p: sum(r["found"] for r in streak_records(p)) for p in PEAKS}
    for p in PEAKS:
        print("peak", p, "found", found[p], "snr", ["%.1f" % float(r["snr"]) for r in streak_records(p)])
    assert RECOVERY_PEAK == min(p for p in PEAKS if found[p] == TM.SET_SIZE)
    recs, tr = streak_records(RECOVERY_PEAK), streak_plan(RECOVERY_PEAK)
    assert min(float(r["snr"]) for r in recs) >= RECOVERY_MIN_SNR > S.DEFAULTS["threshold"]
    errs = [end_errors(r, tr[i]) for i, r in enumerate(recs)]
    print("end distances from the truth line", ["%.1f" % d for d, _ in errs])
    assert all(d <= half_reach() and inside for d, inside in errs)
    for p in PEAKS:                                                   # whatever is found at any peak lies on its streak
        for i, r in enumerate(streak_records(p)):
            if r["found"]:
                d, inside = end_errors(r, streak_plan(p)[i])
                assert d <= half_reach() and inside, (p, i)
    assert not any(r["found"] for r in noise_records())


def test_radon_short_on_the_same_frames():
    """for comparison: the dyadic short search scores strips of 64 binned columns and up, 128 px at bin 2, so a 64 px streak
    fills half a strip at best.  Measured: it finds 5 of the sixteen at peak 0.03 (14 at 0.05), where the streak search finds
    all sixteen"""
    import radon_short_ref as RS
    n_short = 0
    for f in streak_frames(RECOVERY_PEAK):
        recs, n_lines, _ = RS.search_short(f, TM.SET_SIGMA, max_lines=1, bin=2)
        n_short += int(n_lines > 0)
    n_streak = sum(r["found"] for r in streak_records(RECOVERY_PEAK))
    print("found of 16 at peak", RECOVERY_PEAK, ": radon_short", n_short, "streak search", n_streak)
    assert n_short <= n_streak == TM.SET_SIZE


def test_what_the_stars_leave_behind_is_recorded(oracle):
    """synth.make_frame frames after the oracle's remove_stars, seeds 0 - 3 as 372 x 512 crops: peaks 7.79, 7.12, 7.87, 6.46, none
    found (each frame carries a bright trail whose core lies above the clip; its wings and the stars' leftovers make these
    peaks, above the pure-noise ceiling of 5.41 and below the threshold).  Recorded, not asserted: real frames decide."""
    from lfd_amd import synth
    from lfd_amd.detecttrails import default_params
    _, _, prs = default_params()
    rs = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    peaks = []
    for k in range(4):
        img, cat, truth = synth.make_frame(k, shape=TM.SET_SHAPE)
        img = oracle.remove_stars(np.array(img, np.float32), cat, rs)
        rec = S.search(img, TM.SET_SIGMA)
        peaks.append((k, bool(truth["streak"]), float(rec["snr"]), int(rec["found"])))
        assert rec["status"] == S.OK
    print("synthetic frames after remove_stars: (seed, has a streak, peak, found)", peaks)
