"""The light curves on the CPU (restatement only, tests/lc_ref.py): sections worked out by hand, and what the figures mean on the
372 x 512 frames of test_radon_model's set (sky sigma 0.025, sixteen noise frames, a sigma-2 Gaussian trail of peak 0.02 per
frame in sixteen orientations): noise only, a constant trail, a trail twice as bright in its second half, a sinusoidal
modulation, and a crossing trail kept out by a mask plane.  ``python tests/test_lc_model.py`` prints the measured figures the
tolerances below are 1.5 times of."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import lc_ref as LR  # noqa: E402
import mask_ref as MR  # noqa: E402
import stack_ref as S  # noqa: E402
import test_radon_model as TM  # noqa: E402

HALF = 10.0                                                 # masks.half_width without a measured fwhm
TRUE_RATE = TM.SET_PEAK * 2.0 * math.sqrt(2.0 * math.pi)    # flux per px of trail length: 0.1003
# the largest values of the restatement over the sixteen frames (``python tests/test_lc_model.py``), times 1.5:
# (a) noise only: chi2 / dof up to 1.551, |mean_rate| / mean_rate_err up to 1.679
# (b) constant trail: |mean_rate - truth| up to 0.01235 (1.713 mean_rate_err), |mean_rate - stack flux| up to 0.02004
# (c) two halves: a section's |rate - truth| up to 2.435 rate_err (234 sections); chi2 / dof at least 3.332
# (d) sinusoid over 8 sections: a section's |rate - truth| up to 2.408 rate_err (128 sections)
# (e) crossing trail: the masked section's |rate - truth| up to 1.036 rate_err; unmasked, its excess is at least 7.921 rate_err
TOL_CHI2, TOL_ZERO = 1.5 * 1.551, 1.5 * 1.679
TOL_RATE, TOL_STACK = 1.5 * 0.01235, 1.5 * 0.02004
TOL_SEC = 1.5 * 2.435
TOL_SIN = 1.5 * 2.408
TOL_MASKED = 1.5 * 1.036


def line_points(t, shape, a=None, b=None):
    """(ta, tb, point(t)) of trail t's line: its in-frame extent in the injection's t, and the point at t"""
    from lfd_amd import recovery
    th = float(t["theta"])
    c, s = math.cos(th), math.sin(th)
    ta, tb = recovery.extent(float(t["rho"]), th, -np.inf, np.inf, shape)
    return ta, tb, lambda tt: (t["rho"] * c - tt * s, t["rho"] * s + tt * c)


def lc_segment(t, shape, length=None):
    """the light-curve segment of trail t: its in-frame crossing from ta on (``length``: only that many px of it)"""
    ta, tb, pt = line_points(t, shape)
    if length is not None:
        tb = ta + length
    (x1, y1), (x2, y2) = pt(ta), pt(tb)
    return np.array([LR.segment(0, x1, y1, x2, y2, half=HALF)], LR.SEGMENT_DTYPE)


def pieces(t, bounds, amps):
    """trail t cut at the injection's t values ``bounds`` (ascending, the ends open) into len(amps) extents"""
    out = np.array([t] * len(amps), IR.TRAIL_DTYPE)
    edges = [-np.inf, *bounds, np.inf]
    for k, a in enumerate(amps):
        out[k]["t0"] = edges[k] if k == 0 else np.nextafter(edges[k], np.inf)
        out[k]["t1"], out[k]["amplitude"], out[k]["frame"] = edges[k + 1], a, 0
    return out


def ok_sections(rec, sec):
    return [(j, sec[0, j]) for j in range(int(rec[0]["n_sec"])) if sec[0, j]["status"] == LR.SEC_OK]


@functools.lru_cache(maxsize=None)
def figures():
    """every figure of the module's docstring, measured once"""
    tr, table, step = TM.trail_plan()
    noise = TM.noise_frames()
    f = {"chi2": [], "zero": [], "rate": [], "rate_z": [], "stack": [], "sec": [], "chi2_two": [], "sin": [], "masked": [], "bump": []}
    for i in range(TM.SET_SIZE):
        t = tr[i].copy()
        t["frame"] = 0
        seg = lc_segment(t, TM.SET_SHAPE)
        ta, tb, pt = line_points(t, TM.SET_SHAPE)
        tm = 0.5 * (ta + tb)
        # (a) noise only
        rec, sec = LR.light_curves(noise[i], seg, sigma=TM.SET_SIGMA)
        assert rec[0]["status"] == LR.OK and rec[0]["n_ok"] >= 8
        f["chi2"].append(rec[0]["chi2"] / rec[0]["dof"])
        f["zero"].append(abs(rec[0]["mean_rate"]) / rec[0]["mean_rate_err"])
        # (b) a constant trail, against the truth and against the stacked cross-section's flux on the same segment
        img = IR.inject(noise[i:i + 1].copy(), [t], table, step)
        rec, sec = LR.light_curves(img, seg, sigma=TM.SET_SIGMA)
        srec = S.measure(img[0], tuple(float(seg[0][k]) for k in ("x1", "y1", "x2", "y2")), TM.SET_SIGMA)[0]
        assert srec["status"] == S.OK
        f["rate"].append(abs(rec[0]["mean_rate"] - TRUE_RATE))
        f["rate_z"].append(abs(rec[0]["mean_rate"] - TRUE_RATE) / rec[0]["mean_rate_err"])
        f["stack"].append(abs(rec[0]["mean_rate"] - srec["flux"]))
        # (c) twice as bright in the second half
        img = IR.inject(noise[i:i + 1].copy(), pieces(t, [tm], [TM.SET_PEAK, 2 * TM.SET_PEAK]), table, step)
        rec, sec = LR.light_curves(img, seg, sigma=TM.SET_SIGMA)
        for j, o in ok_sections(rec, sec):
            a, b = ta + o["t0"], ta + o["t1"]
            if b < tm - 2 or a > tm + 2:                     # (the section that holds the break belongs to neither half)
                f["sec"].append(abs(o["rate"] - (TRUE_RATE if b < tm else 2 * TRUE_RATE)) / o["rate_err"])
        f["chi2_two"].append(rec[0]["chi2"] / rec[0]["dof"])
        # (d) a sinusoid over 8 sections of 32 px
        amps = [TM.SET_PEAK * (1.0 + 0.5 * math.sin(2.0 * math.pi * k / 8.0)) for k in range(8)]
        img = IR.inject(noise[i:i + 1].copy(), pieces(t, [ta + 32.0 * k for k in range(1, 8)], amps), table, step)
        seg8 = lc_segment(t, TM.SET_SHAPE, 256.0)
        rec, sec = LR.light_curves(img, seg8, sigma=TM.SET_SIGMA)
        assert rec[0]["n_sec"] in (8, 9)                     # (L is 256 up to the rounding of the end points)
        for j, o in (jo for jo in ok_sections(rec, sec) if jo[0] < 8):
            f["sin"].append(abs(o["rate"] - amps[j] / TM.SET_PEAK * TRUE_RATE) / o["rate_err"])
        # (e) a short bright trail across the middle, with and without its mask
        if i % 4 == 0:
            cross = t.copy()
            cross["theta"] = float(t["theta"]) + math.pi / 2
            j = int((tm - ta) // 32.0)                        # the section in the middle, crossed at its centre
            mx, my = pt(ta + 32.0 * j + 16.0)
            cross["rho"] = mx * math.cos(cross["theta"]) + my * math.sin(cross["theta"])
            c0 = -mx * math.sin(cross["theta"]) + my * math.cos(cross["theta"])       # the crossing point in the crossing trail's t
            cross["t0"], cross["t1"], cross["amplitude"] = c0 - 12.0, c0 + 12.0, 3 * TM.SET_PEAK
            img = IR.inject(noise[i:i + 1].copy(), [t, cross], table, step)
            th = float(cross["theta"])
            p0 = (cross["rho"] * math.cos(th) - (c0 - 12.0) * math.sin(th), cross["rho"] * math.sin(th) + (c0 - 12.0) * math.cos(th))
            p1 = (cross["rho"] * math.cos(th) - (c0 + 12.0) * math.sin(th), cross["rho"] * math.sin(th) + (c0 + 12.0) * math.cos(th))
            plane = MR.mask_trails([MR.segment(0, *p0, *p1, half=HALF, cap=2.0, bits=2)], (1, *TM.SET_SHAPE))[0]
            rec, sec = LR.light_curves(img, seg, mask=plane, skip_bits=2, sigma=TM.SET_SIGMA)
            assert sec[0, j]["status"] == LR.SEC_OK and sec[0, j]["coverage"] < 0.7
            f["masked"].append(abs(sec[0, j]["rate"] - TRUE_RATE) / sec[0, j]["rate_err"])
            for kw in (dict(mask=plane, skip_bits=1), dict(mask=plane, skip_bits=0), {}):
                rec, sec = LR.light_curves(img, seg, sigma=TM.SET_SIGMA, **kw)
                assert sec[0, j]["coverage"] > 0.95
                f["bump"].append((sec[0, j]["rate"] - TRUE_RATE) / sec[0, j]["rate_err"])
    return f


def test_one_section_by_hand():
    """8 x 12 pixels, the horizontal segment y = 3 from x = 0 to 10, half 1, sky 2 <= |u| <= 3, sec_len 8: rows 2 .. 4 are core, rows
    0, 1, 5, 6 sky, row 7 nothing; columns 0 .. 7 are section 0, 8 .. 10 section 1 (t = 10 = L on the centre of pixel 10), column
    11 takes no part"""
    img = np.zeros((8, 12), np.float32)
    fl = img[::-1]                                           # fl[y, x]
    fl[2:5] = 0.25                                           # core
    fl[[0, 1, 5, 6]] = 0.125                                 # sky
    fl[7] = 0.5
    fl[3, 2], fl[3, 3], fl[3, 4], fl[3, 5] = np.nan, 0.0, np.inf, 0.75     # four invalid core pixels (0.75 is above the clip)
    fl[0, 1] = -0.0
    fl[4, 9] = 2.0 ** -31                                    # a tie: rounds to the even 0
    fl[2, 9] = 3 * 2.0 ** -31                                # a tie: rounds to the even 2
    seg = [LR.segment(0, 0.0, 3.0, 10.0, 3.0, half=1.0, bg_in=2.0, bg_out=3.0)]
    rec, sec = LR.light_curves(img, seg, sigma=0.5, max_sections=3, sec_len=8.0, clip=0.5, min_core=4, min_sky=4)
    a, b = sec[0, 0], sec[0, 1]
    assert (a["n_geom"], a["n_core"], a["n_sky"]) == (24, 20, 31) and (a["t0"], a["t1"]) == (0.0, 8.0)
    assert a["q_core"] == 20 * 2 ** 28 and a["q_sky"] == 31 * 2 ** 27 and a["status"] == LR.SEC_OK
    assert (a["mean"], a["bkg"], a["sb"], a["flux"], a["rate"], a["coverage"]) == (0.25, 0.125, 0.125, 2.5, 0.25, 20 / 24)
    assert a["flux_err"] == 0.5 * math.sqrt(20.0 + 400.0 / 31.0) and a["rate_err"] == 0.5 * math.sqrt(1.0 / 20.0 + 1.0 / 31.0) * 2.0
    assert (b["n_geom"], b["n_core"], b["n_sky"]) == (9, 9, 12) and (b["t0"], b["t1"]) == (8.0, 10.0)
    assert b["q_core"] == 7 * 2 ** 28 + 0 + 2 and b["q_sky"] == 12 * 2 ** 27
    assert not sec[0, 2].tobytes().strip(b"\0")              # rows past n_sec are zero bytes
    r = rec[0]
    assert (r["status"], r["n_sec"], r["n_ok"], r["first_ok"], r["last_ok"], r["dof"], r["peak_section"]) == (LR.OK, 2, 2, 0, 1, 1, 0)
    assert r["length"] == 10.0 and r["peak_rate"] == 0.25 and r["mean_rate"] == (20 * a["rate"] + 9 * b["rate"]) / 29.0
    assert r["flux"] == r["mean_rate"] * 10.0 and r["flux_err"] == r["mean_rate_err"] * 10.0
    # min_core above what a section holds: LOW, integers kept; no OK section: EMPTY
    rec, sec = LR.light_curves(img, seg, max_sections=3, sec_len=8.0, clip=0.5, min_core=21, min_sky=4)
    assert sec[0, 0]["status"] == LR.SEC_LOW and sec[0, 0]["n_core"] == 20 and np.isnan(sec[0, 0]["rate"])
    assert rec[0]["status"] == LR.EMPTY and rec[0]["n_sec"] == 2 and rec[0]["dof"] == -1 and np.isnan(rec[0]["mean_rate"])
    # one section too many for the rows; the bounding box of the quick path changes nothing
    rec, sec = LR.light_curves(img, seg, max_sections=1, sec_len=8.0)
    assert rec[0]["status"] == LR.TOO_LONG and rec[0]["n_sec"] == 0 and not sec.tobytes().strip(b"\0")
    rng = np.random.default_rng(3)
    frame = rng.normal(0, 0.025, (60, 90)).astype(np.float32)
    ok = LR.valid(frame, 0.125)
    q = np.where(ok, LR.fixed(frame), 0)
    for _ in range(20):
        s = LR.segment(0, *rng.uniform(-20, 100, 4), half=float(rng.choice([1.0, 3.0])))
        g = LR.geometry(s, 8.0, 64)[1]
        assert np.array_equal(LR.sums(frame, g, ok, q), LR.sums(frame, g, ok, q, full=True))


def test_noise_only_segments_are_flat_and_empty():
    f = figures()
    assert max(f["chi2"]) <= TOL_CHI2 and max(f["zero"]) <= TOL_ZERO, (max(f["chi2"]), max(f["zero"]))


def test_a_constant_trail_comes_back():
    f = figures()
    assert max(f["rate"]) <= TOL_RATE and max(f["stack"]) <= TOL_STACK, (max(f["rate"]), max(f["stack"]))


def test_a_step_in_brightness_shows_in_the_sections():
    f = figures()
    assert max(f["sec"]) <= TOL_SEC, max(f["sec"])
    assert min(f["chi2_two"]) > TOL_CHI2, min(f["chi2_two"])        # above everything noise alone gives


def test_a_sinusoid_comes_back_section_by_section():
    f = figures()
    assert max(f["sin"]) <= TOL_SIN, max(f["sin"])


def test_a_mask_plane_removes_a_crossing_trail():
    f = figures()
    assert max(f["masked"]) <= TOL_MASKED, max(f["masked"])
    assert min(f["bump"]) > 3.0, min(f["bump"])                     # with other skip_bits, or without the plane, the bump is there


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for k, v in figures().items():
        print("%-9s n = %3d  min %.4g  max %.4g" % (k, len(v), min(v), max(v)))
