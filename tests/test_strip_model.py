"""The trail strips on the CPU (restatement only, tests/strip_ref.py): cells worked out by hand, the bin rule at its edges, the
identity with the light curves' restatement, and what the figures mean on the 372 x 512 frames of test_radon_model's set (sky
sigma 0.025, sixteen noise frames, a sigma-2 Gaussian trail of peak 0.02 per frame in sixteen orientations; sections of 32 px,
half 14, wing 6).  ``python tests/test_strip_model.py`` prints the measured figures the tolerances below are 1.5 times of."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import lc_ref as LR  # noqa: E402
import strip_ref as SR  # noqa: E402
import test_radon_model as TM  # noqa: E402
from test_lc_model import line_points, pieces  # noqa: E402

HALF, SEC = 14.0, 32.0
TRUE_RATE = TM.SET_PEAK * 2.0 * math.sqrt(2.0 * math.pi)    # flux per px of trail length: 0.1003
BRIGHT = 5.0                                                # the offset and the widening trail: peak 0.1, so that every section passes k_mom
# the extremes of the restatement over the sixteen frames (``python tests/test_strip_model.py``), times 1.5:
# (a) noise only, k_mom 5: 0 of 254 OK sections pass (a 5-sigma excess of noise has probability 3e-7); |rate| up to 2.993 rate_err
# (b) the trail: |rate - 0.1003| up to 2.994 rate_err (254 sections; a section's rate is about 4 rate_err); at the default k_mom 5, 33 of them have moments:
#     |centre| up to 1.300 px, width 1.406 .. 3.366 px against the truth 2
# (c) a peak-0.1 trail 1.5 px off the line: mean_centre 1.466 .. 1.572; (d) sigma 2 -> 4: first-quarter width 2.07 .. 2.30, last 3.30 .. 3.44
TOL_NOISE_SHARE = 0.0
TOL_RATE = 1.5 * 2.994
TOL_CENTRE = 1.5 * 1.300
WIDTH_LO, WIDTH_HI = 2.0 - 1.5 * (2.0 - 1.406), 2.0 + 1.5 * (3.366 - 2.0)


def strip_segment(t, shape, half=HALF, shift=0.0):
    """the strip segment of trail t: its in-frame crossing, moved by ``shift`` px along the normal"""
    ta, tb, pt = line_points(t, shape)
    (x1, y1), (x2, y2) = pt(ta), pt(tb)
    L = math.hypot(x2 - x1, y2 - y1)
    nx, ny = -(y2 - y1) / L, (x2 - x1) / L
    return np.array([SR.segment(0, x1 + shift * nx, y1 + shift * ny, x2 + shift * nx, y2 + shift * ny, half=half)], SR.SEGMENT_DTYPE)


def ok_sections(rec, sec):
    return [sec[0, j] for j in range(int(rec[0]["n_sec"])) if sec[0, j]["status"] == SR.SEC_OK]


@functools.lru_cache(maxsize=None)
def figures():
    """every figure of the module's docstring, measured once"""
    tr, table, step = TM.trail_plan()
    noise = TM.noise_frames()
    f = {"noise_ok": 0, "noise_pass": 0, "noise_z": [], "rate_z": [], "centre": [], "width": [], "shift": [], "w_first": [], "w_last": []}
    sig = (2.0, 2.5, 3.0, 3.5, 4.0)
    wstep = 0.125
    uu = np.arange(-192, 193, dtype=np.float64) * wstep      # out to 24 px: 6 sigma of the widest
    wide = np.stack([np.exp(-(uu * uu) / (2.0 * s * s)) for s in sig]).astype(np.float32)
    for i in range(TM.SET_SIZE):
        t = tr[i].copy()
        t["frame"] = 0
        seg = strip_segment(t, TM.SET_SHAPE)
        kw = dict(sigma=TM.SET_SIGMA, sec_len=SEC, max_sections=32)
        # (a) noise only
        rec, sec, _ = SR.trail_strips(noise[i], seg, **kw)
        for o in ok_sections(rec, sec):
            f["noise_ok"] += 1
            f["noise_pass"] += bool(np.isfinite(o["centre"]))
            f["noise_z"].append(abs(o["rate"]) / o["rate_err"])
        # (b) the set's trail
        img = IR.inject(noise[i:i + 1].copy(), [t], table, step)
        rec, sec, _ = SR.trail_strips(img, seg, **kw)
        assert rec[0]["status"] == SR.OK and rec[0]["n_off"] == 29
        for o in ok_sections(rec, sec):
            f["rate_z"].append(abs(o["rate"] - TRUE_RATE) / o["rate_err"])
            if np.isfinite(o["centre"]):
                f["centre"].append(abs(o["centre"]))
                f["width"].append(float(o["width"]))
        if i % 4:
            continue
        # (c) a bright trail 1.5 px off the given line (the segment is the trail's line moved by -1.5 px: u of the trail is +1.5)
        b = t.copy()
        b["amplitude"] = BRIGHT * TM.SET_PEAK
        img = IR.inject(noise[i:i + 1].copy(), [b], table, step)
        rec, sec, _ = SR.trail_strips(img, strip_segment(t, TM.SET_SHAPE, shift=-1.5), **kw)
        f["shift"].append(float(rec[0]["mean_centre"]))
        # (d) a bright trail whose sigma grows from 2 to 4 along it in five pieces of equal length
        ta, tb, _ = line_points(t, TM.SET_SHAPE)
        pc = pieces(b, [ta + (tb - ta) * k / 5.0 for k in range(1, 5)], [BRIGHT * TM.SET_PEAK] * 5)
        pc["table"] = np.arange(5)
        img = IR.inject(noise[i:i + 1].copy(), pc, wide, wstep)
        rec, sec, _ = SR.trail_strips(img, seg, **kw)
        w = [float(o["width"]) for o in ok_sections(rec, sec) if np.isfinite(o["centre"])]
        assert len(w) >= 8
        f["w_first"].append(float(np.mean(w[:len(w) // 4])))
        f["w_last"].append(float(np.mean(w[-(len(w) // 4):])))
    return f


def test_cells_by_hand():
    """8 x 12 pixels holding the ramp (x + 12 y) 2^-10, the horizontal segment y = 3 from x = 0 to 10, half 2, step 1, sec_len 4:
    rows 1 .. 5 are bins 0 .. 4, columns 0 .. 3 section 0, 4 .. 7 section 1, 8 .. 10 section 2 (t = 10 = L on the centre of pixel
    10); column 11 and rows 0, 6, 7 take no part"""
    img = np.zeros((8, 12), np.float32)
    fl = img[::-1]                                           # fl[y, x]
    for y in range(8):
        fl[y] = (np.arange(12) + 12 * y) * 2.0 ** -10
    fl[3, 5], fl[1, 9], fl[5, 2] = np.nan, 0.5, -0.0         # three invalid pixels: cells (1, 2), (2, 0) and (0, 4)
    seg = [SR.segment(0, 0.0, 3.0, 10.0, 3.0, half=2.0)]
    rec, sec, cel = SR.trail_strips(img, seg, sigma=0.5, max_sections=4, sec_len=4.0, wing=0.5, min_core=4, min_wing=4, k_mom=0.0)
    r = rec[0]
    assert (r["status"], r["n_sec"], r["n_off"], r["K"]) == (SR.OK, 3, 5, 2) and cel.shape == (1, 15)
    c = cel[0].reshape(3, 5)
    cols = {0: range(0, 4), 1: range(4, 8), 2: range(8, 11)}
    for j in range(3):
        for b in range(5):
            y = b + 1
            xs = [x for x in cols[j] if (y, x) not in ((3, 5), (1, 9), (5, 2))]
            assert c[j, b]["n_geom"] == len(cols[j]) and c[j, b]["n"] == len(xs), (j, b)
            assert c[j, b]["q"] == sum(x + 12 * y for x in xs) * 2 ** 20, (j, b)
    # section 0: wing bins 0 and 4 (|u_b| >= 2 - 0.5), core bins 1 .. 3; every step of the record by hand
    a = sec[0, 0]
    assert (a["n_geom"], a["n_core"], a["n_wing"], a["status"]) == (20, 12, 7, SR.SEC_OK) and (a["t0"], a["t1"]) == (0.0, 4.0)
    q_wing = (6 + 48 * 1) + (0 + 1 + 3 + 3 * 60)
    bkg = q_wing * 2.0 ** -10 / 7.0
    v = [(6 + 48 * y) * 2.0 ** -10 / 4.0 - bkg for y in (2, 3, 4)]
    S0 = (0.0 + v[0]) + v[1] + v[2]
    S1 = (0.0 + v[0] * -1.0) + v[1] * 0.0 + v[2] * 1.0
    S2 = (0.0 + v[0] * -1.0 * -1.0) + v[1] * 0.0 * 0.0 + v[2] * 1.0 * 1.0
    assert a["bkg"] == bkg and a["rate"] == S0 * 1.0
    assert a["rate_err"] == 0.5 * 1.0 * math.sqrt(0.25 + 0.25 + 0.25 + 3.0 * 3.0 / 7.0)
    d = S2 / S0 - (S1 / S0) * (S1 / S0)
    assert a["centre"] == S1 / S0 and a["width"] == math.sqrt(d if d > 0 else 0.0)
    assert (sec[0, 2]["t0"], sec[0, 2]["t1"], sec[0, 2]["n_geom"]) == (8.0, 10.0, 15)
    assert not sec[0, 3].tobytes().strip(b"\0")              # rows past n_sec are zero bytes
    assert r["n_ok"] == 3 and r["n_mom"] == sum(np.isfinite(sec[0, :3]["centre"]))
    # min_core above what a section holds: LOW, integers kept; no OK section: EMPTY
    rec, sec, cel2 = SR.trail_strips(img, seg, max_sections=4, sec_len=4.0, wing=0.5, min_core=13, min_wing=4)
    assert sec[0, 0]["status"] == SR.SEC_LOW and sec[0, 0]["n_core"] == 12 and np.isnan(sec[0, 0]["rate"])
    assert rec[0]["status"] == SR.EMPTY and (rec[0]["n_sec"], rec[0]["n_ok"], rec[0]["dev_section"]) == (3, 0, -1)
    assert np.isnan(rec[0]["mean_centre"]) and cel2.tobytes() == cel.tobytes()
    # a wing as wide as the band: every bin is a wing bin
    rec, sec, _ = SR.trail_strips(img, seg, max_sections=4, sec_len=4.0, wing=2.0, min_core=1, min_wing=1)
    assert sec[0, 0]["n_core"] == 0 and sec[0, 0]["n_wing"] == 19 and sec[0, 0]["status"] == SR.SEC_LOW
    # one section, or one cell, too many for the rows; a band of more than MAX_OFF bins
    for kw in (dict(max_sections=2), dict(max_sections=4, max_cells=14)):
        rec, sec, cel = SR.trail_strips(img, seg, sec_len=4.0, **kw)
        assert rec[0]["status"] == SR.TOO_LONG and rec[0]["n_sec"] == 0 and not sec.tobytes().strip(b"\0") and not cel.tobytes().strip(b"\0")
    assert SR.trail_strips(img, seg, sec_len=4.0, max_sections=4, max_cells=15)[0][0]["status"] == SR.EMPTY   # (the default wing: LOW)
    assert SR.trail_strips(img, [SR.segment(0, 0.0, 3.0, 10.0, 3.0, half=64.5)], max_sections=4)[0][0]["n_off"] == 129
    assert SR.trail_strips(img, [SR.segment(0, 0.0, 3.0, 10.0, 3.0, half=64.6)], max_sections=4)[0][0]["status"] == SR.BAD_SEGMENT
    # the bounding box of the quick path changes nothing
    rng = np.random.default_rng(3)
    frame = rng.normal(0, 0.025, (60, 90)).astype(np.float32)
    ok = LR.valid(frame, 0.125)
    q = np.where(ok, LR.fixed(frame), 0)
    for _ in range(20):
        s = SR.segment(0, *rng.uniform(-20, 100, 4), half=float(rng.choice([1.0, 3.0, 9.5])))
        g = SR.geometry(s, SR.DEFAULTS, 64, 1 << 30)[1]
        assert np.array_equal(SR.cells(frame, g, ok, q), SR.cells(frame, g, ok, q, full=True))


def test_the_bin_rule_at_its_edges():
    def g(half, step=1.0):
        return SR.geometry(SR.segment(0, 0.0, 0.0, 10.0, 0.0, half=half), dict(SR.DEFAULTS, step=step), 64, 1 << 30)[1]

    def b_of(geo, us, t=5.0):
        part, j, b = SR.bins(np.array(us, np.float64), np.full(len(us), t), geo)
        return part.tolist(), [int(v) if m else None for v, m in zip(b, part)]
    nxt, prv = np.nextafter(2.25, 3.0), np.nextafter(2.25, 2.0)
    # half 2.25: K = 2, five bins; u = +-half belongs to the outermost bins, the float past it to nothing
    geo = g(2.25)
    assert geo[-1] == 2 and geo[-2] == 5
    assert b_of(geo, [-2.25, 2.25, prv, -prv, nxt, -nxt]) == ([True, True, True, True, False, False], [0, 4, 4, 0, None, None])
    # u_b +- step / 2: the lower edge belongs to the bin, the upper edge to the next one
    e = 2.0 ** -50
    assert b_of(geo, [-0.5, -0.5 - e, 0.5, 0.5 - e, 1.5, -1.5])[1] == [2, 1, 3, 2, 4, 1]
    # (the sum u * inv_u + kc is rounded: the float next below an edge is closer to it than the sum can tell, and goes with the edge)
    assert b_of(geo, [np.nextafter(-0.5, -1.0), np.nextafter(0.5, 0.0)])[1] == [2, 3]
    # half 2.5: u = +half gives 2 K + 1 before the clamp
    geo = g(2.5)
    assert geo[-1] == 2 and b_of(geo, [2.5, -2.5]) == ([True, True], [4, 0])
    # K = 0: one bin, whatever u
    geo = g(0.5)
    assert geo[-1] == 0 and geo[-2] == 1 and b_of(geo, [-0.5, 0.0, 0.5, 0.51]) == ([True, True, True, False], [0, 0, 0, None])
    assert g(0.3)[-1] == 0
    # the ends of n_off: half 32 at step 0.5 and half 64 at step 1 have 129 bins, one float more has too many
    assert g(32.0, 0.5)[-2] == 129 and g(64.0)[-2] == 129 and g(64.5)[-2] == 129
    assert SR.geometry(SR.segment(0, 0.0, 0.0, 10.0, 0.0, half=32.3), dict(SR.DEFAULTS, step=0.5), 64, 1 << 30)[0] == SR.BAD_SEGMENT
    # t == L on a pixel centre takes part, in the last section; past it nothing does
    geo = g(2.0)
    part, j, b = SR.bins(np.zeros(4), np.array([0.0, 8.0, 10.0, np.nextafter(10.0, 11.0)]), geo)
    assert part.tolist() == [True, True, True, False] and j[:3].tolist() == [0, 1, 1] and geo[-3] == 2


def test_summed_over_offsets_a_strip_is_a_light_curve():
    """the identity, with the restatements alone: at the same half, clip, mask and sec_len 8 the strip's cells summed over b are
    lc_ref's n_geom, n_core and q_core per section"""
    rng = np.random.default_rng(11)
    frame = rng.normal(0, 0.05, (70, 100)).astype(np.float32)
    frame[rng.random(frame.shape) < 0.02] = np.nan
    frame[rng.random(frame.shape) < 0.02] = 0.0
    frame[3, 4], frame[5, 6], frame[7, 8] = np.inf, 0.125, np.nextafter(np.float32(0.125), np.float32(1))
    mask = (rng.random(frame.shape) < 0.1).astype(np.uint8) * 5
    for k in range(24):
        half = float(rng.choice([0.5, 2.25, 7.0, 14.0]))
        ends = rng.uniform(-30, 130, 4)
        kw = dict(mask=mask, skip_bits=4) if k % 2 else {}
        step = float(rng.choice([0.5, 1.0, 3.0]))
        rec, sec, cel = SR.trail_strips(frame, [SR.segment(0, *ends, half=half)], max_sections=64, step=step, **kw)
        lrec, lsec = LR.light_curves(frame, [LR.segment(0, *ends, half=half, bg_in=half + 1.0, bg_out=half + 3.0)], max_sections=64,
                                     sec_len=8.0, **kw)
        assert rec[0]["status"] in (SR.OK, SR.EMPTY) and lrec[0]["status"] in (LR.OK, LR.EMPTY) and rec[0]["n_sec"] == lrec[0]["n_sec"]
        ns, no = int(rec[0]["n_sec"]), int(rec[0]["n_off"])
        c = cel[0][:ns * no].reshape(ns, no)
        assert np.array_equal(c["n_geom"].sum(1), lsec[0, :ns]["n_geom"])
        assert np.array_equal(c["n"].sum(1), lsec[0, :ns]["n_core"])
        assert np.array_equal(c["q"].sum(1), lsec[0, :ns]["q_core"])
        assert np.array_equal(sec[0, :ns]["n_geom"], lsec[0, :ns]["n_geom"])


def test_noise_alone_has_no_moments():
    f = figures()
    assert f["noise_ok"] >= 200 and f["noise_pass"] / f["noise_ok"] <= TOL_NOISE_SHARE, (f["noise_pass"], f["noise_ok"])


def test_the_trail_comes_back_section_by_section():
    f = figures()
    assert len(f["rate_z"]) >= 200 and max(f["rate_z"]) <= TOL_RATE, max(f["rate_z"])
    assert len(f["centre"]) >= 16 and max(f["centre"]) <= TOL_CENTRE, max(f["centre"])
    assert WIDTH_LO <= min(f["width"]) and max(f["width"]) <= WIDTH_HI, (min(f["width"]), max(f["width"]))


def test_a_trail_off_the_line_shows_in_the_centre():
    f = figures()
    assert all(abs(c - 1.5) <= 1.0 for c in f["shift"]), f["shift"]         # (within one step of 1.5)


def test_a_widening_trail_shows_in_the_width():
    f = figures()
    assert all(a < b for a, b in zip(f["w_first"], f["w_last"])), (f["w_first"], f["w_last"])


def test_to_uint8():
    from lfd_amd import strips
    assert strips.to_uint8(np.full((3, 4), np.nan)).tolist() == [[0] * 4] * 3
    assert strips.to_uint8(np.full((3, 4), 0.5)).tolist() == [[0] * 4] * 3 and strips.to_uint8(np.zeros((0, 0))).shape == (0, 0)
    m = np.arange(101, dtype=np.float32).reshape(1, 101)
    u = strips.to_uint8(m, 0.0, 100.0)
    assert u.dtype == np.uint8 and u[0, 0] == 0 and u[0, 100] == 255 and u[0, 50] == 128 and (np.diff(u[0].astype(int)) >= 0).all()
    u = strips.to_uint8(m, 10.0, 90.0)                       # the percentile ends: 10 and 90; outside them the stretch is clipped
    assert (u[0, :11] == 0).all() and (u[0, 90:] == 255).all() and u[0, 50] == 128 and 0 < u[0, 11] < u[0, 89] < 255
    m2 = m.copy()
    m2[0, 7] = np.nan
    m2[0, 8] = np.inf
    u = strips.to_uint8(m2, 0.0, 100.0)
    assert u[0, 7] == 0 and u[0, 8] == 0 and u[0, 100] == 255 and u[0, 0] == 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for k, v in figures().items():
        if isinstance(v, list):
            print("%-10s n = %3d  min %.4g  max %.4g" % (k, len(v), min(v), max(v)))
        else:
            print("%-10s %d" % (k, v))
