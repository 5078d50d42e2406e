"""The short-trail search on the CPU (include/lfdmi.h: faint-trail search, steps 10 - 12): the parent-line identity of step 11,
the numpy restatement (tests/radon_short_ref.py) against radon_ref for its plain record, the noise figures the default
short_threshold rests on, quarter-length trails the plain search misses and the short search finds, and two short trails
found by peeling."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_short_ref as S  # noqa: E402
import test_radon_model as TM  # noqa: E402

SHORT_THRESHOLD = 8.5
# the largest short score of the 16 noise-only frames over all their levels: 5.807 (bin 1), 5.045 (bin 2); 1.4 x 5.807 = 8.13 is
# above 8, so the default is the next half-integer, 8.5
NOISE_MAX = {1: 5.807, 2: 5.045}

QUARTER_SHAPE = (512, 512)       # C = 256 = P in every orientation at bin 2: levels 64 and 128
QUARTER_SEED = 23
# the centre column of each orientation's four trails: inside strip 1 / strip 2 of level 64 (their quarter crossing is 64
# columns), or on the boundary of two level-64 strips (only level 128 holds such a trail whole)
QUARTER_CENTRE = (96, 64, 160, 192)
# Peaks before the factor max(|cos|, |sin|) of the trail's angle, which gives every trail the same signal per working column.
# The trails inside a strip share one peak.  A trail that straddles at its midpoint gains at most sqrt(2) on the plain search
# (its whole length fits only the next level, twice as long), and the thresholds 8.5 against 8 and the noise each search picks
# up leave less: over noise seeds 1 - 12 and 20 - 23 no single peak puts all eight of them between the two searches, while
# each of them has such peaks.  So each straddling trail carries the middle of its own window, found with the restatement
# (scores at peaks 0.020 and 0.026, linear between them): the windows are 0.0189 - 0.0210, 0.0261 - 0.0309, 0.0205 - 0.0257,
# 0.0178 - 0.0232, 0.0216 - 0.0324, 0.0190 - 0.0226, 0.0207 - 0.0223 and 0.0224 - 0.0271; inside a strip every peak in
# 0.0188 - 0.0239 serves all eight.
QUARTER_PEAK_INSIDE = 0.021
QUARTER_PEAK_STRADDLE = (0.0200, 0.0285, 0.0231, 0.0205, 0.0270, 0.0208, 0.0215, 0.0247)
# the largest end-point error along the line of the restatement's segment over these 16 trails, times 1.5 for another seed
# (the rule of test_radon_lines_model.PART_TOL)
QUARTER_END_ERROR = 22.39
QUARTER_TOL = 1.5 * QUARTER_END_ERROR


def test_parent_line_restricted_to_the_strip_is_the_candidate():
    """step 11, exhaustive for P = 64: over the columns of strip j the parent's path is the candidate's, row for row"""
    P = 64
    low = 0
    for level in (2, 4, 8, 16, 32):
        for j in range(P // level):
            for s in range(level):
                y0, sp = S.parent_of(level, j, 0, s, P)
                assert 0 <= sp < P and sp == s * (P // level)
                want = L.dyadic_path(s, level)                              # the candidate's rows, y = 0
                got = y0 + L.dyadic_path(sp, P)[j * level:(j + 1) * level]
                assert np.array_equal(got, want), (level, j, s)
                assert y0 == -s * j                                         # d(j L; Sp, P) = s j: no rounding on the way down
                low = min(low, y0 - (level - 1))
    # with y >= -(L-1) the parent row is at least -(L-1) P / L: it never lies below -(P-1)
    assert low == -(31 * 64 // 32) and low > -(P - 1)


def test_candidate_sums_are_the_sums_along_the_parent_path():
    """the stored levels against the cells of the parent line, on a small working array with every level down to 2"""
    rng = np.random.default_rng(4)
    Q = rng.integers(-9, 10, (9, 16)).astype(np.int64)
    Rr, C = Q.shape
    P = 16
    for n, F in S.levels(Q):
        if n == P:
            assert np.array_equal(F[0], R.transform(Q))
            continue
        for j in range(P // n):
            for s in range(n):
                for y in range(-(n - 1), Rr):
                    y0, sp = S.parent_of(n, j, y, s, P)
                    rows = y0 + L.dyadic_path(sp, P)[j * n:(j + 1) * n]
                    cols = np.arange(j * n, (j + 1) * n)
                    ok = (rows >= 0) & (rows < Rr)
                    assert F[j, y + P - 1, s] == Q[rows[ok], cols[ok]].sum(), (n, j, s, y)


@functools.lru_cache(maxsize=None)
def noise_short(b):
    """the restatement's (records, n_lines, plain) of test_radon_model's noise-only frames at bin b, at the defaults"""
    return tuple(S.search_short(f, TM.SET_SIGMA, bin=b) for f in TM.noise_frames())


@pytest.mark.parametrize("b", [1, 2])
def test_plain_record_is_radon_ref_and_noise_stays_below_the_default(b):
    from lfd_amd import radon
    assert radon.RadonShortParams().short_threshold == SHORT_THRESHOLD == S.SHORT_DEFAULTS["short_threshold"]
    snr = []
    for (recs, n_lines, plain), ref in zip(noise_short(b), TM.set_records("noise", b)):
        assert set(plain) == set(ref)
        for key, want in ref.items():
            got = plain[key]
            assert type(got) is type(want) and (got == want or key in ("sum", "snr") and got.tobytes() == want.tobytes()), key
        assert n_lines == 0 and recs[0]["status"] == R.OK and recs[0]["found"] == 0 and recs[0]["c2"] == 0
        assert all(r == S.ZERO for r in recs[1:])
        snr.append(float(recs[0]["snr"]))
    print("largest short score of the noise-only frames at bin", b, ["%.3f" % v for v in snr])
    assert abs(max(snr) - NOISE_MAX[b]) < 1e-3
    # the default: 8 if 1.4 times the largest maximum stays at or below 8, else the next half-integer above it
    top = 1.4 * max(NOISE_MAX.values())
    assert SHORT_THRESHOLD == (8.0 if top <= 8.0 else math.floor(top * 2) / 2 + 0.5)
    assert max(snr) < SHORT_THRESHOLD


@functools.lru_cache(maxsize=None)
def quarter_plan():
    """INJECT records of 16 sigma-2 trails, four per orientation, each over a quarter of its crossing of QUARTER_SHAPE; even
    ones lie inside one level-64 strip at bin 2, odd ones straddle a strip boundary at their midpoint"""
    from lfd_amd import recovery
    h, w = QUARTER_SHAPE
    tr = np.zeros(TM.SET_SIZE, IR.TRAIL_DTYPE)
    for i, deg in enumerate(TM.SET_THETA):
        th = math.radians(deg)
        c, s = math.cos(th), math.sin(th)
        x0, y0 = w / 2 + 7 * (i % 4) - 10, h / 2 - 5 * (i % 3) + 4
        rho = x0 * c + y0 * s
        ta, tb = recovery.extent(rho, th, -np.inf, np.inf, QUARTER_SHAPE)
        pos = 2 * QUARTER_CENTRE[i % 4]                                    # pixels along the orientation's column axis
        tc = (rho * c - pos) / s if TM.SET_Q[i] < 2 else (pos - rho * s) / c
        half = (tb - ta) / 8
        assert ta <= tc - half and tc + half <= tb
        peak = QUARTER_PEAK_STRADDLE[i // 2] if i % 2 else QUARTER_PEAK_INSIDE
        tr[i] = (i, 0, rho, th, tc - half, tc + half, peak * max(abs(c), abs(s)))
    return tr


@functools.lru_cache(maxsize=None)
def quarter_frames():
    _, table, step = TM.trail_plan()
    noise = np.random.default_rng(QUARTER_SEED).normal(0, TM.SET_SIGMA, (TM.SET_SIZE, *QUARTER_SHAPE)).astype(np.float32)
    f = IR.inject(noise, quarter_plan(), table, step)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def quarter_records():
    """the restatement's (records, n_lines, plain) of the quarter-length frames: one round at the defaults, bin 2"""
    return tuple(S.search_short(f, TM.SET_SIGMA, max_lines=1, bin=2) for f in quarter_frames())


def test_quarter_length_trails_are_missed_by_the_plain_search_and_found_by_the_short_one():
    tr = quarter_plan()
    out = quarter_records()
    plain = [float(p["snr"]) for _, _, p in out]
    short = [float(r[0]["snr"]) for r, _, _ in out]
    errs, line_errs = [], []
    for i, (recs, n_lines, _) in enumerate(out):
        r, th = recs[0], float(tr["theta"][i])
        if r["found"]:
            lo, hi = sorted((-r["ex1"] * math.sin(th) + r["ey1"] * math.cos(th), -r["ex2"] * math.sin(th) + r["ey2"] * math.cos(th)))
            errs.append(max(abs(lo - tr["t0"][i]), abs(hi - tr["t1"][i])))
            one = tr[i:i + 1].copy()
            line_errs.append(TM.line_error(r, one[0], QUARTER_SHAPE))
    print("plain snr", ["%.2f" % v for v in plain])
    print("short snr", ["%.2f" % v for v in short], "levels", [r[0]["level"] for r, _, _ in out])
    print("end-point errors along the line (px)", ["%.1f" % e for e in errs])
    print("parent line errors (deg, px)", [("%.2f" % a, "%.1f" % d) for a, d in line_errs])
    assert all(p["status"] == R.OK and p["found"] == 0 for _, _, p in out)           # the plain search: nothing, on every frame
    assert all(n == 1 and r[0]["found"] == 1 for r, n, _ in out)                     # the short search: every one
    assert [r[0]["q"] for r, _, _ in out] == list(TM.SET_Q)
    assert [r[0]["level"] for r, _, _ in out] == [64, 128] * 8                       # a straddling trail fits only the wider strip
    assert max(errs) <= QUARTER_TOL


@functools.lru_cache(maxsize=None)
def two_short_frame():
    """two quarter-length trails on one frame: the inside-a-strip trails of orientations 0 and 2 at 1.5 times their peak"""
    _, table, step = TM.trail_plan()
    tr = quarter_plan()[[0, 8]].copy()
    tr["frame"] = 0
    tr["amplitude"] *= 1.5
    noise = np.random.default_rng(QUARTER_SEED + 1).normal(0, TM.SET_SIGMA, (1, *QUARTER_SHAPE)).astype(np.float32)
    f = IR.inject(noise, tr, table, step)[0]
    f.setflags(write=False)
    return f, tr


def test_two_short_trails_are_found_by_peeling_and_the_third_round_stops():
    f, tr = two_short_frame()
    recs, n_lines, plain = S.search_short(f, TM.SET_SIGMA, bin=2)
    print("short snr by round", ["%.2f" % float(r["snr"]) for r in recs], "plain %.2f" % float(plain["snr"]))
    assert n_lines == 2
    assert sorted(r["q"] for r in recs[:2]) == [0, 2]
    for r in recs[:2]:
        t = tr[0] if r["q"] == 0 else tr[1]
        a, d = TM.line_error(r, t, QUARTER_SHAPE)
        assert r["found"] == 1 and r["seg_n_pix"] >= 32 and a <= 3.0 and d <= 4.0, (a, d)
    stop = recs[2]
    assert stop["status"] == R.OK and stop["found"] == 0 and float(stop["snr"]) < SHORT_THRESHOLD and stop["c2"] == 0
    assert recs[3] == S.ZERO
