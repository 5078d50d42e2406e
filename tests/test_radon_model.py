"""The faint-trail search on the CPU: the numpy restatement (tests/radon_ref.py) against a brute-force enumeration of the
dyadic lines, its invariants, the host conversion of ``lfd_amd.radon`` and the figures the default threshold rests on
(include/lfdmi.h: faint-trail search)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import radon_ref as R  # noqa: E402

SET_SHAPE = (372, 512)
SET_SIZE = 16
SET_SIGMA = 0.025
SET_PEAK = 0.02
# four trails in each orientation's slope range: theta of the normal in degrees (q = 0: [90, 135], 1: [45, 90], 2: [135, 180],
# 3: [0, 45])
SET_THETA = (100, 110, 120, 130, 50, 60, 70, 80, 140, 150, 160, 170, 10, 20, 30, 40)
SET_Q = (0,) * 4 + (1,) * 4 + (2,) * 4 + (3,) * 4


@functools.lru_cache(maxsize=None)
def noise_frames():
    rng = np.random.default_rng(20)
    f = rng.normal(0, SET_SIGMA, (SET_SIZE, *SET_SHAPE)).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def trail_plan():
    """(INJECT records, float32 table of peak 1, step): one sigma-2 Gaussian trail of peak 0.02 per frame through a point near
    the frame's middle"""
    from lfd_amd import inject as I
    h, w = SET_SHAPE
    tr = np.zeros(SET_SIZE, IR.TRAIL_DTYPE)
    tr["t0"], tr["t1"] = -np.inf, np.inf
    for i, deg in enumerate(SET_THETA):
        th = math.radians(deg)
        x0, y0 = w / 2 + 7 * (i % 4) - 10, h / 2 - 5 * (i % 3) + 4
        tr[i] = (i, 0, x0 * math.cos(th) + y0 * math.sin(th), th, -np.inf, np.inf, SET_PEAK)
    table, step = I.gaussian_table(2.0)
    return tr, I.normalise_peak(table).astype(np.float32), step


@functools.lru_cache(maxsize=None)
def trail_frames():
    tr, table, step = trail_plan()
    f = IR.inject(noise_frames().copy(), tr, table, step)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def set_records(kind, b):
    """the restatement's records of the noise-only ('noise') or the trail ('trail') frames at bin b, computed once"""
    frames = noise_frames() if kind == "noise" else trail_frames()
    return tuple(R.search(f, SET_SIGMA, bin=b) for f in frames)


def line_error(rec, tr, shape):
    """(angle between the record's line and the trail in degrees, distance of the trail's in-frame midpoint from the line)"""
    from lfd_amd import recovery
    ta, tb = recovery.extent(float(tr["rho"]), float(tr["theta"]), -np.inf, np.inf, shape)
    c, s = math.cos(tr["theta"]), math.sin(tr["theta"])
    tm = 0.5 * (ta + tb)
    mx, my = tr["rho"] * c - tm * s, tr["rho"] * s + tm * c
    dth = (rec["theta"] - tr["theta"] + math.pi / 2) % math.pi - math.pi / 2
    return abs(math.degrees(dth)), abs(mx * math.cos(rec["theta"]) + my * math.sin(rec["theta"]) - rec["rho"])


def dyadic_pixels(n, j, y, s):
    """the (row, column) set of F_n[j][y][s], enumerated by the recursion of step 4"""
    if n == 1:
        return [(y, j)]
    h = n // 2
    return dyadic_pixels(h, 2 * j, y, s >> 1) + dyadic_pixels(h, 2 * j + 1, y + ((s + 1) >> 1), s >> 1)


@pytest.mark.parametrize("shape", [(24, 32), (37, 50)])
def test_transform_equals_brute_force_sums(shape):
    rng = np.random.default_rng(shape[0])
    Q = rng.integers(-9, 10, shape).astype(np.float32)
    M = (rng.random(shape) < 0.8).astype(np.int64)
    Rr, C = shape
    P = R.pow2_at_least(C)
    S, N = R.transform(Q), R.transform(M)
    assert S.shape == N.shape == (Rr + P - 1, P) and S.dtype == np.float32
    for yi in range(Rr + P - 1):
        for s in range(P):
            px = [(r, c) for r, c in dyadic_pixels(P, 0, yi - (P - 1), s) if 0 <= r < Rr and c < C]
            assert len({c for _, c in px}) == len(px)                   # one pixel per column
            assert S[yi, s] == sum(float(Q[r, c]) for r, c in px), (yi, s)
            assert N[yi, s] == sum(int(M[r, c]) for r, c in px), (yi, s)


def test_every_pixel_lies_on_one_line_per_slope():
    rng = np.random.default_rng(3)
    Q = rng.integers(-9, 10, (37, 50)).astype(np.float32)
    S = R.transform(Q)
    assert (S.sum(axis=0, dtype=np.float64) == float(Q.sum(dtype=np.float64))).all()


def test_drawn_line_comes_back():
    Q = np.zeros((96, 128), np.float32)
    for r, c in dyadic_pixels(128, 0, 10, 57):
        Q[r, c] = 1.0
    S = R.transform(Q)
    yi, s = np.unravel_index(np.argmax(S), S.shape)
    assert (yi - 127, s) == (10, 57) and S[yi, s] == 128 and (S == 128).sum() == 1


@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("shape", [(37, 50), (97, 161), (300, 70)])
def test_line_of_agrees_with_the_restatement(shape, b):
    from lfd_amd import radon
    hb, wb, p01, p23 = radon.working_dims(shape, b)
    assert (p01, p23) == (R.pow2_at_least(wb), R.pow2_at_least(hb))
    for q in range(4):
        P, Rr = (p01, hb) if q < 2 else (p23, wb)
        for y0, s in ((0, 0), (-(P - 1), P - 1), (Rr - 1, 0), (3, P // 2), (-2, 5)):
            got, want = radon.line_of(q, y0, s, shape, b), R.line_of(q, y0, s, shape, b)
            assert got == want
            x1, y1, x2, y2, rho, theta = got
            assert 0 <= theta < math.pi
            for x, y in ((x1, y1), (x2, y2)):
                assert abs(x * math.cos(theta) + y * math.sin(theta) - rho) < 1e-9 * max(1.0, abs(rho), abs(x), abs(y))


def test_search_picks_the_line_through_its_own_pixels():
    """the record's line, mapped to the frame, passes through the pixels of a drawn streak in every orientation"""
    h, w = 60, 90
    for q, (dx, dy) in enumerate(((1.0, 0.4), (1.0, -0.4), (0.4, 1.0), (-0.4, 1.0))):
        f = np.zeros((h, w), np.float32)
        t = np.linspace(-80, 80, 2000)
        x, y = np.rint(w / 2 + t * dx).astype(int), np.rint(h / 2 + t * dy).astype(int)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        f[h - 1 - y[ok], x[ok]] = 0.1                                  # (x, y) of the flipped frame is buffer row H-1-y
        rec = R.search(f, bin=1, min_len=8)
        assert rec["q"] == q and rec["found"] == 1
        th = math.atan2(-dx, dy) % math.pi
        assert abs((rec["theta"] - th + math.pi / 2) % math.pi - math.pi / 2) < math.radians(2.0)
        assert abs(w / 2 * math.cos(rec["theta"]) + h / 2 * math.sin(rec["theta"]) - rec["rho"]) < 2.0


def test_invalid_pixels_are_neither_summed_nor_counted():
    f = np.full((8, 8), 0.01, np.float32)
    f[0, 0], f[1, 1], f[2, 2], f[3, 3], f[4, 4], f[5, 5] = np.nan, np.inf, -np.inf, 0.0, -0.0, 0.2
    V, M = R.prepare(f, 2, 0.125)
    assert M.sum() == 64 - 6 and M.dtype == np.int64
    assert V.dtype == np.float32 and V[3, 0] == np.float32(0.01) + np.float32(0.01)   # flipped: buffer rows 0, 1 hold NaN and inf
    rec = R.search(f, bin=1, min_len=100)
    assert rec["status"] == R.NO_LINE and rec["snr"] == 0 and rec["found"] == 0


def test_parameter_validation():
    from lfd_amd import radon
    assert radon.default_params() == radon.RadonParams(bin=2, clip=0.125, min_len=256, threshold=8.0)
    assert radon.as_params(None) == {} and radon.as_params({"bin": 4}) == {"bin": 4}
    for bad in ({"bin": 3}, {"bin": 0}, {"clip": 0.0}, {"clip": float("nan")}, {"min_len": 0}, {"threshold": float("nan")}):
        with pytest.raises(ValueError):
            radon.as_params(bad)
        with pytest.raises(ValueError):
            radon.RadonParams(**bad).validate()
    with pytest.raises(TypeError):
        radon.as_params({"bins": 2})
    with pytest.raises(ValueError):
        radon.line_of(4, 0, 0, (10, 10), 1)
    with pytest.raises(ValueError):
        radon.line_of(0, 0, 0, (10, 10), 3)


@pytest.mark.parametrize("b", [1, 2])
def test_noise_only_frames_stay_below_the_default_threshold(b):
    snr = [float(r["snr"]) for r in set_records("noise", b)]
    print("noise-only snr at bin", b, ["%.2f" % v for v in snr])
    assert all(r["status"] == R.OK and r["found"] == 0 for r in set_records("noise", b))
    assert max(snr) < 8.0


@pytest.mark.parametrize("b", [1, 2])
def test_faint_trails_are_found_in_every_orientation(b):
    tr, _, _ = trail_plan()
    recs = set_records("trail", b)
    errs = [line_error(r, tr[i], SET_SHAPE) for i, r in enumerate(recs)]
    print("bin", b, "snr", ["%.1f" % float(r["snr"]) for r in recs], "errors (deg, px)", [("%.2f" % a, "%.2f" % d) for a, d in errs])
    assert [r["q"] for r in recs] == list(SET_Q)
    assert all(r["found"] == 1 for r in recs)
    assert max(a for a, _ in errs) <= 0.5 and max(d for _, d in errs) <= 4.0
