"""The wide-trail search on the CPU (include/lfdmi.h: faint-trail search, steps 13 - 16), on its numpy restatement
(tests/radon_wide_ref.py) only: max_width = 1 against radon_lines_ref, the doubling sums against a direct band count, the
noise figures the default wide_threshold rests on, wide faint trails the plain search misses, and a crossing narrower trail
found after the band's peel."""
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
import radon_wide_ref as W  # noqa: E402
import test_radon_lines_model as TL  # noqa: E402
import test_radon_model as TM  # noqa: E402

WIDE_SIGMA_PX = 6.0
# one peak for all sixteen trails (test_radon_model's plan, Gaussian sigma 6 px), the issue's starting value: at bin 2 the plain
# search scores them 5.3 - 7.9 and finds none, the wide search 9.9 - 14.3 and finds all, each at width 8.  (0.0035: 15 of 16
# wide, 0 plain; 0.004: 16 and 0; 0.005: 16 and 2; 0.0055: 16 and 4.)
WIDE_PEAK = 0.0045
# the largest error of the restatement's centre line over those sixteen (1.162 degrees, 3.532 px from the trail's midpoint),
# times 1.5 for another seed
CENTRE_TOL = (1.5 * 1.162, 1.5 * 3.532)


@functools.lru_cache(maxsize=None)
def wide_trail_frames():
    from lfd_amd import inject as I
    tr = TM.trail_plan()[0].copy()
    tr["amplitude"] = WIDE_PEAK
    table, step = I.gaussian_table(WIDE_SIGMA_PX)
    f = IR.inject(TM.noise_frames().copy(), tr, I.normalise_peak(table).astype(np.float32), step)
    f.setflags(write=False)
    return tr, f


@pytest.mark.parametrize("k,b", TL.TWO_CASES)
def test_max_width_1_is_the_several_lines_search(k, b):
    want, want_n = TL.two_trail_lines(k, b)
    got, got_n, plain = W.search_wide(TL.two_trail_frame(k), TM.SET_SIGMA, max_width=1, bin=b)
    assert got_n == want_n == 2
    for g, w in zip(got, want):
        for key, v in w.items():
            assert type(g[key]) is type(v) and (g[key] == v or key in ("sum", "snr", "seg_sum", "seg_snr") and g[key].tobytes() == v.tobytes()), key
        assert g["width"] == (1 if w["status"] == R.OK and w["n_pix"] else 0)
        if g["width"]:
            P = R.pow2_at_least(-(-TM.SET_SHAPE[1 if g["q"] < 2 else 0] // b))
            assert g["width_px"] == b * ((P - 1) / math.sqrt((P - 1) ** 2 + g["s"] ** 2)) and 0.7 * b <= g["width_px"] <= b
    for key, v in plain.items():                                       # and round 0's width-1 pass is the plain search
        assert got[0][key] == v, key


@pytest.mark.parametrize("shape,maxw", [((9, 16), 16), ((21, 5), 8), ((3, 8), 4)])
def test_doubling_sums_equal_a_direct_band_count(shape, maxw):
    rng = np.random.default_rng(shape[0])
    Q = rng.integers(-9, 10, shape).astype(np.float32)                 # small integers: every float32 sum is exact
    M = (rng.random(shape) < 0.8).astype(np.int64)
    Rr, C = shape
    P = R.pow2_at_least(C)
    S, N = R.transform(Q), R.transform(M)
    cols = np.arange(C)
    seen = []
    for k, B, Cn in W.bands(S, N, maxw):
        seen.append(k)
        assert B.dtype == np.float32 and B.shape == S.shape == Cn.shape
        for s in range(P):
            d = L.dyadic_path(s, P)[:C]
            for yi in range(Rr + P - 1):
                tot, cnt = 0.0, 0
                for u in range(k):                                     # lines y .. y+k-1 of slope s share no pixel
                    rows = yi - (P - 1) + u + d
                    ok = (rows >= 0) & (rows < Rr)
                    tot += float(Q[rows[ok], cols[ok]].sum())
                    cnt += int(M[rows[ok], cols[ok]].sum())
                assert B[yi, s] == tot and Cn[yi, s] == cnt, (k, s, yi)
    assert seen == [w for w in (1, 2, 4, 8, 16) if w <= maxw]


@pytest.mark.parametrize("b", [1, 2])
def test_noise_only_frames_stay_below_the_default_threshold_at_every_width(b):
    """DESIGN.md (Wide trails) records these: bin 1 peaks at 5.33, 5.02, 4.91, 4.88, 4.51 for widths 1 .. 16, bin 2 at 4.92, 4.65,
    4.79, 4.34, 4.13"""
    top = {}
    for f in TM.noise_frames():
        wd = {}
        recs, n_lines, _ = W.search_wide(f, TM.SET_SIGMA, max_width=16, bin=b, widths=wd)
        assert n_lines == 0 and recs[0]["status"] == R.OK and recs[0]["found"] == 0 and all(r == W.ZERO for r in recs[1:])
        for k, v in wd.items():
            top[k] = max(top.get(k, -np.inf), v)
    print("noise-only largest score per width at bin", b, {k: "%.2f" % v for k, v in sorted(top.items())})
    assert sorted(top) == [1, 2, 4, 8, 16]
    assert max(top.values()) < W.WIDE_DEFAULTS["wide_threshold"]


def test_wide_faint_trails_the_plain_search_misses():
    tr, frames = wide_trail_frames()
    out = [W.search_wide(f, TM.SET_SIGMA, max_lines=1, bin=2) for f in frames]
    recs = [o[0][0] for o in out]
    plain = [o[2] for o in out]
    errs = [TM.line_error(r, tr[i], TM.SET_SHAPE) for i, r in enumerate(recs)]
    print("plain snr", ["%.1f" % float(p["snr"]) for p in plain], "wide snr", ["%.1f" % float(r["snr"]) for r in recs],
          "width", [r["width"] for r in recs], "errors (deg, px)", [("%.2f" % a, "%.2f" % d) for a, d in errs])
    assert sum(p["found"] for p in plain) == 0
    assert sum(r["found"] for r in recs) == len(recs) == 16
    assert [r["q"] for r in recs] == list(TM.SET_Q)
    assert all(r["width"] >= 4 for r in recs)
    assert all(4.0 * 2 * 0.7 <= r["width_px"] <= r["width"] * 2 for r in recs)
    assert max(a for a, _ in errs) <= CENTRE_TOL[0] and max(d for _, d in errs) <= CENTRE_TOL[1]


def test_a_crossing_narrower_trail_is_found_after_the_band_peel():
    """a sigma-6 trail of peak 0.009 and a crossing sigma-2 trail of peak 0.015 on one noise frame at bin 2: the band first,
    the narrower band in round 2, and the round that stops the frame is noise"""
    from lfd_amd import inject as I
    h, w = TM.SET_SHAPE
    noise = TL.two_trail_noise(0).copy()
    tr = np.zeros(2, IR.TRAIL_DTYPE)
    for i, (deg, peak) in enumerate(((115, 0.009), (20, 0.015))):
        th = math.radians(deg)
        x0, y0 = w / 2 + 7 * i - 10, h / 2 - 5 * i + 4
        tr[i] = (0, 0, x0 * math.cos(th) + y0 * math.sin(th), th, -np.inf, np.inf, peak)
    for i, sig in enumerate((WIDE_SIGMA_PX, 2.0)):
        table, step = I.gaussian_table(sig)
        IR.inject(noise, tr[i:i + 1], I.normalise_peak(table).astype(np.float32), step)
    recs, n_lines, _ = W.search_wide(noise[0], TM.SET_SIGMA, bin=2)
    print("snr", ["%.2f" % float(r["snr"]) for r in recs], "width", [r["width"] for r in recs])
    assert n_lines == 2
    for r, t, tol in zip(recs[:2], tr, (CENTRE_TOL, (0.5, 4.0))):       # (the narrow one: test_radon_lines_model's bounds)
        a, d = TM.line_error(r, t, TM.SET_SHAPE)
        assert a <= tol[0] and d <= tol[1], (a, d)
        assert r["found"] == 1 and r["seg_n_pix"] >= 64 * r["width"] // 2 and 0 <= r["c1"] <= r["c2"]
    assert recs[0]["width"] >= 4 and recs[1]["width"] < recs[0]["width"]
    stop = recs[2]
    assert stop["status"] == R.OK and stop["found"] == 0 and float(stop["snr"]) < 8.0 and stop["c2"] == 0 and stop["width"] >= 1
    assert recs[3] == W.ZERO
