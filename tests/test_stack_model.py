"""The stacked cross-sections on the CPU (include/lfdmi.h: stacked cross-sections), restatement only (tests/stack_ref.py): a block
worked out by hand, the trails of test_radon_model's set measured from a perturbed start line, and its noise-only frames."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stack_ref as S  # noqa: E402
import test_radon_model as TM  # noqa: E402

OFF_PX, OFF_DEG = 1.5, 0.15                      # how far the start line is from the trail
TRUE_FWHM = 2.0 * math.sqrt(2.0 * math.log(2.0)) * 2.0   # Gaussian sigma 2 px
TRUE_FLUX = TM.SET_PEAK * 2.0 * math.sqrt(2.0 * math.pi)
# 1.5 times the largest error of the restatement over the 16 trails (angle 0.154 degrees, centre 0.511 px, fwhm 3.0 against 4.71,
# flux 0.0773 against 0.1003), for another seed
TOL_DEG, TOL_PX, TOL_FWHM, TOL_FLUX = 1.5 * 0.154, 1.5 * 0.511, 1.5 * 1.71, 1.5 * 0.0230


def start_segment(t, shape, off=OFF_PX, ddeg=OFF_DEG):
    """the in-frame crossing of trail t's line moved by ``off`` px along its normal and turned by ``ddeg`` about its middle"""
    from lfd_amd import recovery
    th0 = float(t["theta"])
    c0, s0 = math.cos(th0), math.sin(th0)
    ta, tb = recovery.extent(float(t["rho"]), th0, -np.inf, np.inf, shape)
    tm = 0.5 * (ta + tb)
    mx, my = t["rho"] * c0 - tm * s0 + off * c0, t["rho"] * s0 + tm * c0 + off * s0
    th = th0 + math.radians(ddeg)
    c, s = math.cos(th), math.sin(th)
    rho = mx * c + my * s
    a, b = recovery.extent(rho, th, -np.inf, np.inf, shape)
    return rho * c - a * s, rho * s + a * c, rho * c - b * s, rho * s + b * c


@functools.lru_cache(maxsize=None)
def set_measurements(kind):
    """the restatement's (record, row, sums, counts) of every frame of the set, computed once"""
    frames = TM.noise_frames() if kind == "noise" else TM.trail_frames()
    tr = TM.trail_plan()[0]
    return tuple(S.measure(frames[i], start_segment(tr[i], TM.SET_SHAPE), TM.SET_SIGMA) for i in range(TM.SET_SIZE))


def test_one_block_by_hand():
    """6 x 8 pixels, the horizontal line y = 2.25 from x = 0 to 7, P = 1, step = 1 (K = 1, three bins): t = (y - 2.25) + 1.5, so rows y = 1, 2, 3 fall in bins 0, 1, 2 (t = 0.25, 1.25, 2.25) and rows 0, 4, 5 in
    none (t = -0.75, 3.25, 4.25).  Columns 0 .. 3 are the left half, 4 .. 7 the right one."""
    img = np.zeros((6, 8), np.float32)
    flipped = img[::-1]                              # flipped[y, x]
    flipped[1] = 0.01 * np.arange(1, 9)
    flipped[2] = 0.05
    flipped[3] = [0.02, np.nan, 0.0, 0.2, -0.03, np.inf, -0.0, 0.04]     # NaN, +-0, above clip and inf are not summed
    flipped[0] = flipped[4] = flipped[5] = 0.07      # outside the band
    rec, row, A, N = S.measure(img, (0.0, 2.25, 7.0, 2.25), prof_half=1.0, step=1.0, wing=1, min_cols=8, n_iter=0, k_sig=0.0)
    f = np.float32
    assert N.tolist() == [[4, 4, 1], [4, 4, 2]]
    assert A[0].tolist() == [((f(0.01) + f(0.02)) + f(0.03)) + f(0.04), ((f(0.05) + f(0.05)) + f(0.05)) + f(0.05), f(0.02)]
    assert A[1].tolist() == [((f(0.05) + f(0.06)) + f(0.07)) + f(0.08), ((f(0.05) + f(0.05)) + f(0.05)) + f(0.05), f(-0.03) + f(0.04)]
    m = [(A[0][k] + A[1][k]) / f(N[0][k] + N[1][k]) for k in range(3)]
    bg = sorted(m)[1]                                # P - wing = 0: all three bins are wing bins, none is a core bin
    assert row.tolist() == [m[0] - bg, m[1] - bg, m[2] - bg]
    assert rec["status"] == S.OK and rec["n_col"] == 8 and rec["min_valid"] == 3 and rec["n_pass"] == 1
    assert (rec["x1"], rec["y1"], rec["x2"], rec["y2"]) == (0.0, 2.25, 7.0, 2.25) and rec["theta"] == math.pi / 2 and rec["rho"] == 2.25
    assert rec["shift"] == 0.0 and rec["tilt"] == 0.0 and rec["background"] == float(bg)
    assert rec["flux"] == 0.0 and rec["peak"] == float(max(m) - bg)      # no core bin: |u| < 0 holds for none


def test_trails_come_back():
    tr = TM.trail_plan()[0]
    for i, (rec, row, A, N) in enumerate(set_measurements("trail")):
        assert rec["status"] == S.OK and rec["n_pass"] == 3, i
        ang, dist = TM.line_error(rec, tr[i], TM.SET_SHAPE)
        assert ang <= TOL_DEG and dist <= TOL_PX, (i, ang, dist)
        assert abs(rec["fwhm"] - TRUE_FWHM) <= TOL_FWHM and abs(rec["flux"] - TRUE_FLUX) <= TOL_FLUX, (i, rec["fwhm"], rec["flux"])
        assert rec["peak"] >= S.DEFAULTS["k_sig"] * rec["noise"] and rec["snr"] > 8 and not np.isnan(row).any()
        assert abs(rec["shift"]) > 0.5 and int(N.sum()) > 40 * rec["n_col"]


def test_noise_only_frames_are_too_faint():
    for rec, row, A, N in set_measurements("noise"):
        assert rec["status"] == S.TOO_FAINT and rec["n_pass"] == 1           # and the line was not moved
        assert rec["shift"] == 0.0 and rec["tilt"] == 0.0
        assert 0 < rec["peak"] < S.DEFAULTS["k_sig"] * rec["noise"] and not np.isnan(row).any()


def test_segments_that_cannot_be_measured():
    img = TM.noise_frames()[0]
    nb = S.n_bins()
    for seg, want in (((10.0, 10.0, 10.0, 10.0), S.BAD_SEGMENT), ((math.nan, 0.0, 5.0, 5.0), S.BAD_SEGMENT),
                      ((0.0, 0.0, 2e6, 5.0), S.BAD_SEGMENT), ((100.0, 50.0, 130.0, 60.0), S.TOO_SHORT),
                      ((-500.0, 50.0, -100.0, 60.0), S.TOO_SHORT)):
        rec, row, A, N = S.measure(img, seg)
        assert rec["status"] == want and np.isnan(row).all() and row.shape == (nb,) and not A.any() and not N.any()
        assert all(math.isnan(rec[k]) for k in S.F64_FIELDS)
