"""Trail profiles (include/lfdmi.h: lfdmi_measure_trails) on the CPU: the definition, restated in tests/trail_ref.py, against
ground truth on synthetic frames, and its fwhm / depth against the reference's definitions.  The device is checked against the
same restatement in tests/test_gpu_trail_profiles.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trail_ref as T  # noqa: E402

from lfd_amd import synth  # noqa: E402

H, W = 1489, 2048
SIGMA = 2.0


def truth_line(y0, x0, ang, h=H):
    """rho, theta (flipped frame) of synth._add_streak's line through buffer (row y0, column x0) at angle ang"""
    phi = math.radians(ang)
    nx, ny = math.sin(phi), math.cos(phi)          # y = h-1-row
    rho = x0 * nx + (h - 1 - y0) * ny
    if ny < 0 or (ny == 0 and nx < 0):
        nx, ny, rho = -nx, -ny, -rho
    return rho, math.atan2(ny, nx)


def hough_record(rho, theta, drho=0.0, dtheta=0.0):
    """the record's line: the truth on HoughLines' grid (rho 20 px, theta 1 degree) plus an extra offset, as float32"""
    th = round(math.degrees(theta)) * math.pi / 180 + dtheta
    return np.float32(round(rho / 20.0) * 20.0 + drho), np.float32(th)


def streak_frame(y0, x0, ang, peak=1.0, seed=0, profile=None, half_len=None, h=H, w=W):
    rng = np.random.default_rng(seed)
    img = rng.normal(0.0, 0.025, (h, w)).astype(np.float32)
    if profile is None and half_len is None:
        synth._add_streak(img, y0, x0, ang, peak, SIGMA)
        return img
    phi = math.radians(ang)
    yy = np.arange(h, dtype=np.float64)[:, None]
    xx = np.arange(w, dtype=np.float64)[None, :]
    d = (xx - x0) * math.sin(phi) - (yy - y0) * math.cos(phi)
    a = (xx - x0) * math.cos(phi) + (yy - y0) * math.sin(phi)
    prof = profile(d) if profile is not None else np.exp(-d * d / (2 * SIGMA * SIGMA))
    if half_len is not None:
        prof = prof * (np.abs(a) <= half_len)
    img += (peak * prof).astype(np.float32)
    return img


def line_error(rho, theta, y0, x0, ang, h=H, w=W):
    """largest distance of the line (rho, theta) from the truth over the truth's run across the frame"""
    phi = math.radians(ang)
    a = np.linspace(-4000, 4000, 16001)
    x = x0 + a * math.cos(phi)
    row = y0 + a * math.sin(phi)
    ins = (x >= 0) & (x <= w - 1) & (row >= 0) & (row <= h - 1)
    x, y = x[ins], (h - 1 - row)[ins]
    return float(np.max(np.abs(x * math.cos(theta) + y * math.sin(theta) - rho)))


@pytest.mark.parametrize("y0,x0,ang", [(700.3, 1000.7, 30.0), (811.0, 1203.4, 62.5), (650.8, 900.2, 121.0), (744.5, 1024.5, 12.0)])
def test_refined_line_and_fwhm_against_truth(y0, x0, ang):
    img = streak_frame(y0, x0, ang, seed=int(ang))
    rho, theta = truth_line(y0, x0, ang)
    hr, ht = hough_record(rho, theta, drho=7.0, dtheta=math.radians(0.3))
    rec, prof = T.measure(img, hr, ht)
    assert rec["status"] == T.OK
    err = line_error(rec["rho"], rec["theta"], y0, x0, ang)
    err_hough = line_error(float(hr), float(ht), y0, x0, ang)
    assert err < 0.2, (err, err_hough)
    assert err_hough > 1.0                      # the Hough line is worse on the same frame
    assert abs(rec["fwhm"] - 2.3548 * SIGMA) < 0.03 * 2.3548 * SIGMA, rec["fwhm"]
    assert rec["fwhm_arcsec"] == rec["fwhm"] * T.DEFAULTS["pixscale"]
    assert abs(rec["depth"]) < 2.0
    assert 0.9 < rec["peak"] < 1.05 and abs(rec["background"]) < 0.01
    assert rec["fwhm"] == T.calc_fwhm(prof, (np.arange(len(prof)) - len(prof) // 2) * T.DEFAULTS["prof_step"])


def test_doughnut_depth():
    # two Gaussians of sigma 3 px, 9 px apart: a 36 % dip, wide enough for bilinear sampling of the pixel grid to keep it
    s, sd = 4.5, 3.0
    dough = lambda d: np.exp(-(d - s) ** 2 / (2 * sd ** 2)) + np.exp(-(d + s) ** 2 / (2 * sd ** 2))  # noqa: E731
    g = np.linspace(-10, 10, 200001)
    fg = dough(g)
    dip = (fg.max() - dough(np.array([0.0]))[0]) / fg.max() * 100
    y0, x0, ang = 720.0, 1030.0, 40.0
    img = streak_frame(y0, x0, ang, profile=dough, seed=3)
    rho, theta = truth_line(y0, x0, ang)
    rec, prof = T.measure(img, *hough_record(rho, theta, drho=-6.0))
    assert rec["status"] == T.OK
    assert line_error(rec["rho"], rec["theta"], y0, x0, ang) < 0.2
    assert abs(rec["depth"] - dip) < 2.0, (rec["depth"], dip)
    assert rec["depth"] == T.depth(prof, np.float32(rec["peak"]))


def test_partial_trail_extent():
    y0, x0, ang, half = 760.0, 1010.0, 25.0, 500.0
    img = streak_frame(y0, x0, ang, half_len=half, seed=5)
    rho, theta = truth_line(y0, x0, ang)
    rec, _ = T.measure(img, *hough_record(rho, theta, drho=5.0))
    assert rec["status"] == T.OK
    phi = math.radians(ang)
    ends = [(x0 + a * math.cos(phi), H - 1 - (y0 + a * math.sin(phi))) for a in (-half, half)]
    got = [(rec["x1"], rec["y1"]), (rec["x2"], rec["y2"])]
    for gx, gy in got:
        assert min(math.hypot(gx - ex, gy - ey) for ex, ey in ends) < T.DEFAULTS["seg_len"]
    assert abs(math.dist(*got) - 2 * half) < 2 * T.DEFAULTS["seg_len"]
    L = T.DEFAULTS["seg_len"]
    assert (rec["n_seg"] - 1) * L < rec["n_pos"] <= rec["n_seg"] * L      # whole segments, the last one possibly partial
    assert abs(rec["n_pos"] - 2 * half) < 2 * L                           # a 1000-px trail: its positions, to a segment per end


def test_corner_line_is_too_short_and_diagonal_through_a_corner_is_measured():
    img = streak_frame(700.0, 1000.0, 30.0, seed=7)
    rec, prof = T.measure(img, np.float32(60.0), np.float32(math.pi / 4))   # cuts the corner at the origin: ~170 px
    assert rec["status"] == T.TOO_SHORT and np.isnan(prof).all() and math.isnan(rec["fwhm"])
    # a trail along the frame's diagonal, from corner to corner
    ang = math.degrees(math.atan2(H - 1, W - 1))
    img = streak_frame(0.0, 0.0, ang, seed=8)
    rho, theta = truth_line(0.0, 0.0, ang)
    rec, _ = T.measure(img, *hough_record(rho, theta, drho=4.0))
    assert rec["status"] == T.OK
    assert line_error(rec["rho"], rec["theta"], 0.0, 0.0, ang) < 0.2


def test_no_trail_is_too_faint_and_not_found():
    img = np.random.default_rng(9).normal(0.0, 0.025, (H, W)).astype(np.float32)
    rec, prof = T.measure(img, np.float32(900.0), np.float32(0.6))
    assert rec["status"] == T.TOO_FAINT and np.isnan(prof).all()
    rec, prof = T.measure(img, np.float32(900.0), np.float32(0.6), found=0)
    assert rec["status"] == T.NOT_FOUND and np.isnan(prof).all()


def test_star_squares_and_bad_pixels_are_left_out():
    y0, x0, ang = 700.0, 1000.0, 35.0
    img = streak_frame(y0, x0, ang, seed=11)
    rho, theta = truth_line(y0, x0, ang)
    r = hough_record(rho, theta, drho=3.0)
    star = np.zeros(img.shape, bool)
    star[690:720, 985:1015] = True               # a square on the trail
    blotted = img.copy()
    blotted[star] = 0.0
    a, pa = T.measure(img, *r, star_mask=star)
    b, pb = T.measure(blotted, *r, star_mask=star)
    assert a == b and np.array_equal(pa, pb)
    bad = img.copy()
    bad[400, 500:520] = np.nan
    bad[900, 1200] = np.inf
    c, pc = T.measure(bad, *r)
    assert c["status"] == T.OK and np.isfinite(pc).all()


# ---- the reference's definitions on hand-built arrays --------------------------------------------------------------------------
def ref_calc_fwhm(obj, scale):
    """ConvolutionObject.calc_fwhm, lfd/analysis/profiles/convolutionobj.py:160-178, as written there (self.peak = obj.max())"""
    peak = obj.max()
    left = np.where(obj >= peak / 2.)[0][0]
    right = np.where(obj >= peak / 2.)[0][-1]
    if left == right:
        return 0.0
    return abs(scale[right]) + abs(scale[left])


def ref_depth(obj):
    """samplers.py:158-162"""
    mid = obj[int(len(obj) / 2)]
    return (obj.max() - mid) / obj.max() * 100.0


@pytest.mark.parametrize("obj", [
    np.array([0, 1, 3, 7, 10, 7, 3, 1, 0], np.float32),                 # symmetric
    np.array([0, 0, 2, 9, 10, 8, 6, 5, 4, 1, 0], np.float32),           # asymmetric
    np.array([0, 5, 5, 5, 5, 5, 5, 5, 0], np.float32),                  # flat top
    np.array([0, 1, 8, 10, 4, 10, 8, 1, 0], np.float32),                # doughnut
    np.array([0, 0, 0, 0, 10, 0, 0, 0, 0], np.float32),                 # one bin: fwhm 0
])
def test_fwhm_and_depth_follow_the_reference(obj):
    scale = (np.arange(len(obj)) - len(obj) // 2) * 0.25
    assert T.calc_fwhm(obj, scale) == ref_calc_fwhm(obj, scale)
    assert T.depth(obj) == pytest.approx(ref_depth(obj), rel=1e-6)


def test_hand_values():
    scale = (np.arange(9) - 4) * 0.5
    assert T.calc_fwhm(np.array([0, 1, 3, 7, 10, 7, 3, 1, 0], np.float32), scale) == 1.0
    assert T.calc_fwhm(np.array([0, 5, 5, 5, 5, 5, 5, 5, 0], np.float32), scale) == 3.0
    assert T.depth(np.array([0, 1, 8, 10, 4, 10, 8, 1, 0], np.float32)) == 60.0


def test_library_defaults_match_the_definition():
    from lfd_amd import _native
    p = _native.make_trail_params()
    assert {k: getattr(p, k) for k, _ in p._fields_} == T.DEFAULTS
    assert _native.trail_bins(p) == T.n_bins()
    assert _native.TRAIL_DTYPE.names == T.FIELDS
    with pytest.raises(TypeError):
        _native.make_trail_params(width=3)
