"""What a preview shows, measured on the restatement (tests/preview_ref.py): eight 372 x 512 frames of sigma-0.025 noise, each
with a Gaussian trail of sigma 2 px and peak 0.02 (0.8 sigma per pixel: invisible at full resolution) at its own angle, at the
defaults (bin 4, ranks 10000 and 995000 ppm) through the asinh table.  The bound below is the extreme measured over the eight
frames with the margin stated beside it; and the overlay's rails are checked to leave the trail itself visible."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402

from lfd_amd import masks, previews  # noqa: E402

H, W, BIN, SIGMA, PEAK, WIDTH = 372, 512, 4, 0.025, 0.02, 2.0
ANGLES = (10.0, 35.0, 60.0, 85.0, 100.0, 125.0, 150.0, 175.0)


def line(angle):
    """a segment through the frame's middle at `angle` degrees, in flipped coordinates, far longer than the frame"""
    a = math.radians(angle)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return cx - 1000.0 * math.cos(a), cy - 1000.0 * math.sin(a), cx + 1000.0 * math.cos(a), cy + 1000.0 * math.sin(a)


def distance(x1, y1, x2, y2, x, y):
    L = math.hypot(x2 - x1, y2 - y1)
    return ((x - x1) * -(y2 - y1) / L) + ((y - y1) * (x2 - x1) / L)


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(20240607)
    out = np.empty((len(ANGLES), H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i, a in enumerate(ANGLES):
        u = distance(*line(a), xx, yy)
        flipped = rng.normal(0.0, SIGMA, (H, W)) + PEAK * np.exp(-0.5 * (u / WIDTH) ** 2)
        out[i] = flipped[::-1]                              # buffer rows
    return out


@functools.lru_cache(maxsize=None)
def previews_of_them():
    return R.frame_previews(frames(), previews.lut("asinh"), bin=BIN)


def cell_distance(angle):
    hp, wp = -(-H // BIN), -(-W // BIN)
    y = ((np.arange(hp) + 0.5) * BIN - 0.5)[:, None]
    x = ((np.arange(wp) + 0.5) * BIN - 0.5)[None, :]
    return distance(*line(angle), x, y)


def contrasts():
    out, _, rec = previews_of_them()
    res = []
    for i, a in enumerate(ANGLES):
        on = np.abs(cell_distance(a)) <= BIN / 2.0          # the cells the line runs through
        img = out[i].astype(np.float64)
        med = np.median(img)
        scatter = 1.4826 * np.median(np.abs(img - med))
        res.append((np.median(img[on]) - med) / scatter)
    return res


def test_every_frame_is_ok_and_uses_the_table():
    out, cells, rec = previews_of_them()
    assert (rec["status"] == R.OK).all() and (rec["n_empty"] == 0).all() and (rec["n_cells"] == 93 * 128).all()
    assert out.min() == 0 and out.max() == 255
    assert ((rec["lo_f"] < 0) & (rec["hi_f"] > 0)).all()


def test_a_faint_trail_stands_out_after_binning():
    """The median byte on the cells the line runs through, above the frame's median byte, in units of the frame's byte scatter
    (1.4826 times the median absolute deviation): measured 1.59 .. 1.83 over the eight angles.  A pixel of the trail's ridge is
    0.8 sigma above the noise; a cell of 16 pixels has noise of sigma / 4 and, up to half a cell off the line, between 0.5 and
    0.85 of the peak, so 1.6 .. 2.7 is what the binning alone promises, and the asinh table, nearly linear this low, keeps it.
    Asserted with a margin of 15 % under the measured minimum."""
    c = contrasts()
    assert min(c) >= 1.59 * 0.85, c
    assert max(c) <= 3.0, c                                 # (a trail that outshone this would be a mistake in the test's own frames)


def test_the_rails_leave_the_trail_visible():
    out, _, _ = previews_of_them()
    half = 10.0
    for i, a in enumerate(ANGLES):
        seg = masks.segments([(0, *line(a), half)], cap=float("inf"))
        rgb = previews.overlay(out[i], seg, BIN, color=(255, 0, 255))
        marked = (rgb != out[i][:, :, None]).any(axis=2) | ((rgb[:, :, 0] == 255) & (rgb[:, :, 1] == 0) & (rgb[:, :, 2] == 255))
        u = cell_distance(a)
        assert not marked[np.abs(u) < half].any(), a        # never a cell within half of the line
        assert marked[(u >= half) & (u <= half + BIN)].all() and marked[(u <= -half) & (u >= -half - BIN)].all(), a
        assert not marked[np.abs(u) > half + BIN].any(), a
        assert (rgb[~marked] == out[i][~marked][:, None]).all(), a


def test_overlay_respects_cap_and_skips_bad_segments():
    gray = np.full((20, 30), 100, np.uint8)
    seg = masks.segments([(0, 20.0, 40.0, 60.0, 40.0, 4.0)], cap=0.0)     # a horizontal piece, x 20 .. 60, at y = 40
    rgb = previews.overlay(gray, seg, 4, color=(1, 2, 3))
    marked = (rgb != 100).any(axis=2)
    # centres: x = 4 i + 1.5, y = 4 r + 1.5; rails 4 <= |y - 40| <= 8: rows r = 8 (33.5), 11 (45.5); 20 <= x <= 60: i = 5 .. 14
    assert sorted(set(np.nonzero(marked)[0])) == [8, 11] and sorted(set(np.nonzero(marked)[1])) == list(range(5, 15))
    assert (rgb[marked] == (1, 2, 3)).all()
    bad = masks.segments([(0, 5.0, 5.0, 5.0, 5.0, 4.0), (0, float("nan"), 0.0, 1.0, 1.0, 4.0)])
    assert (previews.overlay(gray, bad, 4) == 100).all()
