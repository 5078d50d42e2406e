"""The source finder at the smallest shapes that cross each of its tiling constants (lfd_amd/csrc/stars/k_stars.h), bit for bit
against the restatement (tests/stars_ref.py):

  STR_TW = 64, STR_TH = 16   the tile of k_stars_detect; a word of the bit plane is one tile row (frames narrower than, exactly,
                             and one more than a tile; sources on the seams and in the corners)
  halo = sep + 1             sep = 1 and sep = 8 (STR_MAX_SEP); ties across a seam
  64 lanes per ballot        a row with more than 64 candidates (two words, and the popcount walk of k_stars_measure)
  STR_THREADS = 256          k_stars_rows gives a thread ceil(h / 256) rows: h = 300 takes two
  STR_MAX_R = 32, STR_PW     rad = 1, rad = r_max, and the first source that fails r_max (EXTENDED); rings longer than a wave
                             (8 r > 64 from r = 9); the patch clipped at all four corners
  max_obj                    fewer slots than candidates (TRUNCATED: the first max_obj in raster order), and no candidate at all
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402
from test_gpu_stars import assert_records  # noqa: E402

pytestmark = pytest.mark.gpu


def check(ctx, frames, sigma=None, **params):
    """the device against the restatement on these frames; returns the restatement's (records, frame records)"""
    frames = np.ascontiguousarray(frames, np.float32)
    want = R.find_stars_batch(frames, sigma, **params)
    assert_records(ctx.find_stars(frames, sigma=sigma, **params), want, params)
    be = frames.astype(">f4")
    assert_records(ctx.find_stars(be, sigma=sigma, **params), want, ("big-endian", params))
    return want


def blob(img, y, x, peak, s=1.0, half=4):
    """an exact little source: peak / (1 + d2 / s) on a (2 half + 1)^2 stamp, clipped to the frame"""
    h, w = img.shape
    for yy in range(max(y - half, 0), min(y + half + 1, h)):
        for xx in range(max(x - half, 0), min(x + half + 1, w)):
            img[yy, xx] += np.float32(peak / (1.0 + ((yy - y) ** 2 + (xx - x) ** 2) / s))


def live(rec, frec):
    return [rec[i, :int(frec[i]["n_out"])] for i in range(len(frec))]


@pytest.mark.parametrize("shape", [(70, 33), (16, 64), (17, 65), (33, 129)])
def test_frame_sizes_corners_and_seams(gpu_ctx, shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    frames = rng.normal(0, 0.025, (3, h, w)).astype(np.float32)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):          # the four corners
        blob(frames[0], y, x, 3.0)
    seams_x = [x for x in (31, 32, 63, 64, 65, 127, 128) if x < w]
    seams_y = [y for y in (15, 16, 17, 31, 32, 47, 48) if y < h]
    for k, x in enumerate(seams_x):                                          # on and beside the tile seams
        blob(frames[1], seams_y[k % len(seams_y)] if seams_y else h // 2, x, 2.0 + k, half=2)
    for k, y in enumerate(seams_y):
        blob(frames[2], y, (k * 13 + 5) % w, 2.0 + k, half=2)
    frames[2, h // 2, w // 2] = np.nan
    for sep in (1, 3, 8):
        rec, frec = check(gpu_ctx, frames, sep=sep, max_obj=64)
        assert frec["n_found"].min() >= 1 and frec["status"].max() == R.OK
        if sep == 1:
            corners = {(int(r["x"]), int(r["y"])) for r in live(rec, frec)[0]}
            assert any(x <= 1 and y <= 1 for x, y in corners) and any(x >= w - 2 and y >= h - 2 for x, y in corners)
            assert all(r["flags"] & R.EDGE for r in live(rec, frec)[0] if r["x"] in (0, w - 1) or r["y"] in (0, h - 1))


def test_radius_one_rmax_and_extended(gpu_ctx):
    h, w = 72, 150
    img = np.zeros((3, h, w), np.float32)
    # rad 1: a pixel of 1 ringed, two pixels out, by -0.5: S is negative all around it
    img[0, 20:25, 20:25] = -0.5
    img[0, 21:24, 21:24] = 0.0
    img[0, 22, 22] = 1.0
    # flat squares of 1 with a centre of 2: S = 10 on the 3 x 3 about the centre, its first pixel the candidate, one px up and
    # left of the centre; the square of half-width 29 ends at its ring 31, the one of half-width 30 reaches ring 32
    for f, (cx, hw) in ((1, (40, 29)), (2, (40, 30)), (2, (110, 29))):
        img[f, 35 - hw:35 + hw + 1, cx - hw:cx + hw + 1] = 1.0
        img[f, 35, cx] = 2.0
    rec, frec = check(gpu_ctx, img, max_obj=16)
    l0, l1, l2 = live(rec, frec)
    assert [int(r["rad"]) for r in l0 if (r["x"], r["y"]) == (22, 22)] == [1]
    # (each plateau's leading pixel, where S first reaches 9, is a candidate too: extended)
    peaks = lambda recs: [(int(r["x"]), int(r["y"]), int(r["rad"]), int(r["flags"])) for r in recs if r["s_peak"] == 10.0]  # noqa: E731
    assert peaks(l1) == [(39, 34, 32, 0)] and len(l1) == 2 and l1[0]["flags"] == R.EXTENDED
    assert peaks(l2) == [(39, 34, 0, R.EXTENDED), (109, 34, 32, 0)] and len(l2) == 4
    # a smaller r_max makes every one of them extended, and the peak pixel alone is measured
    rec, frec = check(gpu_ctx, img[1:], r_max=8, max_obj=16)
    for r in np.concatenate(live(rec, frec)):
        assert r["flags"] == R.EXTENDED and r["flux"] == 1.0 and (r["xc"], r["yc"]) == (r["x"], r["y"])
    check(gpu_ctx, img, r_max=1, max_obj=16)
    check(gpu_ctx, img, edge_frac=1.0, k_edge=40.0, max_obj=16)
    check(gpu_ctx, img, edge_frac=0.0, k_edge=0.01, max_obj=16)


def test_ties(gpu_ctx):
    h, w = 48, 100
    img = np.zeros((3, h, w), np.float32)
    img[0, 10:35, 50:75] = 1.0                                # a flat 25 x 25 plateau across the seam at x = 64 and y = 16, 32
    for f, gap in ((1, 3), (2, 4)):                           # two equal peaks sep and sep + 1 apart, across the seam
        img[f, 15, 62], img[f, 15, 62 + gap] = 4.0, 4.0
        img[f, 40, 20], img[f, 40 + gap, 20] = 4.0, 4.0
    rec, frec = check(gpu_ctx, img, sep=3, max_obj=32)
    assert frec["n_found"][0] >= 1 and frec["n_found"][2] >= frec["n_found"][1]
    for sep in (1, 2, 4, 8):
        check(gpu_ctx, img, sep=sep, max_obj=32)


def test_cap_long_row_and_empty_frame(gpu_ctx):
    h, w = 12, 230
    img = np.zeros((2, h, w), np.float32)
    for i in range(72):                                       # 72 candidates on row 4: a pixel every three columns, values rising
        img[0, 5, 1 + 3 * i] = np.float32(1.0 + 0.125 * i)
    img[0, 9, 100] = 50.0
    rec, frec = check(gpu_ctx, img, sep=1, r_max=4, max_obj=128)
    assert frec["n_found"].tolist() == [73, 0] and frec["n_out"].tolist() == [73, 0]
    assert np.count_nonzero(live(rec, frec)[0]["y"] == 4) == 72
    for cap in (1, 64, 65, 72, 73):
        rec2, frec2 = check(gpu_ctx, img, sep=1, r_max=4, max_obj=cap)
        assert frec2["status"].tolist() == [R.TRUNCATED if cap < 73 else R.OK, R.OK] and frec2["n_out"].tolist() == [cap, 0]
        assert rec2[0].tobytes() == rec[0, :cap].tobytes()


def test_tall_frame_sigmas_and_bad_pixels(gpu_ctx):
    h, w = 300, 40
    rng = np.random.default_rng(300)
    frames = rng.normal(0, 0.025, (4, h, w)).astype(np.float32)
    for f in range(4):
        for k, y in enumerate((0, 1, 127, 128, 255, 256, 257, 298, 299)):
            blob(frames[f], y, (7 * k + 3 * f) % w, 1.0 + k)
        frames[f] *= np.float32(1 + f)
    frames[1, 128, 8] = np.inf                                # inside sources
    frames[1, 127, 10] = np.nan
    frames[2, 256, 37] = -np.inf
    sig = np.array([0.025, 0.05, 0.075, 0.1], np.float32)
    rec, frec = check(gpu_ctx, frames, sig, max_obj=64)
    assert frec["n_found"].min() >= 5
    rec1, frec1 = check(gpu_ctx, frames, None, max_obj=64)
    assert frec1["n_found"][3] > frec["n_found"][3]           # (the sigma counts)
