"""The source finder on the CPU (include/lfdmi.h: source finder), restatement only (tests/stars_ref.py): what the defaults do on
``synth.make_frame`` frames of 372 x 512 -- which truth stars come back, what noise alone yields, where a streak's ridge
maxima end up -- a block worked out by hand, and the catalogue of step 8 through the oracle's remove_stars.

Measured with the defaults over seeds 0 .. 15 (25 stars per frame, sky sigma 0.025): of the truth stars whose pixel has S >= T,
84 - 100 % per frame come back as a non-extended source within 1 px (the misses are blends: a brighter neighbour inside the
window); 8 noise-only frames give 0 candidates each; the 12 frames with a streak have 36 - 79 candidates on the ridge, none of
them non-extended; the largest rad of a non-extended source is 23.  Each bound below is 1.5 times the worst case seen."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402

SHAPE = (372, 512)
SEEDS = range(16)
N_STAR = 25                         # make_frame's density on this shape
MAX_MISS = 1.5 * 4 / 25             # worst frame: 21 of 25
MAX_NOISE = 1.5 * 0                 # worst noise-only frame: no candidate
MAX_RIDGE_COMPACT = 1.5 * 0         # worst streak frame: no non-extended candidate on the ridge


@functools.lru_cache(maxsize=None)
def frame(k):
    from lfd_amd import synth
    img, cat, truth = synth.make_frame(k, shape=SHAPE)
    rec, frec = R.find_stars(img)
    return img, cat, truth, rec[:int(frec["n_out"])], frec


def test_truth_stars_come_back():
    T = np.float32(R.DEFAULTS["k_det"] * 3.0 * 0.025)
    for k in SEEDS:
        img, cat, truth, rec, frec = frame(k)
        assert frec["status"] == R.OK and frec["n_found"] == frec["n_out"]
        S = R.smooth(R.clean(img))
        compact = rec[(rec["flags"] & R.EXTENDED) == 0]
        seen = missed = 0
        for y, x in zip(cat["ROWC"][:N_STAR, 0], cat["COLC"][:N_STAR, 0]):
            iy, ix = int(np.floor(y)), int(np.floor(x))
            if not (0 <= iy < SHAPE[0] and 0 <= ix < SHAPE[1]) or S[iy, ix] < T:
                continue
            seen += 1
            d = np.hypot(compact["xc"].astype(np.float64) - x, compact["yc"].astype(np.float64) - y)
            missed += not (len(d) and d.min() <= 1.0)
        print(k, "truth above T", seen, "missed", missed)
        assert seen >= 20 and missed <= MAX_MISS * seen, (k, seen, missed)
        assert compact["rad"].min() >= 1 and compact["rad"].max() <= 1.5 * 23


def test_noise_alone_yields_nothing():
    rng = np.random.default_rng(5)
    for s in range(8):
        rec, frec = R.find_stars(rng.normal(0, 0.025, SHAPE).astype(np.float32))
        print("noise", s, int(frec["n_found"]))
        assert frec["n_found"] <= MAX_NOISE


def test_ridge_maxima_are_extended():
    kinds = set()
    for k in SEEDS:
        img, cat, truth, rec, frec = frame(k)
        if truth["streak"] == "none":
            continue
        kinds.add(truth["streak"])
        phi = np.deg2rad(truth["angle_deg"])
        d = (rec["x"] - truth["x0"]) * np.sin(phi) - (rec["y"] - truth["y0"]) * np.cos(phi)
        ridge = np.abs(d) <= 2.0
        compact = ridge & ((rec["flags"] & R.EXTENDED) == 0)
        print(k, truth["streak"], "ridge candidates", int(ridge.sum()), "non-extended", int(compact.sum()))
        assert ridge.sum() >= 10 and compact.sum() <= MAX_RIDGE_COMPACT, k
        assert np.all(rec["rad"][ridge] == 0)
    assert kinds == {"bright", "dim"}


def test_one_source_by_hand():
    """9 x 11 pixels, sigma 1/15 so that T = 1 and the floor of E is 0.6; one pixel of 8 at (x 4, y 3) and one of 2 beside it at
    x 5: S is 10 on (3 .. 5, 2 .. 4), 8 on column 3 and 2 on column 6 of those rows; the first of the three equal maxima in raster
    order is (4, 2) -- and the window sees its equals later in raster order only"""
    f = np.float32
    img = np.zeros((9, 11), f)
    img[3, 4], img[3, 5] = 8.0, 2.0
    sigma = f(1.0 / 15.0)
    rec, frec = R.find_stars(img, sigma, sep=1, r_max=4, max_obj=8)
    S = R.smooth(R.clean(img))
    assert S[2:5, 3:7].tolist() == [[8.0, 10.0, 10.0, 2.0]] * 3 and S.sum() == 90.0
    assert (int(frec["n_found"]), int(frec["n_out"]), int(frec["status"])) == (1, 1, R.OK)
    r = rec[0]
    # rings about (4, 2): r = 1 holds 10s, r = 2 holds S[4] = 10 (row 4), r = 3 is all zero (row 5, columns 1 and 7) < E = 0.6
    assert (r["x"], r["y"], r["rad"], r["s_peak"]) == (4, 2, 3, 10.0) and r["flags"] == R.EDGE       # (row 2 - 3 is off the frame)
    assert r["flux"] == 10.0 and r["xc"] == f(4 + 2.0 / 10.0) and r["yc"] == f(2 + 10.0 / 10.0)
    assert not rec[1:].view(np.uint8).any()
    # a cap of one source less: none here, but the record says how many there were
    two = img.copy()
    two[7, 9] = 8.0
    rec2, frec2 = R.find_stars(two, sigma, sep=1, r_max=4, max_obj=1)
    assert (int(frec2["n_found"]), int(frec2["n_out"]), int(frec2["status"])) == (2, 1, R.TRUNCATED) and rec2[0] == r
    # non-finite pixels count as zero
    bad = img.copy()
    bad[0, 0], bad[8, 10] = np.nan, np.inf
    assert R.find_stars(bad, sigma, sep=1, r_max=4, max_obj=8)[0].tobytes() == rec.tobytes()
    assert R.find_stars(img.astype(">f4"), sigma, sep=1, r_max=4, max_obj=8)[0].tobytes() == rec.tobytes()


def test_catalogue_through_remove_stars(oracle):
    """``lfd_amd.stars.to_catalog`` (step 8 on the host, equal to the restatement's) through the oracle's remove_stars: every
    non-extended source's square |d| <= rad is zero afterwards, and no extended candidate's peak is blotted by its own row.
    remove_stars slices img[x-d:x+d] as Python does: a start below zero counts from the far edge and the slice is empty, so a
    source closer than its half-width d to the top or left edge is NOT blotted, by either catalogue (include/lfdmi.h, step 8).
    Both sides are asserted: the squares of sources with x >= d and y >= d are zero, the others' pixels are untouched."""
    from lfd_amd import stars
    from lfd_amd.detecttrails import default_params
    prs = default_params()[2]
    rs = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    checked = untouched = 0
    for k in (4, 9):
        img, cat, truth, rec, frec = frame(k)
        cat = stars.to_catalog(rec[None], np.array([frec]), prs["pixscale"])
        want = R.to_catalog(rec[None], np.array([frec]), prs["pixscale"])
        assert all(np.array_equal(cat[key], want[key]) and cat[key].dtype == want[key].dtype for key in want)
        compact = rec[(rec["flags"] & R.EXTENDED) == 0]
        ext = rec[(rec["flags"] & R.EXTENDED) != 0]
        assert len(ext) >= 10 and len(compact) >= 10
        blot = img.copy()
        oracle.remove_stars(blot, R.frame_catalog(cat, 0), rs)
        for r in compact:
            d = int(np.ceil(np.float32(r["rad"] * prs["pixscale"])) / prs["pixscale"]) + 10
            assert r["rad"] + 10 <= d <= 42
            sq = (slice(max(r["y"] - r["rad"], 0), r["y"] + r["rad"] + 1), slice(max(r["x"] - r["rad"], 0), r["x"] + r["rad"] + 1))
            if r["x"] >= d and r["y"] >= d:
                assert not blot[sq].any(), (k, r)
                checked += 1
            else:
                alone = img.copy()
                one = {key: (v[:, (rec["x"] == r["x"]) & (rec["y"] == r["y"])] if key != "count" else np.array([1], np.int32)) for key, v in cat.items()}
                oracle.remove_stars(alone, R.frame_catalog(one, 0), rs)
                assert np.array_equal(alone.view(np.uint32), img.view(np.uint32)), (k, r)
                untouched += 1
        # the extended rows alone blot nothing
        only = {key: (v[:, (rec["flags"] & R.EXTENDED) != 0] if key != "count" else np.array([len(ext)], np.int32)) for key, v in cat.items()}
        same = img.copy()
        oracle.remove_stars(same, R.frame_catalog(only, 0), rs)
        assert np.array_equal(same.view(np.uint32), img.view(np.uint32))
    print("squares zeroed", checked, "sources near the low edges left untouched", untouched)
    assert checked >= 20 and untouched >= 2
