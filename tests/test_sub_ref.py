"""The restatement of the trail subtraction (tests/sub_ref.py) against answers worked by hand, on frames of 8 x 40 or smaller.

The frame-based cases use a horizontal segment from (0, 3) to (39, 3) of the flipped frame with half 3, step 1, wing 1 and
sec_len 4: t = x and u = y - 3, so K = 3, n_off = 7, bin b holds the row u = b - 3, the wing bins are b = 0, 1, 5, 6, the core
bins b = 2, 3, 4, there are 10 sections and every cell holds the 4 pixels x = 4j .. 4j + 3 of its row.  Every value is a small
dyadic fraction, so every step is exact and the expected numbers can be written down."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sub_ref as UR  # noqa: E402

H, W = 8, 40
SEG = UR.segment(0, 0.0, 3.0, 39.0, 3.0, half=3.0)
KW = dict(sec_len=4.0, step=1.0, wing=1.0, min_n=1, min_wing=1, max_sections=16)
WING = np.float32(2.0 ** -6)
Q = 1 << 30


def band_frame(core):
    """rows of the flipped frame y = 0 .. 6 are the band (u = -3 .. 3); wing rows hold 2^-6, core rows core[x]; row 7 is outside"""
    f = np.full((H, W), WING, np.float32)
    for y in (2, 3, 4):
        f[H - 1 - y] = core
    f[0] = np.float32(0.5)                                              # flipped row 7: outside the band
    return f


def geo(seg=SEG, **kw):
    p = dict(UR.DEFAULTS, **{k: v for k, v in kw.items() if k != "max_sections"})
    status, g = UR.SR.geometry(seg, p, 16, 1 << 20)
    assert status == UR.OK
    return g, p


def cells_of(n, q):
    """int64 [n_sec, n_off, 3] cells from arrays n and q (n_geom = n)"""
    n, q = np.asarray(n, np.int64), np.asarray(q, np.int64)
    return np.stack([n, n, q], axis=-1)


def test_a_constant_band_gives_that_constant_minus_the_wing_mean():
    f = band_frame(np.full(W, 2.0 ** -4, np.float32))
    clean, rec, tab = UR.subtract_trails(f, [SEG], smooth=2, min_sec=1, **KW)
    r = rec[0]
    assert (r["status"], r["n_sec"], r["n_off"], r["K"], r["n_usable"], r["n_model"]) == (UR.OK, 10, 7, 3, 10, 30)
    m = tab[0][:70].reshape(10, 7)
    assert (m[:, [0, 1, 5, 6]] == 0).all() and (m[:, 2:5] == np.float32(2.0 ** -4 - 2.0 ** -6)).all()
    assert r["n_pix"] == 120 and r["q_removed"] == 120 * (Q // 16 - Q // 64) and r["removed"] == 120 * 0.046875
    assert r["peak"] == 0.046875 and r["peak_section"] == 0              # ties: the lowest j
    want = f.copy()
    want[H - 1 - 4:H - 1 - 1] = WING                                    # the core rows come down to the wings' level
    assert np.array_equal(clean.view(np.uint32), want.view(np.uint32))


def test_divisions_truncate_toward_zero():
    g, p = geo(smooth=0, min_sec=1, **KW)
    n = np.zeros((10, 7), np.int64)
    q = np.zeros((10, 7), np.int64)
    n[:, [0, 1, 5, 6]] = 1
    n[:, 2:5] = 2
    q[0, [0, 1, 5, 6]] = [-2, -2, -2, -1]                               # Q = -7, N = 4: B = -1 (floor would give -2)
    q[0, 2:5] = [-3, 3, -1]                                             # q / n = -1, 1, 0 (floor: -2, 1, -1)
    m, M, n_usable, has, X = UR.model(cells_of(n, q), g, p)
    assert X[0][2:5] == [-1 - -1, 1 - -1, 0 - -1] == [0, 2, 1] and n_usable == 10 and has[:, 2:5].all()
    assert M[0][2:5] == [0, 2, 1] and m[0, 3] == np.float32(2.0 ** -29)
    assert UR.tdiv(-7, 4) == -1 and UR.tdiv(7, 4) == 1 and UR.tdiv(-8, 4) == -2 and UR.tdiv(-1, 2) == 0


def column_cells(xs, n_sec=None):
    """cells of n_sec sections whose wing sums are zero (B = 0) and whose core bin b = 3 holds one pixel of q = xs[j] (None:
    no valid pixel, so the excess is absent)"""
    n_sec = len(xs) if n_sec is None else n_sec
    n = np.zeros((n_sec, 7), np.int64)
    q = np.zeros((n_sec, 7), np.int64)
    n[:, [0, 1, 5, 6]] = 1
    for j, x in enumerate(xs):
        if x is not None:
            n[j, 3], q[j, 3] = 1, x
    return cells_of(n, q)


def seg_of_sections(n_sec):
    return UR.segment(0, 0.0, 3.0, 4.0 * n_sec - 1.0, 3.0, half=3.0)


def test_the_even_count_median_and_min_sec():
    g, p = geo(seg_of_sections(4), smooth=2, min_sec=1, **KW)
    c = column_cells([10, -7, None, 4])
    m, M, _, has, X = UR.model(c, g, p)
    # j = 0: rows 0 .. 2 hold {10, -7}: -7 + (10 - -7) / 2 = -7 + 8 = 1 (17 / 2 truncates)
    # j = 1: rows 0 .. 3 hold {-7, 4, 10}: 4;  j = 2: the same;  j = 3: rows 1 .. 3 hold {-7, 4}: -7 + 11 / 2 = -2
    assert [M[j][3] for j in range(4)] == [1, 4, 4, -2] and has[:, 3].all()
    assert M[2][3] == 4 and X[2][3] is None                              # an absent section still gets its neighbours' model
    # min_sec at c and at c - 1
    for min_sec, want in ((2, [1, 4, 4, -2]), (3, [0, 4, 4, 0]), (4, [0, 0, 0, 0])):
        m, M, _, has, _ = UR.model(c, g, dict(p, min_sec=min_sec))
        assert [M[j][3] for j in range(4)] == want and has[:, 3].tolist() == [v != 0 for v in want], min_sec
    # a negative even-count median: {-10, -7}: -10 + 3 / 2 = -9
    m, M, _, _, _ = UR.model(column_cells([-10, -7]), geo(seg_of_sections(2), smooth=1, min_sec=2, **KW)[0], dict(p, smooth=1, min_sec=2))
    assert M[0][3] == M[1][3] == -9


def test_no_smoothing_one_section_and_fewer_sections_than_the_window():
    g, p = geo(seg_of_sections(4), smooth=0, min_sec=1, **KW)
    m, M, _, has, _ = UR.model(column_cells([10, -7, None, 4]), g, p)
    assert [M[j][3] for j in range(4)] == [10, -7, 0, 4] and has[:, 3].tolist() == [True, True, False, True]   # R = 0: the cell itself
    g1, p1 = geo(seg_of_sections(1), smooth=8, min_sec=1, **KW)
    assert g1[-3] == 1
    m, M, _, has, _ = UR.model(column_cells([6]), g1, p1)
    assert M[0][3] == 6 and m[0, 3] == np.float32(6 * 2.0 ** -30) and int(has.sum()) == 1   # (the other core bins hold no pixel: absent)
    g3, p3 = geo(seg_of_sections(3), smooth=8, min_sec=3, **KW)           # n_sec = 3 < R = 8: every window is the whole segment
    m, M, _, has, _ = UR.model(column_cells([5, 1, 9]), g3, p3)
    assert [M[j][3] for j in range(3)] == [5, 5, 5]


def test_interpolation_clamps_at_both_ends_and_below_the_first_bin():
    # a ramp along the trail: the core of section j holds 2^-6 + (j + 1) 2^-8, so with R = 0 the model is m_j = (j + 1) 2^-8
    core = (2.0 ** -6 + (np.arange(W) // 4 + 1) * 2.0 ** -8).astype(np.float32)
    f = band_frame(core)
    clean, rec, tab = UR.subtract_trails(f, [SEG], smooth=0, min_sec=1, **KW)
    m = tab[0][:70].reshape(10, 7)
    assert m[:, 3].tolist() == [(j + 1) * 2.0 ** -8 for j in range(10)] and rec[0]["peak_section"] == 9
    g, _ = geo(smooth=0, min_sec=1, **KW)
    geom, v = UR.value((H, W), g, m)
    row = v[H - 1 - 3]                                                  # u = 0: a = x / 4 - 0.5
    assert row[0] == row[1] == row[2] == np.float32(2.0 ** -8)           # a < 0, a = 0: no extrapolation below the first section
    assert row[4] == np.float32(1.5 * 2.0 ** -8) and row[6] == np.float32(2.0 ** -7)         # a = 0.5 and a = 1
    assert row[38] == row[39] == np.float32(10 * 2.0 ** -8)              # a = 9 and a = 9.25 > n_sec - 1: none above the last
    assert row[37] == np.float32(9.75 * 2.0 ** -8)
    assert np.array_equal(clean[H - 1 - 3], f[H - 1 - 3] - row) and not geom[0].any()
    # g < 0: a band of half 3.4 about y = 3.3 reaches the row u = -3.3, where g = -0.3; b0 = 0 and fb = 0, so the value is the
    # first bin's, which is a wing bin's 0, and the row is not written (an extrapolated fb = -0.3 would have written it)
    seg = UR.segment(0, 0.0, 3.3, 39.0, 3.3, half=3.4)
    clean, rec, tab = UR.subtract_trails(f, [seg], smooth=0, min_sec=1, **dict(KW, wing=0.5))
    assert rec[0]["status"] == UR.OK and rec[0]["K"] == 3 and rec[0]["n_pix"] > 0
    assert np.array_equal(clean[H - 1 - 0].view(np.uint32), f[H - 1 - 0].view(np.uint32))
    assert not np.array_equal(clean[H - 1 - 3], f[H - 1 - 3])


def test_zeros_and_nans_inside_the_band_keep_their_bits():
    f = band_frame(np.full(W, 2.0 ** -4, np.float32))
    bits = f.view(np.uint32)
    r = H - 1 - 3
    bits[r, 5], bits[r, 6], bits[r, 7], bits[r, 8] = 0x80000000, 0x00000000, 0x7FC12345, 0xFF800000   # -0, +0, a NaN, -inf
    before = f.copy()
    clean, rec, tab = UR.subtract_trails(f, [SEG], smooth=2, min_sec=1, **KW)
    assert np.array_equal(f.view(np.uint32), before.view(np.uint32))     # the input is never changed
    assert clean.view(np.uint32)[r, 5:9].tolist() == [0x80000000, 0x00000000, 0x7FC12345, 0xFF800000]
    assert rec[0]["n_pix"] == 116 and clean[r, 9] == WING and clean[r, 4] == WING


def test_crossing_segments_apply_in_index_order_and_the_order_shows():
    rng = np.random.default_rng(4)
    f = rng.normal(0.0, 0.025, (H, W)).astype(np.float32)
    a, b = UR.segment(0, 0.0, 1.0, 39.0, 6.0, half=2.5), UR.segment(0, 0.0, 6.0, 39.0, 1.0, half=2.5)
    kw = dict(KW, wing=0.75, smooth=1, min_sec=1)
    ab, rab, tab_ab = UR.subtract_trails(f, [a, b], **kw)
    ba, rba, tab_ba = UR.subtract_trails(f, [b, a], **kw)
    assert np.array_equal(tab_ab[0], tab_ba[1]) and np.array_equal(tab_ab[1], tab_ba[0])   # the models come from the frame as passed
    assert rab[0] == rba[1] and rab[1] == rba[0]
    assert (ab.view(np.uint32) != ba.view(np.uint32)).any()              # at least one bit: float32 subtraction in another order
    p = dict(UR.DEFAULTS, **{k: v for k, v in kw.items() if k != "max_sections"})
    va = UR.value((H, W), UR.SR.geometry(a, p, 16, 1 << 20)[1], tab_ab[0][:rab[0]["n_sec"] * rab[0]["n_off"]].reshape(rab[0]["n_sec"], -1))[1]
    vb = UR.value((H, W), UR.SR.geometry(b, p, 16, 1 << 20)[1], tab_ab[1][:rab[1]["n_sec"] * rab[1]["n_off"]].reshape(rab[1]["n_sec"], -1))[1]
    both = (va != 0) & (vb != 0)
    assert both.any() and np.array_equal(ab[both], (f[both] - va[both]) - vb[both])         # the ascending one


def test_apply_0_returns_the_same_record_and_leaves_the_frames_alone():
    f = band_frame(np.full(W, 2.0 ** -4, np.float32))
    clean1, rec1, tab1 = UR.subtract_trails(f, [SEG], smooth=2, min_sec=1, **KW)
    clean0, rec0, tab0 = UR.subtract_trails(f, [SEG], smooth=2, min_sec=1, apply=0, **KW)
    assert rec0.tobytes() == rec1.tobytes() and np.array_equal(tab0, tab1) and rec0[0]["n_pix"] == 120
    assert np.array_equal(clean0.view(np.uint32), f.view(np.uint32)) and (clean1 != f).any()
    with pytest.raises(AssertionError):
        UR.subtract_trails(f, [UR.segment(1, 0.0, 3.0, 39.0, 3.0, half=3.0)], **KW)         # a frame outside [0, n)
