"""The restatement of the short-streak search (tests/streak_ref.py) against answers worked by hand (tests/streak_cases.py):
the segment's path, planted segments in both orientations, the 45-degree tie, the half-valid rule at its edge, frames without a
candidate, an orientation too narrow for a segment, and the peel footprint cell by cell (include/lfdmi.h: short-streak search)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_cases as SC  # noqa: E402
import streak_ref as S  # noqa: E402

P8 = {"bin": 1, "length": 8, "threshold": 8.0}


def same(got, want):
    for k in S.FIELDS:
        a, b = got[k], want[k]
        if isinstance(b, (float, np.floating)):
            assert np.asarray(a).tobytes() == np.asarray(b, np.asarray(a).dtype).tobytes(), (k, a, b)
        else:
            assert int(a) == int(b), (k, a, b)


def test_off_for_every_slope_of_length_8():
    for s in range(-7, 8):
        got = [S.off(i, s, 8) for i in range(8)]
        want = [v if s >= 0 else -v for v in SC.OFF8[abs(s)]]
        assert got == want, s
        assert got[0] == 0 and got[-1] == s
    for L in (16, 32, 64):                                            # the ends, and one step at a time, at every length
        for s in range(-(L - 1), L):
            o = [S.off(i, s, L) for i in range(L)]
            assert o[0] == 0 and o[-1] == s and all(abs(b - a) <= 1 for a, b in zip(o, o[1:]))


@pytest.mark.parametrize("q", [0, 1])
def test_planted_segment_comes_back(q):
    f, key = SC.planted(q)
    rec = S.search(f, SC.SIGMA, **P8)
    same(rec, SC.expected(key))
    assert rec["sum"] == np.float32(0.5) and rec["n_pix"] == 8 and rec["found"] == 1      # 8 / 16 at sigma 1/64: snr 11.3
    G, M = S.prepare(f, 1, 0.125)
    assert G.max() == SC.G_AMP and G.min() == SC.G_BG and (M == 1).all()


def test_planted_segment_in_pixels():
    """q = 0, s = 3, r0 = 2, c0 = 1 at bin 1: from (1, 2) to (8, 5) in (x, y)"""
    rec = S.search(SC.planted(0)[0], SC.SIGMA, **P8)
    assert (rec["x1"], rec["y1"], rec["x2"], rec["y2"]) == (1.0, 2.0, 8.0, 5.0)
    rec = S.search(SC.planted(1)[0], SC.SIGMA, **P8)                  # q = 1: (r, c) -> (x, y): (9, 3) to (7, 10)
    assert (rec["x1"], rec["y1"], rec["x2"], rec["y2"]) == (9.0, 3.0, 7.0, 10.0)
    x1, y1, x2, y2, _, _ = S.line_of(0, 3, 2, 1, 8, 4)                # bin 4: cell centres b i + 1.5
    assert (x1, y1, x2, y2) == (5.5, 9.5, 33.5, 21.5)


def test_the_diagonal_tie_goes_to_q0():
    f, key = SC.diagonal()
    rec = S.search(f, SC.SIGMA, **P8)
    same(rec, SC.expected(key))
    G, M = S.prepare(f, 1, 0.125)
    for q in (0, 1):                                                  # the very same sums in both orientations
        sums, r_lo = S.segment_sums(S.orient(G, q), 7, 8)
        assert r_lo == 0 and sums[2, 2] == 8 * SC.G_AMP


def test_half_valid_rule_at_its_edge():
    rec = S.search(SC.half_valid(4), SC.SIGMA, **P8)
    same(rec, SC.expected((0, 0, 0, 0), n_amp=4))
    assert 2 * rec["n_pix"] == 8
    rec = S.search(SC.half_valid(3), SC.SIGMA, **P8)
    same(rec, S.none_record())
    assert rec["status"] == S.NONE and rec["snr"] == 0 and rec["found"] == 0


def test_blotted_frame_has_no_streak():
    recs, n = S.rounds(SC.blotted(), SC.SIGMA, **dict(P8, max_streaks=3))
    same(recs[0], S.none_record())
    assert n == 0 and all(r["status"] == 0 and r["snr"] == 0 for r in recs[1:])


def test_narrow_frame_has_only_q1():
    f, key = SC.tall()
    rec = S.search(f, SC.SIGMA, **P8)
    same(rec, SC.expected(key))
    assert rec["q"] == 1
    G, _ = S.prepare(f, 1, 0.125)
    assert S.segment_sums(S.orient(G, 0), 0, 8)[0] is None


def test_peel_footprint_cell_by_cell():
    rec = {"q": 0, "s": 3, "r0": 2, "c0": 1}
    centre = {0: 2, 1: 2, 2: 2, 3: 3, 4: 3, 5: 4, 6: 4, 7: 5, 8: 5, 9: 5}    # column -> row: off = 0 0 1 1 2 2 3 3, ends clamped
    want = np.zeros((12, 12), bool)
    for c, r in centre.items():
        for d in (-1, 0, 1):
            want[r + d, c] = True
    got = S.peel_mask((12, 12), rec, 8, 1)
    assert np.array_equal(got, want) and got.sum() == 30
    assert np.array_equal(S.peel_mask((12, 12), dict(rec, q=1), 8, 1), want.T)
    line = np.zeros((12, 12), bool)                                   # hw = 0: the segment's own cells
    for i in range(8):
        line[2 + SC.OFF8[3][i], 1 + i] = True
    assert np.array_equal(S.peel_mask((12, 12), rec, 8, 0), line)
    edge = S.peel_mask((12, 12), {"q": 0, "s": -3, "r0": 3, "c0": 4}, 8, 2)      # clipped by the array, never wrapped
    assert edge[:, :2].sum() == 0 and edge[0, 11] and edge[2, 11] and not edge[3, 11]


def test_rounds_peel_and_lay_out():
    f, key = SC.planted(0)
    put = SC.put(f.copy(), [(10, c) for c in range(2, 10)], np.float32(3.0 / 64))     # a second, fainter segment on row 10
    recs, n = S.rounds(put, SC.SIGMA, **dict(P8, max_streaks=4, peel_halfwidth=1, threshold=8.0))
    assert n == 2 and (recs[0]["q"], recs[0]["s"], recs[0]["r0"], recs[0]["c0"]) == key
    assert (recs[1]["q"], recs[1]["s"], recs[1]["r0"], recs[1]["c0"]) == (0, 0, 10, 2) and recs[1]["found"] == 1
    assert recs[2]["status"] == S.OK and recs[2]["found"] == 0 and recs[3]["status"] == 0 and recs[3]["n_pix"] == 0
    same(S.rounds(put, SC.SIGMA, **dict(P8, max_streaks=1, peel_halfwidth=1))[0][0], recs[0])
    same(S.search(put, SC.SIGMA, **P8), recs[0])


def test_range_rule():
    assert S.in_range(0.125, 2, 32) and S.in_range(0.125, 4, 64) and not S.in_range(8.0, 4, 64)
    assert S.in_range(2047.0 / 64, 1, 64) and not S.in_range(32.0, 1, 64)          # 2^25 * 64 = 2^31
    with pytest.raises(ValueError):
        S.rounds(SC.blotted(), clip=32.0, bin=1, length=64)
