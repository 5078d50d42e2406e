"""The restatement of the frame previews (tests/preview_ref.py) against answers worked by hand (tests/preview_cases.py), and
the pieces of it one at a time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_cases as P  # noqa: E402
import preview_ref as R  # noqa: E402


@pytest.mark.parametrize("name", P.NAMES)
def test_hand_worked(name):
    c = P.CASES[name]
    out, cells, rec = R.frame_previews(c.frames, P.TEST_LUT, **c.kwargs())
    P.check(name, out, cells, rec)


def test_the_cases_hold_what_they_are_named_for():
    assert set(P.NAMES) >= {"truncating_division", "partial_last_row_and_column", "some_and_all_pixels_not_finite",
                            "clamp_and_infinities", "ranks_at_the_ends", "one_cell", "flat_empty_ordinary", "both_ends_of_the_table",
                            "tie_on_the_boundary"}
    assert P.TEST_LUT[0] != 0 and len({int(P.TEST_LUT[k]) for k in (0, 1023, 2047, 3071, 4095)}) == 5


def test_fixed_rounds_to_even_and_clamps():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5], np.float64) * 2.0 ** -30
    valid, q = R.fixed(v.astype(np.float32))
    assert valid.all() and q.tolist() == [0, 2, 2, 0, -2]
    valid, q = R.fixed(np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 0.0, -0.0], np.float32))
    assert valid.tolist() == [False, False, False, True, True, True, True]
    assert q.tolist() == [0, 0, 0, 2 ** 54, -2 ** 54, 0, 0]
    assert R.given_fixed(1e300) == 2 ** 54 and R.given_fixed(-1e300) == -2 ** 54 and R.given_fixed(2.5 * 2.0 ** -30) == 2


def test_truncating_division():
    q = np.array([-3, 3, -4, 0, -1], np.int64)
    assert R.trunc_div(q, np.array([2, 2, 2, 5, 256])).tolist() == [-1, 1, -2, 0, 0]


def test_the_largest_cell_stays_inside_int64():
    f = np.full((16, 16), 1e30, np.float32)
    assert R.cells(f, 16).tolist() == [[2 ** 54]]
    assert R.cells(-f, 16).tolist() == [[-2 ** 54]]


def test_levels_reach_both_ends_with_the_widest_limits():
    m = np.array([-2 ** 54, 0, 2 ** 54, R.EMPTY_CELL], np.int64)
    assert R.levels(m, -2 ** 54, 2 ** 54).tolist() == [0, 2047, 4095, 0]


def test_big_endian_frames_are_the_same_frames():
    rng = np.random.default_rng(5)
    f = rng.normal(0, 0.025, (2, 9, 11)).astype(np.float32)
    a = R.frame_previews(f, P.TEST_LUT, bin=2)
    b = R.frame_previews(f.astype(">f4"), P.TEST_LUT, bin=2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
