"""The detection rounds on the oracle (tests/rounds_ref.py), without a GPU: frames with 0 .. 3 streaks (tests/rounds_cases.py).
Measured outcomes, asserted below so that they stay true: with half = 16 every streak comes back, strongest first, and the
round after the last streak finds nothing (found = 0); with the default half = 10 the band is narrower than the dilated streak,
the
rounds after the first return the first streak's wing (dup_of = 0) up to the cap, or stop at a rejected line set."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_cases as RC  # noqa: E402
import rounds_ref as RR  # noqa: E402

from lfd_amd import _native  # noqa: E402
from lfd_amd.detecttrails import default_params  # noqa: E402

SUBSETS = ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))


@pytest.fixture(scope="module")
def world(oracle):
    assert hasattr(_native.lib(), "lfdmi_detect_rounds")
    pb, pd, prs = default_params()
    rs = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    return oracle, pb, pd, rs


def run(world, field, which, **kw):
    O, pb, pd, rs = world
    img, cat = RC.frame(field, which)
    return RR.rounds(img, RR.oracle_detect(O, pb, pd, cat, rs), **kw)


@pytest.mark.parametrize("field", [0, 1])
def test_each_streak_is_found_alone(world, field):
    for s in range(3):
        recs, nf, dups = run(world, field, (s,), max_trails=1)
        assert nf == 1 and RC.same_cell(recs[0], RC.STREAKS[s], RC.SHAPE[0]), (s, recs[0])


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("which", SUBSETS, ids=lambda w: "streaks" + "".join(map(str, w)) if w else "empty")
def test_every_streak_comes_back_in_some_round(world, field, which):
    recs, nf, dups = run(world, field, which, max_trails=5, half=RC.HALF)
    print(which, nf, dups.tolist(), [(int(r["found"]), float(r["rho"]), float(r["theta"])) for r in recs])
    for s in which:
        assert any(RC.same_cell(recs[k], RC.STREAKS[s], RC.SHAPE[0]) for k in range(nf)), (s, nf, recs)
    # measured: nothing but the streaks is found, strongest first, no wing at this half; the round after the last finds nothing
    assert nf == len(which) and dups.tolist() == [-1] * 5
    assert [next(s for s in which if RC.same_cell(recs[k], RC.STREAKS[s], RC.SHAPE[0])) for k in range(nf)] == sorted(which)
    assert int(recs[nf]["status"]) == 0 and int(recs[nf]["found"]) == 0
    assert recs[nf + 1:].tobytes() == bytes((4 - nf) * RR.RESULT_DTYPE.itemsize)


def test_an_empty_frame_finds_nothing(world):
    for field in (0, 1, 2):
        recs, nf, dups = run(world, field, ())
        assert nf == 0 and dups.tolist() == [-1] * 4


def test_the_default_half_leaves_the_wings(world):
    """measured: at half = 10 the band is narrower than the dilated streak 0.  Beside the dim streak 2 every later round finds
    streak 0's wing again and says so (dup_of = 0); beside streak 1 the wing spoils round 1's line sets (rejected_by_theta)
    and the frame stops with one trail"""
    recs, nf, dups = run(world, 0, (0, 2), max_trails=4)
    print(nf, dups.tolist(), recs)
    assert nf == 4 and dups.tolist() == [-1, 0, 0, 0]
    assert all(RC.same_cell(recs[k], RC.STREAKS[0], RC.SHAPE[0]) for k in range(4))
    recs, nf, dups = run(world, 0, (0, 1), max_trails=4)
    print(nf, dups.tolist(), recs)
    assert nf == 1 and int(recs[1]["found"]) == 0 and int(recs[1]["rejected_by_theta"]) == 1


@pytest.mark.parametrize("name", list(RC.BANDS))
def test_the_hand_placed_streaks_are_found(world, name):
    """what tests/test_gpu_rounds_edges.py relies on: round 0 finds the hand-placed streak at the stated angle, so a later
    round gathers with a band that is near-vertical, horizontal, through a corner, of zero width or wider than a tile"""
    import math
    O, pb, pd, rs = world
    img, cat, half = RC.band_frame(name)
    recs, nf, dups = RR.rounds(img, RR.oracle_detect(O, pb, pd, cat, rs), 3, half)
    print(name, nf, dups.tolist(), recs)
    assert nf >= 1 and round(math.degrees(float(recs[0]["theta"]))) == RC.BANDS[name][2]
    r = recs[0]
    if name == "horizontal":
        assert abs(int(r["y1"]) - int(r["y2"])) <= 1           # one row over the 2560 px between the end points
    if "corner" in name:                                       # the band covers a corner pixel of the frame
        h, w = RC.SHAPE
        m = RR.band(r, half, h, w)
        assert m[0, 0] or m[0, w - 1] or m[h - 1, 0] or m[h - 1, w - 1]
