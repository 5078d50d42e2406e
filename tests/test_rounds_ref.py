"""The detection rounds' definition (include/lfdmi.h: detection rounds) as tests/rounds_ref.py restates it, on hand-made cases
with scripted detectors: the dup_of arithmetic on worked end points, the stop rules, the zero-filled tails, and which pixels a
round's frame has lost.  Needs the library only for the symbol that marks the feature."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_ref as RR  # noqa: E402

from lfd_amd import _native  # noqa: E402


def test_the_library_has_the_call():
    assert "lfdmi_detect_rounds" in _native.SYMBOLS and hasattr(_native.lib(), "lfdmi_detect_rounds")


def line(x1, y1, x2, y2, found=1, status=0):
    return RR.record(status=status, found=found, x1=x1, y1=y1, x2=x2, y2=y2)


def test_dup_of_on_worked_end_points():
    # record 0: the horizontal line y = 100 from x = -1000 to 1000; nrm = (0, 1), u = y - 100
    r0 = line(-1000, 100, 1000, 100)
    assert RR.dup_of([r0, line(-1000, 120, 1000, 80)], 1, 20.0) == 0          # |u| = 20 at either end: on the bound
    assert RR.dup_of([r0, line(-1000, 121, 1000, 80)], 1, 20.0) == -1         # one end at 21
    assert RR.dup_of([r0, line(-1000, 100, 1000, 100)], 1, 0.0) == 0          # the same line, dup_dist 0
    # a 3-4-5 line: (0, 0) - (800, 600), nrm = (-0.6, 0.8); the point (50, 0) has u = -30, (0, 25) has u = 20
    r0 = line(0, 0, 800, 600)
    assert RR.dup_of([r0, line(0, 25, 800, 625)], 1, 20.0) == 0
    assert RR.dup_of([r0, line(50, 0, 850, 600)], 1, 29.0) == -1
    assert RR.dup_of([r0, line(50, 0, 850, 600)], 1, 30.0) == 0
    # the smallest j wins; a record that is not found, and record 0, have none; a segment of length 0 matches nothing
    a, b = line(-1000, 100, 1000, 100), line(-1000, 110, 1000, 110)
    assert RR.dup_of([a, b, line(-1000, 105, 1000, 105)], 2, 20.0) == 0
    assert RR.dup_of([line(-1000, 300, 1000, 300), b, line(-1000, 105, 1000, 105)], 2, 20.0) == 1
    assert RR.dup_of([a, line(-1000, 100, 1000, 100, found=0)], 1, 20.0) == -1
    assert RR.dup_of([a, line(-1000, 100, 1000, 100, status=-5)], 1, 20.0) == -1
    assert RR.dup_of([a], 0, 20.0) == -1
    assert RR.dup_of([line(5, 5, 5, 5), line(5, 5, 5, 5)], 1, 20.0) == -1


def scripted(recs):
    seen = []

    def detect(frame, k):
        seen.append(frame.copy())
        return recs[k]
    return detect, seen


def test_the_stop_rules_and_the_zero_filled_tail():
    frame = np.ones((40, 60), np.float32)
    nothing = RR.record(n_lines_equ=7)                                        # found 0, kept as returned
    a, b = line(-1000, 10, 1000, 10), line(-1000, 30, 1000, 30)
    # nothing in round 0
    recs, nf, dups = RR.rounds(frame, scripted([nothing])[0], 4)
    assert nf == 0 and int(recs[0]["n_lines_equ"]) == 7 and recs[1:].tobytes() == bytes(3 * RR.RESULT_DTYPE.itemsize)
    assert dups.tolist() == [-1, -1, -1, -1]
    # two found, then nothing: the record at n_found is the round that found nothing, the one after it is zero
    det, seen = scripted([a, b, nothing])
    recs, nf, dups = RR.rounds(frame, det, 4)
    assert nf == 2 and len(seen) == 3 and int(recs[2]["n_lines_equ"]) == 7 and recs[3].tobytes() == bytes(RR.RESULT_DTYPE.itemsize)
    # a failed round stops the frame like an empty one
    recs, nf, dups = RR.rounds(frame, scripted([a, RR.record(status=-6, found=1)])[0], 4)
    assert nf == 1 and int(recs[1]["status"]) == -6 and dups.tolist() == [-1, -1, -1, -1]
    # the cap: max_trails rounds and no more, max_trails = 1 is the plain call
    det, seen = scripted([a, b, a, b])
    recs, nf, dups = RR.rounds(frame, det, 2)
    assert nf == 2 and len(seen) == 2 and len(recs) == 2
    det, seen = scripted([a])
    recs, nf, dups = RR.rounds(frame, det, 1)
    assert nf == 1 and len(seen) == 1 and seen[0] is not frame and np.array_equal(seen[0], frame)


def test_a_round_sees_the_bands_of_all_lines_so_far_and_the_frame_stays():
    H, W = 40, 60
    frame = np.full((H, W), 3.0, np.float32)
    keep = frame.copy()
    a, b = line(-1000, 10, 1000, 10), line(20, -1000, 20, 1000)               # y = 10 and x = 20
    det, seen = scripted([a, b, RR.record()])
    RR.rounds(frame, det, 4, half=2.0)
    assert np.array_equal(frame, keep)
    rows = slice(H - 1 - 12, H - 1 - 8 + 1)                                   # flipped rows 8 .. 12
    want1 = keep.copy()
    want1[rows] = 0
    want2 = want1.copy()
    want2[:, 18:23] = 0
    assert np.array_equal(seen[0], keep) and np.array_equal(seen[1], want1) and np.array_equal(seen[2], want2)
    assert not np.signbit(seen[2][rows]).any()                                # +0
