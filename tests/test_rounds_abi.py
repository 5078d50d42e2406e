"""lfdmi_rounds_params as _native sees it: size, offsets, defaults, ranges."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_ref as RR  # noqa: E402

from lfd_amd import _native, rounds  # noqa: E402


def test_the_layouts_agree():
    S = _native.RoundsParamsStruct
    assert C.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("max_trails", 0), ("pad", 4), ("half", 8), ("dup_dist", 16)]
    assert C.sizeof(_native.Result) == _native.RESULT_DTYPE.itemsize == RR.RESULT_DTYPE.itemsize == 48
    assert RR.RESULT_DTYPE == _native.RESULT_DTYPE
    assert _native.ROUNDS_MAX_TRAILS == RR.MAX_TRAILS == rounds.MAX_TRAILS == 8


def test_the_defaults():
    p = _native.make_rounds_params()
    assert (p.max_trails, p.pad, p.half, p.dup_dist) == (4, 0, 10.0, 20.0)
    assert rounds.default_params() == RR.DEFAULTS
    p = _native.make_rounds_params(max_trails=2, half=3.5)
    assert (p.max_trails, p.half, p.dup_dist) == (2, 3.5, 20.0)
    with pytest.raises(TypeError) as e:
        _native.make_rounds_params(no_such_field=1)
    assert str(e.value) == "unknown rounds parameter 'no_such_field'"
    with pytest.raises(TypeError):
        rounds.as_params(width=3)
    assert rounds.as_params({"half": 4.0}, max_trails=2) == {"half": 4.0, "max_trails": 2}


def test_segments_and_rows(tmp_path):
    import numpy as np
    rec = np.zeros((2, 3), _native.RESULT_DTYPE)
    rec[0, 0] = (0, 1, 5.0, 1.5, -10, 20, 30, 40, 0, 0, 0, 0)
    rec[0, 1] = (0, 2, 6.0, 0.5, -11, 21, 31, 41, 0, 0, 0, 0)
    n_found, dup = np.array([2, 0], np.int32), np.array([[-1, 0, -1], [-1, -1, -1]], np.int32)
    segs, where = rounds.segments(rec, n_found)
    assert where == [(0, 0), (0, 1)] and segs.dtype == _native.MASK_SEGMENT_DTYPE
    assert segs["x1"].tolist() == [-10.0, -11.0] and segs["y2"].tolist() == [40.0, 41.0] and segs["frame"].tolist() == [0, 0]
    assert rounds.segments(rec, n_found, dup, skip_dups=True)[1] == [(0, 0)]
    path = tmp_path / "trails.txt"
    with open(path, "w") as f:
        for i, k in where:
            f.write(rounds.format_row((94, 1, "r", 100 + i), k, rec[i, k], dup[i, k]) + "\n")
    rows = rounds.read_trails(path)
    assert [r["round"] for r in rows] == [0, 1] and rows[1]["dup_of"] == 0 and rows[1]["rho"] == 6.0 and rows[0]["x1"] == -10
    assert rows[0]["filter"] == "r" and tuple(rows[0]) == rounds.TRAIL_COLUMNS
