"""lfdmi_streak and lfdmi_streak_params as Python sees them, without a GPU: the structs' layout against the header and ctypes,
the library's defaults, the exported symbols, and the rules ``streaks.as_params`` applies -- every LFDMI_ERR_ARG of the call's
parameters, the int32 range rule among them (tests/test_gpu_streak.py holds the library to the same values on a device: its
check sits behind the context)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_ref as S  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402

REFUSED = ({"bin": 0}, {"bin": 3}, {"bin": 8}, {"length": 4}, {"length": 12}, {"length": 128}, {"max_streaks": 0}, {"max_streaks": 9},
           {"peel_halfwidth": -1}, {"clip": 0.0}, {"clip": -0.125}, {"clip": float("nan")}, {"clip": float("inf")},
           {"threshold": 0.0}, {"threshold": -1.0}, {"threshold": float("nan")}, {"threshold": float("inf")},
           {"clip": 32.0, "bin": 1, "length": 64}, {"clip": 8.0, "bin": 4, "length": 64}, {"clip": 1e30})
TAKEN = ({}, {"bin": 1}, {"bin": 4}, {"length": 8}, {"length": 64}, {"max_streaks": 1}, {"max_streaks": 8}, {"peel_halfwidth": 0},
         {"clip": 2047.0 / 64, "bin": 1, "length": 64}, {"clip": 1.9, "bin": 4, "length": 64}, {"threshold": 1e-3})


def header_text():
    with open(os.path.join(ROOT, "include", "lfdmi.h")) as f:
        return f.read()


def test_struct_layout():
    from lfd_amd import _native, streaks
    assert C.sizeof(_native.Streak) == _native.STREAK_DTYPE.itemsize == 88
    names = [k for k, _ in _native.Streak._fields_]
    assert names == list(_native.STREAK_DTYPE.names) == header_struct("lfdmi_streak")
    assert names == ["status", "found", "q", "s", "r0", "c0", "n_pix", "sum", "snr", "pad", "x1", "y1", "x2", "y2", "rho", "theta"]
    for k in names:
        assert getattr(_native.Streak, k).offset == _native.STREAK_DTYPE.fields[k][1], k
        assert getattr(_native.Streak, k).size == _native.STREAK_DTYPE.fields[k][0].itemsize, k
    assert [getattr(_native.Streak, k).offset for k in ("sum", "snr", "pad", "x1", "theta")] == [28, 32, 36, 40, 80]
    assert [k for k, _ in _native.StreakParamsStruct._fields_] == header_struct("lfdmi_streak_params") == list(streaks.PARAM_NAMES)
    assert C.sizeof(_native.StreakParamsStruct) == 24
    assert [getattr(_native.StreakParamsStruct, k).offset for k in streaks.PARAM_NAMES] == [0, 4, 8, 12, 16, 20]
    assert streaks.STREAK_DTYPE is _native.STREAK_DTYPE


def test_symbols_and_constants():
    from lfd_amd import _native, streaks
    lib = _native.lib()
    text = header_text()
    for name in ("lfdmi_default_streak_params", "lfdmi_streak_search", "lfdmi_streak_tile"):
        assert name in _native.SYMBOLS and getattr(lib, name) is not None and re.search(r"\b%s\(" % name, text), name
    m = re.search(r"int lfdmi_streak_search\(([^;]*)\);", text)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["ctx", "frames", "dtype", "n", "h", "w", "loc", "sigma", "p", "out",
                                                                          "n_streaks"]
    assert len(lib.lfdmi_streak_search.argtypes) == 11
    assert "#define LFDMI_STREAK_MAX_STREAKS 8\n" in text and "enum { LFDMI_STREAK_OK = 0, LFDMI_STREAK_NONE = 1 };" in text
    assert (_native.STREAK_OK, _native.STREAK_NONE, _native.STREAK_MAX_STREAKS) == (0, 1, 8) == (S.OK, S.NONE, streaks.MAX_STREAKS)
    assert "#define LFDMI_VERSION 300\n" in text and lib.lfdmi_version() == 300
    tr, tc = streaks.tile()
    assert tr >= 1 and tc >= 1


def test_defaults_without_a_gpu():
    from lfd_amd import _native, streaks
    p = _native.make_streak_params()
    assert (p.bin, p.length, p.max_streaks, p.peel_halfwidth, p.clip, p.threshold) == (2, 32, 4, 8, 0.125, 8.0)
    assert streaks.default_params() == S.DEFAULTS
    assert _native.make_streak_params(length=16).length == 16
    with pytest.raises(TypeError):
        _native.make_streak_params(len=16)
    assert S.in_range(p.clip, p.bin, p.length) and int(p.clip * 2 ** 20) * p.bin * p.bin * p.length <= 2 ** 24


def test_as_params_refuses_what_the_library_refuses():
    from lfd_amd import streaks
    for bad in REFUSED:
        with pytest.raises(ValueError):
            streaks.as_params(bad)
        full = dict(S.DEFAULTS)
        full.update(bad)
        with pytest.raises(ValueError):                               # the restatement draws the same line
            S.check_params(full)
    for good in TAKEN:
        assert streaks.as_params(good) == good
        full = dict(S.DEFAULTS)
        full.update(good)
        S.check_params(full)
    assert streaks.as_params(None) == {} and streaks.as_params(True) == {}
    with pytest.raises(TypeError):
        streaks.as_params({"min_len": 3})
    with pytest.raises(ValueError):
        streaks.as_params({"max_streaks": 2.5})
    assert streaks.in_range(0.125, 2, 32) and not streaks.in_range(32.0, 1, 64) and streaks.in_range(2047.0 / 64, 1, 64)


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.STREAK_DTYPE)
    ns = np.zeros(1, np.int32)
    rc = _native.lib().lfdmi_streak_search(None, None, 0, 0, 0, 0, 0, None, None, _native._ptr(res), _native._ptr(ns))
    assert rc == _native.ERR_ARG


def test_streak_rows_round_trip(tmp_path):
    from lfd_amd import streaks
    rec = {"q": 1, "s": -7, "r0": 300, "c0": 12, "n_pix": 120, "snr": np.float32(9.25), "x1": 0.5, "y1": 1.0 / 3, "x2": 1e-7, "y2": -2.5}
    row = streaks.format_row((94, 1, "r", 101), 2, rec)
    assert row.split()[:10] == ["94", "1", "r", "101", "2", "1", "-7", "300", "12", "120"] and len(row.split()) == len(streaks.STREAK_COLUMNS)
    p = tmp_path / "streaks.txt"
    p.write_text(row + "\n\n")
    got, = streaks.read_streaks(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "streak": 2, "q": 1, "s": -7, "r0": 300, "c0": 12, "n_pix": 120,
                   "snr": 9.25, "x1": 0.5, "y1": 1.0 / 3, "x2": 1e-7, "y2": -2.5}


def test_segments_of_found_streaks():
    from lfd_amd import masks, streaks
    rec = np.zeros((2, 3), streaks.STREAK_DTYPE)
    rec[0, 0] = (0, 1, 0, 3, 2, 1, 8, 0.5, 11.0, 0, 1.0, 2.0, 8.0, 5.0, 0.0, 0.0)
    rec[0, 1] = (0, 0, 0, 0, 9, 9, 8, 0.1, 2.0, 0, 9.0, 9.0, 16.0, 9.0, 0.0, 0.0)     # the stopping record: not a segment
    rec[1, 0] = (1, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    segs = streaks.segments(rec, [1, 0])
    assert segs.dtype == masks.SEGMENT_DTYPE and len(segs) == 1
    assert (segs[0]["frame"], segs[0]["x1"], segs[0]["y1"], segs[0]["x2"], segs[0]["y2"]) == (0, 1.0, 2.0, 8.0, 5.0)
    assert segs[0]["half"] == masks.half_width(float("nan")) and segs[0]["bits"] == 1
    assert streaks.segments(rec, [1, 0], half=4.0)[0]["half"] == 4.0 and len(streaks.segments(rec, [0, 0])) == 0
