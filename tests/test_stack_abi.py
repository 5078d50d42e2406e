"""lfdmi_stack, lfdmi_stack_segment and lfdmi_stack_params as Python sees them, without a GPU: the layouts against the header, the
library's defaults, and the rules ``StackParams.validate`` applies (tests/test_gpu_stack.py holds the library to the same values
on a device: its check sits behind the context)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stack_ref as S  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402

# what both sides refuse, and what both take
REFUSED = ({"step": 0.0}, {"step": -0.5}, {"step": 0.7}, {"prof_half": 24.0, "step": 0.04}, {"wing": 24}, {"wing": 30}, {"wing": 0},
           {"n_iter": -1}, {"n_iter": 17}, {"min_cols": 1}, {"clip": 0.0}, {"clip": float("nan")}, {"prof_half": 40.0},
           {"box": -1.0}, {"max_shift": float("inf")}, {"k_sig": float("nan")})
TAKEN = ({}, {"step": 0.25}, {"step": 1.0}, {"prof_half": 25.6, "step": 0.05}, {"wing": 23}, {"n_iter": 0}, {"n_iter": 16},
         {"min_cols": 2}, {"clip": float("inf")}, {"prof_half": 39.5, "step": 0.5}, {"box": 0.0}, {"max_shift": 0.0})


def test_layouts():
    from lfd_amd import _native
    assert _native.STACK_DTYPE.itemsize == 152 and _native.STACK_SEGMENT_DTYPE.itemsize == 40
    assert list(_native.STACK_DTYPE.names) == header_struct("lfdmi_stack") == list(S.FIELDS)
    assert list(_native.STACK_SEGMENT_DTYPE.names) == header_struct("lfdmi_stack_segment")
    assert [k for k, _ in _native.StackParamsStruct._fields_] == header_struct("lfdmi_stack_params")
    assert C.sizeof(_native.StackParamsStruct) == 72
    off = 0
    for k in _native.STACK_DTYPE.names:                   # no padding: four int32, then doubles
        assert _native.STACK_DTYPE.fields[k][1] == off, k
        off += _native.STACK_DTYPE.fields[k][0].itemsize
    assert _native.StackParamsStruct.prof_half.offset == 16 and _native.StackParamsStruct.clip.offset == 12
    assert {"lfdmi_default_stack_params", "lfdmi_stack_profiles"} <= set(_native.SYMBOLS)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert re.search(r"#define LFDMI_STACK_MAX_HALF 40\.0\b", text) and _native.STACK_MAX_HALF == 40.0
    assert re.search(r"LFDMI_STACK_OK = 0, LFDMI_STACK_BAD_SEGMENT = 1, LFDMI_STACK_TOO_SHORT = 2, LFDMI_STACK_TOO_FAINT = 3", text)
    assert (_native.STACK_OK, _native.STACK_BAD_SEGMENT, _native.STACK_TOO_SHORT, _native.STACK_TOO_FAINT) == (0, 1, 2, 3)
    assert _native.lib().lfdmi_version() == 300


def test_defaults_without_a_gpu():
    from lfd_amd import _native, stack
    p = _native.make_stack_params()
    got = {k: getattr(p, k) for k, _ in _native.StackParamsStruct._fields_}
    assert got == S.DEFAULTS == stack.StackParams().as_dict() == stack.default_params().as_dict()
    assert (p.prof_half, p.step, p.wing, p.n_iter, p.min_cols, p.box, p.max_shift, p.clip) == (24.0, 0.5, 8, 2, 64, 4.0, 8.0, 0.125)
    assert _native.stack_bins(p) == S.n_bins() == 97
    assert _native.make_stack_params(step=0.25).step == 0.25
    with pytest.raises(TypeError):
        _native.make_stack_params(prof_step=0.25)


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import stack
    for bad in REFUSED:
        with pytest.raises(ValueError):
            stack.StackParams(**bad).validate()
        with pytest.raises(ValueError):
            stack.as_params(bad)
    for good in TAKEN:
        assert stack.as_params(good) == good
    assert stack.as_params(None) == {}
    with pytest.raises(ValueError):
        stack.StackParams(wing=2.5).validate()
    with pytest.raises(TypeError):
        stack.as_params({"prof_step": 0.5})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    out = np.zeros(1, _native.STACK_DTYPE)
    seg = np.zeros(1, _native.STACK_SEGMENT_DTYPE)
    rc = _native.lib().lfdmi_stack_profiles(None, None, _native.F32, 0, 8, 8, _native.HOST, _native._ptr(seg), 1, None, None,
                                            _native._ptr(out), None, None, None)
    assert rc == _native.ERR_ARG


def test_segments_and_trail_records():
    from lfd_amd import _native, stack
    lines = np.zeros((2, 3), _native.RADON_LINE_DTYPE)
    lines["ex1"], lines["ey1"], lines["ex2"], lines["ey2"] = [[1, 2, 3], [4, 5, 6]], 7, 8, 9
    segs, where = stack.segments_from_radon_lines(lines, [2, 1])
    assert where == [(0, 0), (0, 1), (1, 0)] and segs.dtype == _native.STACK_SEGMENT_DTYPE
    assert segs["frame"].tolist() == [0, 0, 1] and segs["x1"].tolist() == [1.0, 2.0, 4.0] and segs["y2"].tolist() == [9.0] * 3
    res = np.zeros(3, _native.RESULT_DTYPE)
    res["found"], res["x1"], res["y2"] = [1, 0, 2], [5, 6, 7], [9, 9, 11]
    segs, frames = stack.segments_from_results(res)
    assert frames == [0, 2] and segs["x1"].tolist() == [5.0, 7.0] and segs["y2"].tolist() == [9.0, 11.0]
    rec = np.zeros(4, _native.STACK_DTYPE)
    rec["status"], rec["n_col"], rec["peak"], rec["flux"] = [0, 1, 2, 3], 100, 0.5, 7.0
    tr = stack.to_trails(rec)
    assert tr.dtype == _native.TRAIL_DTYPE and tr["n_pos"].tolist() == [100] * 4 and tr["peak"].tolist() == [0.5] * 4
    assert tr["status"].tolist() == [_native.TRAIL_OK, _native.TRAIL_NOT_FOUND, _native.TRAIL_TOO_SHORT, _native.TRAIL_TOO_FAINT]
    row = stack.format_row((94, 1, "r", 12), 1, rec[0]).split()
    assert len(row) == len(stack.PROFILE_COLUMNS) and row[:6] == ["94", "1", "r", "12", "1", "0"] and row[10] == "100"


def test_dropin_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    with pytest.raises(ValueError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_profiles=True)
    with pytest.raises(ValueError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_lines=2, radon_profiles=True,
                     stack_params={"step": 0.7})
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_lines=2, radon_profiles=True,
                 stack_params={"step": 0.25})
