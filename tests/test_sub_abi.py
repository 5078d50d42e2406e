"""lfdmi_sub and lfdmi_sub_params as Python sees them, without a GPU: the layouts against the header and against the
restatement, the library's defaults, the exported symbols, and the Python side of the trail subtraction (parameters, segments,
model maps, rows)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sub_ref as UR  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402


def test_layouts():
    from lfd_amd import _native
    N = _native
    assert N.SUB_DTYPE.itemsize == 56 and C.sizeof(N.SubParamsStruct) == 48 and N.SUB_PARAMS is N.SubParamsStruct
    assert list(N.SUB_DTYPE.names) == header_struct("lfdmi_sub")
    assert [k for k, _ in N.SubParamsStruct._fields_] == header_struct("lfdmi_sub_params")
    assert N.SUB_DTYPE == UR.SUB_DTYPE and N.STRIP_SEGMENT_DTYPE == UR.SEGMENT_DTYPE
    off = 0
    for k in N.SUB_DTYPE.names:                                         # no padding the header does not name
        assert N.SUB_DTYPE.fields[k][1] == off, k
        off += N.SUB_DTYPE.fields[k][0].itemsize
    assert off == 56
    P = N.SubParamsStruct
    assert (P.sec_len.offset, P.step.offset, P.wing.offset, P.clip.offset, P.smooth.offset, P.min_sec.offset, P.min_n.offset,
            P.min_wing.offset, P.apply.offset) == (0, 8, 16, 24, 28, 32, 36, 40, 44)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert "trail subtraction" in text
    assert re.search(r"#define LFDMI_SUB_MAX_SMOOTH 8\b", text) and N.SUB_MAX_SMOOTH == UR.MAX_SMOOTH == 8
    assert re.search(r"LFDMI_SUB_OK = 0, LFDMI_SUB_BAD_SEGMENT = 1, LFDMI_SUB_TOO_LONG = 2, LFDMI_SUB_EMPTY = 3", text)
    assert (N.SUB_OK, N.SUB_BAD_SEGMENT, N.SUB_TOO_LONG, N.SUB_EMPTY) == (UR.OK, UR.BAD_SEGMENT, UR.TOO_LONG, UR.EMPTY) == (0, 1, 2, 3)


def test_symbols_are_exported():
    from lfd_amd import _native
    assert {"lfdmi_default_sub_params", "lfdmi_subtract_trails"} <= set(_native.SYMBOLS)
    lib = _native.lib()
    for name in ("lfdmi_default_sub_params", "lfdmi_subtract_trails"):
        assert getattr(lib, name) is not None
    assert len(lib.lfdmi_subtract_trails.argtypes) == 17 and len(lib.lfdmi_default_sub_params.argtypes) == 1


def test_defaults_without_a_gpu():
    from lfd_amd import _native, subtract
    p = _native.make_sub_params()
    got = {k: getattr(p, k) for k in subtract.PARAM_NAMES}
    assert got == UR.DEFAULTS == {"sec_len": 32.0, "step": 1.0, "wing": 6.0, "clip": 0.125, "smooth": 2, "min_sec": 3, "min_n": 8,
                                  "min_wing": 8, "apply": 1}
    assert subtract.DEFAULT_WING == p.wing and subtract.PARAM_NAMES == tuple(UR.DEFAULTS)
    assert _native.make_sub_params(sec_len=4.0, smooth=8).smooth == 8
    with pytest.raises(TypeError):
        _native.make_sub_params(section=1)
    for bad in ({"sec_len": 3.9}, {"sec_len": 4097.0}, {"sec_len": float("nan")}, {"step": 0.49}, {"step": 8.1}, {"wing": 0.0},
                {"wing": float("inf")}, {"clip": 0.0}, {"clip": float("inf")}, {"clip": 1025.0}, {"smooth": -1}, {"smooth": 9},
                {"smooth": 0}, {"min_sec": 0}, {"min_sec": 6}, {"smooth": 8, "min_sec": 18}, {"min_n": 0}, {"min_wing": 0},
                {"min_wing": 1.5}, {"apply": 2}):
        with pytest.raises(ValueError):
            subtract.as_params(bad)
    for good in ({}, {"sec_len": 4.0}, {"sec_len": 4096.0}, {"step": 0.5}, {"step": 8.0}, {"smooth": 0, "min_sec": 1},
                 {"smooth": 8, "min_sec": 17}, {"min_n": 1, "min_wing": 1}, {"apply": 0}):
        assert subtract.as_params(good) == good
    with pytest.raises(TypeError):
        subtract.as_params({"k_mom": 5.0})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    out = np.zeros(1, _native.SUB_DTYPE)
    seg = np.zeros(1, _native.STRIP_SEGMENT_DTYPE)
    rc = _native.lib().lfdmi_subtract_trails(None, None, _native.F32, 0, 8, 8, _native.HOST, None, 0, _native._ptr(seg), 1, None, None,
                                             _native._ptr(out), None, 4, 8)
    assert rc == _native.ERR_ARG
    _native.lib().lfdmi_default_sub_params(None)                        # (a NULL is ignored)


def test_segments_maps_and_rows(tmp_path):
    from lfd_amd import _native, masks, subtract
    lines = np.zeros((2, 3), _native.RADON_LINE_DTYPE)
    lines["ex1"], lines["ey1"], lines["ex2"], lines["ey2"] = [[1, 2, 3], [4, 5, 6]], 7, 8, 9
    ms, where = masks.segments_from_radon_lines(lines, [2, 1])
    ss = subtract.segments_from_mask_segments(ms)
    assert ss.dtype == _native.STRIP_SEGMENT_DTYPE and ss["frame"].tolist() == [0, 0, 1] and (ss["half"] == ms["half"] + 6.0).all()
    assert (subtract.segments_from_mask_segments(ms, margin=2.5)["half"] == ms["half"] + 2.5).all()
    frames = np.random.default_rng(1).normal(0, 0.025, (1, 40, 90)).astype(np.float32)
    frames[0, 17:23] += np.float32(0.05)
    sg = np.array([UR.segment(0, 2.0, 20.0, 80.0, 21.0, half=14.0)], UR.SEGMENT_DTYPE)
    clean, rec, tab = UR.subtract_trails(frames, sg, sec_len=8.0, max_sections=16)
    m = subtract.model_maps(rec[0], tab[0])
    assert m.shape == (10, 29) and m.dtype == np.float32 and np.array_equal(m, tab[0][:290].reshape(10, 29))
    bad = np.zeros(1, _native.SUB_DTYPE)[0]
    bad["status"] = subtract.BAD_SEGMENT
    assert subtract.model_maps(bad, tab[0]).shape == (0, 0)
    rows = subtract.format_rows((94, 1, "r", 12), "detect", 0, rec[0])
    assert len(rows) == 1 and len(rows[0].split()) == len(subtract.SUB_COLUMNS) == 14
    path = tmp_path / "subtracted.txt"
    path.write_text("\n".join(rows) + "\n")
    back = subtract.read_subtracted(str(path))[0]
    assert back["source"] == "detect" and back["filter"] == "r" and back["status"] == subtract.OK
    for k in ("n_sec", "n_usable", "n_model", "n_pix", "peak_section", "removed", "peak"):
        assert back[k] == rec[0][k], k
