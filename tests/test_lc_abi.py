"""lfdmi_lc, lfdmi_lc_section, lfdmi_lc_segment and lfdmi_lc_params as Python sees them, without a GPU: the layouts against the
header and against the restatement, the library's defaults, the exported symbols, and the Python side of the light curves
(segments, rows, magnitudes)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402


def test_layouts():
    from lfd_amd import _native
    assert _native.LC_SEGMENT_DTYPE.itemsize == 64 and _native.LC_DTYPE.itemsize == 88 and _native.LC_SECTION_DTYPE.itemsize == 112
    assert C.sizeof(_native.LcParamsStruct) == 24 and _native.LC_PARAMS is _native.LcParamsStruct
    assert list(_native.LC_SEGMENT_DTYPE.names) == header_struct("lfdmi_lc_segment")
    assert list(_native.LC_DTYPE.names) == header_struct("lfdmi_lc")
    assert list(_native.LC_SECTION_DTYPE.names) == header_struct("lfdmi_lc_section")
    assert [k for k, _ in _native.LcParamsStruct._fields_] == header_struct("lfdmi_lc_params")
    assert _native.LC_SEGMENT_DTYPE == LR.SEGMENT_DTYPE and _native.LC_DTYPE == LR.LC_DTYPE and _native.LC_SECTION_DTYPE == LR.SECTION_DTYPE
    for dt in (_native.LC_SEGMENT_DTYPE, _native.LC_DTYPE, _native.LC_SECTION_DTYPE):      # no padding the header does not name
        off = 0
        for k in dt.names:
            assert dt.fields[k][1] == off, k
            off += dt.fields[k][0].itemsize
        assert off == dt.itemsize
    P = _native.LcParamsStruct
    assert (P.sec_len.offset, P.clip.offset, P.min_core.offset, P.min_sky.offset) == (0, 8, 12, 16)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert "light curves" in text
    assert re.search(r"#define LFDMI_LC_MAX_SECTIONS 1024\b", text) and _native.LC_MAX_SECTIONS == LR.MAX_SECTIONS == 1024
    assert re.search(r"#define LFDMI_LC_MAX_BG 64\.0\b", text) and _native.LC_MAX_BG == LR.MAX_BG == 64.0
    assert re.search(r"LFDMI_LC_OK = 0, LFDMI_LC_BAD_SEGMENT = 1, LFDMI_LC_TOO_LONG = 2, LFDMI_LC_EMPTY = 3", text)
    assert re.search(r"LFDMI_LC_SEC_OK = 0, LFDMI_LC_SEC_LOW = 1, LFDMI_LC_SEC_EMPTY = 2", text)
    assert (_native.LC_OK, _native.LC_BAD_SEGMENT, _native.LC_TOO_LONG, _native.LC_EMPTY) == (LR.OK, LR.BAD_SEGMENT, LR.TOO_LONG, LR.EMPTY) == (0, 1, 2, 3)
    assert (_native.LC_SEC_OK, _native.LC_SEC_LOW, _native.LC_SEC_EMPTY) == (LR.SEC_OK, LR.SEC_LOW, LR.SEC_EMPTY) == (0, 1, 2)


def test_symbols_are_exported():
    from lfd_amd import _native
    assert {"lfdmi_default_lc_params", "lfdmi_light_curves"} <= set(_native.SYMBOLS)
    lib = _native.lib()
    for name in ("lfdmi_default_lc_params", "lfdmi_light_curves"):
        assert getattr(lib, name) is not None
    assert len(lib.lfdmi_light_curves.argtypes) == 16


def test_defaults_without_a_gpu():
    from lfd_amd import _native, lightcurve
    p = _native.make_lc_params()
    got = {k: getattr(p, k) for k, _ in _native.LcParamsStruct._fields_}
    assert got == LR.DEFAULTS == {"sec_len": 32.0, "clip": 0.125, "min_core": 32, "min_sky": 32}
    assert _native.make_lc_params(sec_len=8.0).sec_len == 8.0
    with pytest.raises(TypeError):
        _native.make_lc_params(section=8.0)
    assert lightcurve.PARAM_NAMES == tuple(LR.DEFAULTS)
    for bad in ({"sec_len": 7.9}, {"sec_len": 4097.0}, {"sec_len": float("nan")}, {"clip": 0.0}, {"clip": float("inf")}, {"clip": 1025.0},
                {"min_core": 0}, {"min_sky": 0}, {"min_sky": 1.5}):
        with pytest.raises(ValueError):
            lightcurve.as_params(bad)
    for good in ({}, {"sec_len": 8.0}, {"sec_len": 4096.0}, {"clip": 1024.0}, {"min_core": 1, "min_sky": 1}):
        assert lightcurve.as_params(good) == good
    with pytest.raises(TypeError):
        lightcurve.as_params({"section": 8})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    out = np.zeros(1, _native.LC_DTYPE)
    sec = np.zeros((1, 4), _native.LC_SECTION_DTYPE)
    seg = np.zeros(1, _native.LC_SEGMENT_DTYPE)
    rc = _native.lib().lfdmi_light_curves(None, None, _native.F32, 0, 8, 8, _native.HOST, None, 0, _native._ptr(seg), 1, None, None,
                                          _native._ptr(out), _native._ptr(sec), 4)
    assert rc == _native.ERR_ARG
    _native.lib().lfdmi_default_lc_params(None)                         # (a NULL is ignored)


def test_segments_rows_and_magnitudes(tmp_path):
    from lfd_amd import _native, lightcurve, masks
    segs = lightcurve.segments([(2, 1.0, 2.0, 3.0, 4.0, 8.0), (0, 0.0, 0.0, 9.0, 0.0, 50.0)])
    assert segs.dtype == _native.LC_SEGMENT_DTYPE and segs["frame"].tolist() == [2, 0]
    assert segs["bg_in"].tolist() == [12.0, 54.0] and segs["bg_out"].tolist() == [28.0, 64.0]
    assert lightcurve.segments([(0, 0, 0, 1, 1, 3.0)], bg_gap=0.0, bg_width=5.0)[0]["bg_out"] == 8.0
    lines = np.zeros((2, 3), _native.RADON_LINE_DTYPE)
    lines["ex1"], lines["ey1"], lines["ex2"], lines["ey2"] = [[1, 2, 3], [4, 5, 6]], 7, 8, 9
    ms, where = masks.segments_from_radon_lines(lines, [2, 1])
    ls = lightcurve.segments_from_mask_segments(ms)
    assert where == [(0, 0), (0, 1), (1, 0)] and ls["frame"].tolist() == [0, 0, 1] and ls["x1"].tolist() == [1.0, 2.0, 4.0]
    assert (ls["half"] == ms["half"]).all() and (ls["half"] == 10.0).all() and (ls["bg_in"] == 14.0).all() and (ls["bg_out"] == 30.0).all()
    # magnitudes and variability
    assert lightcurve.magnitude(1.0) == 22.5 and abs(lightcurve.magnitude(100.0) - 17.5) < 1e-12
    m = lightcurve.magnitude([10.0, 0.0, -1.0, np.nan])
    assert m[0] == 20.0 and np.isnan(m[1:]).all()
    rec = np.zeros(3, _native.LC_DTYPE)
    rec["chi2"], rec["dof"] = [6.0, 1.0, np.nan], [3, 0, -1]
    v = lightcurve.variability(rec)
    assert v[0] == 2.0 and np.isnan(v[1:]).all()
    # the rows: written and read back
    frames = np.random.default_rng(1).normal(0, 0.025, (1, 40, 90)).astype(np.float32)
    seg = np.array([LR.segment(0, 2.0, 20.0, 80.0, 21.0, half=3.0)], LR.SEGMENT_DTYPE)
    rec, sec = LR.light_curves(frames, seg, max_sections=8, sec_len=16.0)
    rows = lightcurve.format_rows((94, 1, "r", 12), "detect", 0, rec[0], sec[0])
    assert len(rows) == int(rec[0]["n_sec"]) == 5 and all(len(r.split()) == len(lightcurve.LC_COLUMNS) for r in rows)
    p = tmp_path / "lightcurves.txt"
    p.write_text("\n".join(rows) + "\n")
    back = lightcurve.read_lightcurves(str(p))
    assert [r["section"] for r in back] == list(range(5)) and back[0]["source"] == "detect" and back[0]["filter"] == "r"
    for j, r in enumerate(back):
        assert r["n_core"] == sec[0, j]["n_core"] and r["t1"] == sec[0, j]["t1"]
        assert r["rate"] == sec[0, j]["rate"] or (np.isnan(r["rate"]) and np.isnan(sec[0, j]["rate"]))
    srow = lightcurve.format_summary_row((94, 1, "r", 12), "radon", 3, rec[0])
    assert len(srow.split()) == len(lightcurve.SUMMARY_COLUMNS)
    s = tmp_path / "lightcurve_summary.txt"
    s.write_text(srow + "\n")
    back = lightcurve.read_summary(str(s))[0]
    assert back["line"] == 3 and back["n_sec"] == 5 and back["mean_rate"] == rec[0]["mean_rate"] and back["dof"] == rec[0]["dof"]
