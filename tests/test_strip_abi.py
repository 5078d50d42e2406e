"""lfdmi_strip, lfdmi_strip_section, lfdmi_strip_cell, lfdmi_strip_segment and lfdmi_strip_params as Python sees them, without a
GPU: the layouts against the header and against the restatement, the library's defaults, the exported symbols, and the Python
side of the trail strips (segments, maps, rows)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strip_ref as SR  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402


def test_layouts():
    from lfd_amd import _native
    N = _native
    assert N.STRIP_SEGMENT_DTYPE.itemsize == 48 and N.STRIP_DTYPE.itemsize == 56 and N.STRIP_SECTION_DTYPE.itemsize == 72
    assert N.STRIP_CELL_DTYPE.itemsize == 16
    assert C.sizeof(N.StripParamsStruct) == 48 and N.STRIP_PARAMS is N.StripParamsStruct
    assert list(N.STRIP_SEGMENT_DTYPE.names) == header_struct("lfdmi_strip_segment")
    assert list(N.STRIP_DTYPE.names) == header_struct("lfdmi_strip")
    assert list(N.STRIP_SECTION_DTYPE.names) == header_struct("lfdmi_strip_section")
    assert list(N.STRIP_CELL_DTYPE.names) == header_struct("lfdmi_strip_cell")
    assert [k for k, _ in N.StripParamsStruct._fields_] == header_struct("lfdmi_strip_params")
    assert N.STRIP_SEGMENT_DTYPE == SR.SEGMENT_DTYPE and N.STRIP_DTYPE == SR.STRIP_DTYPE
    assert N.STRIP_SECTION_DTYPE == SR.SECTION_DTYPE and N.STRIP_CELL_DTYPE == SR.CELL_DTYPE
    for dt in (N.STRIP_SEGMENT_DTYPE, N.STRIP_DTYPE, N.STRIP_SECTION_DTYPE, N.STRIP_CELL_DTYPE):   # no padding the header does not name
        off = 0
        for k in dt.names:
            assert dt.fields[k][1] == off, k
            off += dt.fields[k][0].itemsize
        assert off == dt.itemsize
    P = N.StripParamsStruct
    assert (P.sec_len.offset, P.step.offset, P.wing.offset, P.k_mom.offset, P.clip.offset, P.min_core.offset, P.min_wing.offset) == \
        (0, 8, 16, 24, 32, 36, 40)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert "trail strips" in text
    assert re.search(r"#define LFDMI_STRIP_MAX_SECTIONS 1024\b", text) and N.STRIP_MAX_SECTIONS == SR.MAX_SECTIONS == 1024
    assert re.search(r"#define LFDMI_STRIP_MAX_OFF 129\b", text) and N.STRIP_MAX_OFF == SR.MAX_OFF == 129
    assert re.search(r"LFDMI_STRIP_OK = 0, LFDMI_STRIP_BAD_SEGMENT = 1, LFDMI_STRIP_TOO_LONG = 2, LFDMI_STRIP_EMPTY = 3", text)
    assert re.search(r"LFDMI_STRIP_SEC_OK = 0, LFDMI_STRIP_SEC_LOW = 1, LFDMI_STRIP_SEC_EMPTY = 2", text)
    assert (N.STRIP_OK, N.STRIP_BAD_SEGMENT, N.STRIP_TOO_LONG, N.STRIP_EMPTY) == (SR.OK, SR.BAD_SEGMENT, SR.TOO_LONG, SR.EMPTY) == (0, 1, 2, 3)
    assert (N.STRIP_SEC_OK, N.STRIP_SEC_LOW, N.STRIP_SEC_EMPTY) == (SR.SEC_OK, SR.SEC_LOW, SR.SEC_EMPTY) == (0, 1, 2)


def test_symbols_are_exported():
    from lfd_amd import _native
    assert {"lfdmi_default_strip_params", "lfdmi_trail_strips"} <= set(_native.SYMBOLS)
    lib = _native.lib()
    for name in ("lfdmi_default_strip_params", "lfdmi_trail_strips"):
        assert getattr(lib, name) is not None
    assert len(lib.lfdmi_trail_strips.argtypes) == 18 and len(lib.lfdmi_default_strip_params.argtypes) == 1


def test_defaults_without_a_gpu():
    from lfd_amd import _native, strips
    p = _native.make_strip_params()
    got = {k: getattr(p, k) for k in strips.PARAM_NAMES}
    assert got == SR.DEFAULTS == {"sec_len": 8.0, "step": 1.0, "wing": 6.0, "k_mom": 5.0, "clip": 0.125, "min_core": 8, "min_wing": 8}
    assert p.pad == 0 and strips.DEFAULT_WING == p.wing
    assert _native.make_strip_params(sec_len=4.0, step=0.5).step == 0.5
    for bad in ("section", "pad"):
        with pytest.raises(TypeError):
            _native.make_strip_params(**{bad: 1})
    assert strips.PARAM_NAMES == tuple(SR.DEFAULTS)
    for bad in ({"sec_len": 3.9}, {"sec_len": 4097.0}, {"sec_len": float("nan")}, {"step": 0.49}, {"step": 8.1}, {"wing": 0.0},
                {"wing": float("inf")}, {"k_mom": -1.0}, {"clip": 0.0}, {"clip": float("inf")}, {"clip": 1025.0}, {"min_core": 0},
                {"min_wing": 0}, {"min_wing": 1.5}):
        with pytest.raises(ValueError):
            strips.as_params(bad)
    for good in ({}, {"sec_len": 4.0}, {"sec_len": 4096.0}, {"step": 0.5}, {"step": 8.0}, {"k_mom": 0.0}, {"min_core": 1, "min_wing": 1}):
        assert strips.as_params(good) == good
    with pytest.raises(TypeError):
        strips.as_params({"section": 8})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    out = np.zeros(1, _native.STRIP_DTYPE)
    sec = np.zeros((1, 4), _native.STRIP_SECTION_DTYPE)
    cel = np.zeros((1, 8), _native.STRIP_CELL_DTYPE)
    seg = np.zeros(1, _native.STRIP_SEGMENT_DTYPE)
    rc = _native.lib().lfdmi_trail_strips(None, None, _native.F32, 0, 8, 8, _native.HOST, None, 0, _native._ptr(seg), 1, None, None,
                                          _native._ptr(out), _native._ptr(sec), 4, _native._ptr(cel), 8)
    assert rc == _native.ERR_ARG
    _native.lib().lfdmi_default_strip_params(None)                      # (a NULL is ignored)


def test_segments_maps_and_rows(tmp_path):
    from lfd_amd import _native, masks, strips
    segs = strips.segments([(2, 1.0, 2.0, 3.0, 4.0, 8.0), (0, 0.0, 0.0, 9.0, 0.0, 50.0)])
    assert segs.dtype == _native.STRIP_SEGMENT_DTYPE and segs["frame"].tolist() == [2, 0] and segs["half"].tolist() == [8.0, 50.0]
    lines = np.zeros((2, 3), _native.RADON_LINE_DTYPE)
    lines["ex1"], lines["ey1"], lines["ex2"], lines["ey2"] = [[1, 2, 3], [4, 5, 6]], 7, 8, 9
    ms, where = masks.segments_from_radon_lines(lines, [2, 1])
    ss = strips.segments_from_mask_segments(ms)
    assert ss["frame"].tolist() == [0, 0, 1] and ss["x1"].tolist() == [1.0, 2.0, 4.0] and (ss["half"] == ms["half"] + 6.0).all()
    assert (strips.segments_from_mask_segments(ms, margin=2.5)["half"] == ms["half"] + 2.5).all()
    # the needed cells: the restatement's count
    p = _native.make_strip_params(sec_len=8.0)
    sg = np.array([SR.segment(0, 2.0, 20.0, 80.0, 21.0, half=14.0), SR.segment(0, 0.0, 0.0, 5000.0, 0.0, half=3.0),
                   SR.segment(0, 0.0, 0.0, np.nan, 0.0, half=3.0), SR.segment(0, 0.0, 0.0, 9.0, 0.0, half=80.0)], SR.SEGMENT_DTYPE)
    assert _native.strip_cells_needed(sg, p, 256) == SR.cells_needed(sg, dict(SR.DEFAULTS), 256) == 10 * 29
    # maps and rows of a measured segment: written and read back
    frames = np.random.default_rng(1).normal(0, 0.025, (1, 40, 90)).astype(np.float32)
    rec, sec, cel = SR.trail_strips(frames, sg[:1], max_sections=16)
    m = strips.maps(rec[0], cel[0])
    assert m["mean"].shape == m["n"].shape == m["n_geom"].shape == (10, 29) and m["mean"].dtype == np.float32
    assert np.array_equal(m["mean"], SR.mean_map(cel[0][:290]).reshape(10, 29), equal_nan=True)
    assert np.isnan(m["mean"][m["n"] == 0]).all() and np.isfinite(m["mean"][m["n"] > 0]).all()
    bad = np.zeros(1, _native.STRIP_DTYPE)[0]
    bad["status"] = strips.BAD_SEGMENT
    assert strips.maps(bad, cel[0])["mean"].shape == (0, 0)
    rows = strips.format_rows((94, 1, "r", 12), "detect", 0, rec[0], sec[0])
    assert len(rows) == 10 and all(len(r.split()) == len(strips.STRIP_COLUMNS) == 17 for r in rows)
    path = tmp_path / "strips.txt"
    path.write_text("\n".join(rows) + "\n")
    back = strips.read_strips(str(path))
    assert [r["section"] for r in back] == list(range(10)) and back[0]["source"] == "detect" and back[0]["filter"] == "r"
    for j, r in enumerate(back):
        assert r["n_core"] == sec[0, j]["n_core"] and r["t1"] == sec[0, j]["t1"] and r["status"] == sec[0, j]["status"]
        for k in ("rate", "centre", "width"):
            assert r[k] == sec[0, j][k] or (np.isnan(r[k]) and np.isnan(sec[0, j][k]))
    strips.write_png(str(tmp_path / "s.png"), m["mean"])
    assert (tmp_path / "s.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
