"""lfdmi_radon_wide and lfdmi_radon_wide_params as Python sees them, without a GPU: the record's layout against the header,
the library's defaults, the symbol list, and the rules ``RadonWideParams.validate`` applies -- every LFDMI_ERR_ARG of the call
(tests/test_gpu_radon_wide.py holds the library to the same values on a device: its check sits behind the context)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_radon_lines_abi import header_struct  # noqa: E402

# what both sides refuse, and what both take, with a handle of min_len = 64
REFUSED = ({"max_width": 0}, {"max_width": 3}, {"max_width": 12}, {"max_width": 32}, {"max_width": -4}, {"max_lines": 0},
           {"max_lines": 9}, {"peel_halfwidth": -1}, {"min_seg": 0}, {"min_seg": 65}, {"wide_threshold": 0.0},
           {"wide_threshold": -1.0}, {"wide_threshold": float("inf")}, {"wide_threshold": float("nan")})
TAKEN = ({}, {"max_width": 1}, {"max_width": 2}, {"max_width": 16}, {"max_lines": 1}, {"max_lines": 8}, {"peel_halfwidth": 0},
         {"min_seg": 1}, {"min_seg": 64}, {"wide_threshold": 1e-3})


def test_record_layout():
    from lfd_amd import _native
    assert C.sizeof(_native.RadonWide) == _native.RADON_WIDE_DTYPE.itemsize == 152
    names = [k for k, _ in _native.RadonWide._fields_]
    assert names == list(_native.RADON_WIDE_DTYPE.names) == header_struct("lfdmi_radon_wide")
    line = list(_native.RADON_LINE_DTYPE.names)
    assert names[:len(line)] == line and names[len(line):] == ["width", "pad2", "width_px"]       # lfdmi_radon_line comes first
    for k in names:
        assert getattr(_native.RadonWide, k).offset == _native.RADON_WIDE_DTYPE.fields[k][1], k
        assert getattr(_native.RadonWide, k).size == _native.RADON_WIDE_DTYPE.fields[k][0].itemsize, k
    for k in line:                                                    # the segment fields sit where the lines' do
        assert _native.RADON_WIDE_DTYPE.fields[k][1] == _native.RADON_LINE_DTYPE.fields[k][1], k
    assert (_native.RadonWide.width.offset, _native.RadonWide.pad2.offset, _native.RadonWide.width_px.offset) == (136, 140, 144)
    assert [k for k, _ in _native.RadonWideParamsStruct._fields_] == header_struct("lfdmi_radon_wide_params")
    assert C.sizeof(_native.RadonWideParamsStruct) == 24
    assert [getattr(_native.RadonWideParamsStruct, k).offset for k, _ in _native.RadonWideParamsStruct._fields_] == [0, 4, 8, 12, 16, 20]


def test_symbols():
    from lfd_amd import _native
    assert {"lfdmi_default_radon_wide_params", "lfdmi_radon_search_wide"} <= set(_native.SYMBOLS)
    lib = _native.lib()
    assert hasattr(lib, "lfdmi_default_radon_wide_params") and hasattr(lib, "lfdmi_radon_search_wide")
    assert _native.RADON_MAX_WIDTH == 16
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfdmi.h")) as f:
        assert "#define LFDMI_RADON_MAX_WIDTH 16\n" in f.read()


def test_defaults_without_a_gpu():
    from lfd_amd import _native, radon
    p = _native.make_radon_wide_params()
    assert (p.max_width, p.max_lines, p.peel_halfwidth, p.min_seg, p.wide_threshold, p.pad) == (8, 4, 8, 64, 8.0, 0)
    assert radon.default_wide_params() == radon.RadonWideParams() == radon.RadonWideParams(8, 4, 8, 64, 8.0)
    assert _native.make_radon_wide_params(max_width=16).max_width == 16
    with pytest.raises(TypeError) as e:
        _native.make_radon_wide_params(width=16)
    assert str(e.value) == "unknown radon wide parameter 'width'"
    import radon_wide_ref as W
    assert W.WIDE_DEFAULTS == radon.RadonWideParams().as_dict()


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import radon
    for bad in REFUSED:
        with pytest.raises(ValueError):
            radon.RadonWideParams(**bad).validate(min_len=64)
        with pytest.raises(ValueError):
            radon.as_wide_params(bad, min_len=64)
    for good in TAKEN:
        assert radon.as_wide_params(good, min_len=64) == good
        radon.RadonWideParams(**good).validate(64)
    assert radon.as_wide_params(None) == {}
    radon.RadonWideParams(min_seg=65).validate()                     # without a handle's min_len only the lower bound is known
    with pytest.raises(ValueError):
        radon.RadonWideParams(max_lines=2.5).validate()
    with pytest.raises(TypeError):
        radon.as_wide_params({"threshold": 3})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.RADON_WIDE_DTYPE)
    nl = np.zeros(1, np.int32)
    rc = _native.lib().lfdmi_radon_search_wide(None, None, None, 0, 0, 0, None, None, _native._ptr(res), _native._ptr(nl), None)
    assert rc == _native.ERR_ARG


def test_wide_rows_round_trip(tmp_path):
    from lfd_amd import radon
    rec = {"width": 8, "width_px": 15.5, "snr": np.float32(9.25), "n_pix": 4000, "ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7, "ey2": -2.5,
           "seg_snr": np.float32(12.3), "seg_n_pix": 3210}
    row = radon.format_wide_row((94, 1, "r", 101), 1, rec)
    assert row.split()[:7] == ["94", "1", "r", "101", "1", "8", "15.5"] and len(row.split()) == len(radon.WIDE_COLUMNS)
    assert radon.WIDE_COLUMNS == ("run", "camcol", "filter", "field", "line", "width", "width_px", "snr", "n_pix", "ex1", "ey1", "ex2",
                                  "ey2", "seg_snr", "seg_n_pix")
    p = tmp_path / "radon_wide.txt"
    p.write_text(row + "\n\n")
    got, = radon.read_wide(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "line": 1, "width": 8, "width_px": 15.5, "snr": 9.25,
                   "n_pix": 4000, "ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7, "ey2": -2.5, "seg_snr": float(np.float32(12.3)),
                   "seg_n_pix": 3210}


def test_segments_of_found_bands():
    from lfd_amd import _native, masks, stack
    lines = np.zeros((2, 3), _native.RADON_WIDE_DTYPE)
    lines[1, 0]["ex1"], lines[1, 0]["ey1"], lines[1, 0]["ex2"], lines[1, 0]["ey2"] = 1.5, 2.5, 30.5, 40.5
    lines[1, 0]["width"], lines[1, 0]["width_px"] = 8, 13.0
    lines[1, 1]["width_px"] = 2.0
    segs, where = masks.segments_from_radon_wide(lines, [0, 2])
    assert where == [(1, 0), (1, 1)] and segs.dtype == masks.SEGMENT_DTYPE
    assert segs["half"].tolist() == [13.0 / 2 + 2, 3.0] and segs["frame"].tolist() == [1, 1]
    assert (segs[0]["x1"], segs[0]["y1"], segs[0]["x2"], segs[0]["y2"]) == (1.5, 2.5, 30.5, 40.5)
    ssegs, swhere = stack.segments_from_radon_wide(lines, [0, 2])
    assert swhere == where and (ssegs[0]["x1"], ssegs[0]["y2"]) == (1.5, 40.5) and ssegs["frame"].tolist() == [1, 1]


def test_dropin_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd import radon
    from lfd_amd.detecttrails import DetectTrails
    kw = {"run": 94, "camcol": 1, "filter": "r", "savepath": str(tmp_path)}
    with pytest.raises(ValueError):                                   # a mode of the faint-trail search
        DetectTrails(radon_wide=True, **kw)
    for bad in ({"max_width": 12}, {"min_seg": 257}, {"wide_threshold": 0.0}, {"max_lines": 9}):
        with pytest.raises(ValueError):
            DetectTrails(radon=True, radon_wide=bad, **kw)
    with pytest.raises(TypeError):
        DetectTrails(radon=True, radon_wide={"width": 8}, **kw)
    dt = DetectTrails(radon=True, radon_wide=True, **kw)
    assert dt.radon_wide == {} and dt.radon_wide_file == os.path.join(str(tmp_path), "radon_wide.txt")
    dt = DetectTrails(radon=True, radon_wide={"min_seg": 256}, radon_profiles=True, **kw)   # profiles without radon_lines
    assert dt.radon_wide == {"min_seg": 256}
    dt = DetectTrails(radon=True, radon_wide=radon.RadonWideParams(max_lines=2), **kw)
    assert dt.radon_wide["max_lines"] == 2 and DetectTrails(**kw).radon_wide is None
