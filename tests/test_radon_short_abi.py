"""lfdmi_radon_short and lfdmi_radon_short_params as Python sees them, without a GPU: the record's layout against the header,
the library's defaults, and the rules ``RadonShortParams.validate`` applies -- every LFDMI_ERR_ARG of the call
(tests/test_gpu_radon_short.py holds the library to the same values on a device: its check sits behind the context)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402

# what both sides refuse, and what both take, with a handle of bin = 1 (min_seg at most min_strip / 2)
REFUSED = ({"min_strip": 32}, {"min_strip": 96}, {"min_strip": 0}, {"max_lines": 0}, {"max_lines": 9}, {"peel_halfwidth": -1},
           {"min_seg": 0}, {"min_seg": 33}, {"min_strip": 128, "min_seg": 65}, {"short_threshold": 0.0}, {"short_threshold": -1.0},
           {"short_threshold": float("inf")}, {"short_threshold": float("nan")})
TAKEN = ({}, {"min_strip": 128, "min_seg": 64}, {"max_lines": 1}, {"max_lines": 8}, {"peel_halfwidth": 0}, {"min_seg": 1},
         {"min_seg": 32}, {"short_threshold": 1e-3})


def test_record_layout():
    from lfd_amd import _native
    assert C.sizeof(_native.RadonShort) == _native.RADON_SHORT_DTYPE.itemsize == 152
    names = [k for k, _ in _native.RadonShort._fields_]
    assert names == list(_native.RADON_SHORT_DTYPE.names) == header_struct("lfdmi_radon_short")
    line = list(_native.RADON_LINE_DTYPE.names)
    assert names[:len(line)] == line and names[len(line):] == ["level", "strip", "ys", "ss"]     # lfdmi_radon_line comes first
    for k in names:
        assert getattr(_native.RadonShort, k).offset == _native.RADON_SHORT_DTYPE.fields[k][1], k
        assert getattr(_native.RadonShort, k).size == _native.RADON_SHORT_DTYPE.fields[k][0].itemsize, k
    for k in line:                                                    # the segment fields sit where the lines' do
        assert _native.RADON_SHORT_DTYPE.fields[k][1] == _native.RADON_LINE_DTYPE.fields[k][1], k
    assert [k for k, _ in _native.RadonShortParamsStruct._fields_] == header_struct("lfdmi_radon_short_params")
    assert C.sizeof(_native.RadonShortParamsStruct) == 24
    assert {"lfdmi_default_radon_short_params", "lfdmi_radon_search_short"} <= set(_native.SYMBOLS)


def test_defaults_without_a_gpu():
    from lfd_amd import _native, radon
    p = _native.make_radon_short_params()
    assert (p.min_strip, p.max_lines, p.peel_halfwidth, p.min_seg, p.short_threshold, p.pad) == (64, 4, 8, 32, 8.5, 0)
    assert radon.default_short_params() == radon.RadonShortParams() == radon.RadonShortParams(64, 4, 8, 32, 8.5)
    assert _native.make_radon_short_params(min_strip=128).min_strip == 128
    with pytest.raises(TypeError):
        _native.make_radon_short_params(strip=128)
    import radon_short_ref as S
    assert S.SHORT_DEFAULTS == radon.RadonShortParams().as_dict()


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import radon
    for bad in REFUSED:
        with pytest.raises(ValueError):
            radon.RadonShortParams(**bad).validate(bin=1)
        with pytest.raises(ValueError):
            radon.as_short_params(bad, bin=1)
    for good in TAKEN:
        assert radon.as_short_params(good, bin=1) == good
        radon.RadonShortParams(**good).validate(1)
    assert radon.as_short_params(None) == {}
    radon.RadonShortParams(min_seg=128).validate(bin=2)              # min_strip * bin * bin / 2
    with pytest.raises(ValueError):
        radon.RadonShortParams(min_seg=129).validate(bin=2)
    radon.RadonShortParams(min_seg=129).validate()                  # without a handle's bin only the lower bound is known
    with pytest.raises(ValueError):
        radon.RadonShortParams(max_lines=2.5).validate()
    with pytest.raises(TypeError):
        radon.as_short_params({"threshold": 3})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.RADON_SHORT_DTYPE)
    nl = np.zeros(1, np.int32)
    rc = _native.lib().lfdmi_radon_search_short(None, None, None, 0, 0, 0, None, None, _native._ptr(res), _native._ptr(nl), None)
    assert rc == _native.ERR_ARG


def test_short_rows_round_trip(tmp_path):
    from lfd_amd import radon
    rec = {"level": 128, "strip": 3, "snr": np.float32(9.25), "n_pix": 400, "ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7, "ey2": -2.5,
           "seg_snr": np.float32(12.3), "seg_n_pix": 321}
    row = radon.format_short_row((94, 1, "r", 101), 1, rec)
    assert row.split()[:7] == ["94", "1", "r", "101", "1", "128", "3"] and len(row.split()) == len(radon.SHORT_COLUMNS)
    p = tmp_path / "radon_short.txt"
    p.write_text(row + "\n\n")
    got, = radon.read_short(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "line": 1, "level": 128, "strip": 3, "snr": 9.25,
                   "n_pix": 400, "ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7, "ey2": -2.5, "seg_snr": float(np.float32(12.3)),
                   "seg_n_pix": 321}


def test_dropin_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd import radon
    from lfd_amd.detecttrails import DetectTrails
    with pytest.raises(ValueError):                                   # a mode of the faint-trail search
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon_short=True)
    for bad in ({"min_strip": 96}, {"min_seg": 129}, {"short_threshold": 0.0}, {"max_lines": 9}):
        with pytest.raises(ValueError):
            DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_short=bad)
    with pytest.raises(TypeError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_short={"strip": 64})
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_short=True)
    assert dt.radon_short == {} and dt.radon_short_file == os.path.join(str(tmp_path), "radon_short.txt")
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_short={"min_seg": 128},
                      radon_profiles=True)                            # bin 2: min_seg up to 128; profiles without radon_lines
    assert dt.radon_short == {"min_seg": 128}
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, radon_short=radon.RadonShortParams(max_lines=2))
    assert dt.radon_short["max_lines"] == 2 and DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path)).radon_short is None
