"""lfdmi_preview_params and lfdmi_preview_frame as _native sees them: sizes, offsets, defaults; the stretch tables; the image
checker's file names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402

from lfd_amd import _native, previews  # noqa: E402


def test_the_layouts_agree():
    S = _native.PreviewParamsStruct
    assert C.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("bin", 0), ("mode", 4), ("lo_ppm", 8), ("hi_ppm", 12)]
    D = _native.PREVIEW_FRAME_DTYPE
    assert D.itemsize == 48 and D == R.FRAME_DTYPE == previews.FRAME_DTYPE
    assert [D.fields[k][1] for k in D.names] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert (_native.PREVIEW_OK, _native.PREVIEW_FLAT, _native.PREVIEW_EMPTY) == (R.OK, R.FLAT, R.EMPTY) == (0, 1, 2)
    assert (_native.PREVIEW_RANK, _native.PREVIEW_GIVEN) == (R.RANK, R.GIVEN) == (0, 1)
    assert _native.PREVIEW_LUT == R.LUT == 4096 and _native.PREVIEW_BINS == R.BINS
    assert _native.PREVIEW_EMPTY_CELL == R.EMPTY_CELL == np.iinfo(np.int64).min


def test_the_defaults():
    p = _native.make_preview_params()
    assert {k: getattr(p, k) for k, _ in p._fields_} == R.DEFAULTS == {"bin": 4, "mode": 0, "lo_ppm": 10000, "hi_ppm": 995000}
    p = _native.make_preview_params(bin=8, mode="given")
    assert (p.bin, p.mode, p.lo_ppm) == (8, 1, 10000)
    with pytest.raises(TypeError) as e:
        _native.make_preview_params(no_such_field=1)
    assert str(e.value) == "unknown preview parameter 'no_such_field'"
    with pytest.raises(ValueError):
        _native.make_preview_params(mode="median")
    with pytest.raises(ValueError):
        previews.as_params({"bin": 3})
    with pytest.raises(ValueError):
        previews.as_params({"lo_ppm": 7, "hi_ppm": 6})
    with pytest.raises(TypeError):
        previews.as_params({"binning": 4})
    assert previews.as_params(None) == {}


def test_the_header_declares_what_is_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lfdmi.h")).read()
    assert "int lfdmi_frame_previews(" in text and "void lfdmi_default_preview_params(" in text
    assert "lfdmi_frame_previews" in _native.SYMBOLS and "lfdmi_default_preview_params" in _native.SYMBOLS


@pytest.mark.parametrize("kind", previews.LUT_KINDS)
def test_stretch_tables(kind):
    t = previews.lut(kind)
    assert t.dtype == np.uint8 and t.shape == (4096,) and t[0] == 0 and t[-1] == 255
    assert (np.diff(t.astype(int)) >= 0).all()
    if kind == "linear":
        assert t[2048] == 128 and t[1024] == 64
    if kind == "asinh":
        assert t[409] == 75          # 255 asinh(1) / asinh(10): a tenth of the range gets 29 % of the bytes, linear gives it 10 %
        assert np.abs(previews.lut("asinh", softening=1e3).astype(int) - previews.lut("linear").astype(int)).max() <= 1
    with pytest.raises(ValueError):
        previews.lut("log")
    with pytest.raises(ValueError):
        previews.lut("asinh", softening=0.0)


def test_filename_round_trip():
    # the image checker's format, restated literally
    for run, camcol, filt, field in [(94, 1, "r", 12), (2888, 6, "z", 139), (1, 3, "u", 1), (123456, 2, "g", 1000), (7, 1, "i", 12345)]:
        name = previews.filename(run, camcol, filt, field)
        assert name == f"frame-{filt}-{run:06d}-{camcol}-{field:04}.fits.png"
        assert previews.parse_filename(name) == (run, camcol, filt, field, "fits.png")
        assert previews.parse_filename(os.path.join("some", "dir", name)) == (run, camcol, filt, field, "fits.png")
    assert previews.filename(94, 1, "r", 12) == "frame-r-000094-1-0012.fits.png"
    assert previews.filename(94, 1, "r", 12, ext="png") == "frame-r-000094-1-0012.png"
    assert previews.parse_filename("frame-r-000094-1-0012.png")[4] == "png"
    for bad in ("frame-r-94-1-0012.fits.png", "strip-r-000094-1-0012.png", "frame-r-000094-1-12.fits.png"):
        with pytest.raises(ValueError):
            previews.parse_filename(bad)


def test_previews_txt_round_trip(tmp_path):
    rec = np.zeros(1, previews.FRAME_DTYPE)[0]
    rec["status"], rec["n_cells"], rec["n_empty"], rec["lo_f"], rec["hi_f"] = 0, 190000, 464, -0.0123, 0.25
    path = tmp_path / "previews.txt"
    with open(path, "w") as f:
        f.write(" ".join(previews.PREVIEW_COLUMNS) + "\n")
        f.write(previews.format_row((94, 1, "r", 12), 4, rec, previews.filename(94, 1, "r", 12)) + "\n")
    (row,) = previews.read_previews(path)
    assert tuple(row) == previews.PREVIEW_COLUMNS
    assert row == {"run": 94, "camcol": 1, "filter": "r", "field": 12, "status": 0, "bin": 4, "lo": -0.0123, "hi": 0.25,
                   "n_cells": 190000, "n_empty": 464, "file": "frame-r-000094-1-0012.fits.png"}
