"""lfdmi_psf_params, lfdmi_psf_star and lfdmi_seeing_frame as Python sees them, without a GPU: the layouts against the header,
the library's defaults, and the rules ``PsfParams.validate`` applies (tests/test_gpu_psf.py holds the library to the same values
on a device: its check sits behind the context)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as R  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402

# what both sides refuse, and what both take
REFUSED = ({"win": 0}, {"win": 17}, {"gap": -1}, {"gap": 9}, {"ring": 0}, {"ring": 9}, {"iso": 0}, {"iso": 65}, {"rad_max": 0},
           {"rad_max": 33}, {"min_stars": 0}, {"min_stars": 1025}, {"max_used": 0}, {"max_used": 1025}, {"k_peak": 0.0},
           {"k_peak": -1.0}, {"k_peak": float("nan")}, {"k_peak": float("inf")}, {"e_max": -0.1}, {"e_max": 1.5},
           {"e_max": float("nan")}, {"sat": 0.0}, {"sat": -1.0}, {"sat": 4096.5}, {"sat": float("nan")}, {"sat": float("inf")})
TAKEN = ({}, {"win": 1}, {"win": 16}, {"gap": 0}, {"gap": 8}, {"ring": 1}, {"ring": 8}, {"iso": 1}, {"iso": 64}, {"rad_max": 1},
         {"rad_max": 32}, {"min_stars": 1}, {"min_stars": 1024}, {"max_used": 1}, {"max_used": 1024}, {"k_peak": 0.5},
         {"e_max": 0.0}, {"e_max": 1.0}, {"sat": 1e-3}, {"sat": 4096.0}, {"win": 16, "gap": 8, "ring": 8})


def test_layouts():
    from lfd_amd import _native
    assert _native.PSF_STAR_DTYPE.itemsize == 64 and _native.SEEING_FRAME_DTYPE.itemsize == 64
    assert list(_native.PSF_STAR_DTYPE.names) == header_struct("lfdmi_psf_star") == list(R.STAR_DTYPE.names)
    assert list(_native.SEEING_FRAME_DTYPE.names) == header_struct("lfdmi_seeing_frame") == list(R.FRAME_DTYPE.names)
    assert _native.PSF_STAR_DTYPE == R.STAR_DTYPE and _native.SEEING_FRAME_DTYPE == R.FRAME_DTYPE
    assert [k for k, _ in _native.PsfParamsStruct._fields_] == header_struct("lfdmi_psf_params") == list(R.DEFAULTS)
    assert C.sizeof(_native.PsfParamsStruct) == 56 and _native.PsfParamsStruct.win.offset == 24
    off = 0
    for dt in (_native.PSF_STAR_DTYPE, _native.SEEING_FRAME_DTYPE):          # no padding but the named one
        off = 0
        for k in dt.names:
            assert dt.fields[k][1] == off, k
            off += dt.fields[k][0].itemsize
        assert off == 64
    assert {"lfdmi_default_psf_params", "lfdmi_measure_seeing"} <= set(_native.SYMBOLS)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert re.search(r"LFDMI_PSF_OK = 0, LFDMI_PSF_NOT_CANDIDATE = 1, LFDMI_PSF_CLIPPED = 2, LFDMI_PSF_CROWDED = 3, LFDMI_PSF_BAD_PIXEL = 4", text)
    assert re.search(r"LFDMI_SEEING_OK = 0, LFDMI_SEEING_FEW = 1", text) and re.search(r"#define LFDMI_PSF_MAX_SAT 4096\.0\b", text)
    assert (_native.PSF_OK, _native.PSF_NOT_CANDIDATE, _native.PSF_CLIPPED, _native.PSF_CROWDED, _native.PSF_BAD_PIXEL) == \
        (R.OK, R.NOT_CANDIDATE, R.CLIPPED, R.CROWDED, R.BAD_PIXEL) == (0, 1, 2, 3, 4)
    assert (_native.SEEING_OK, _native.SEEING_FEW) == (R.SEEING_OK, R.SEEING_FEW) == (0, 1) and _native.PSF_MAX_SAT == R.MAX_SAT == 4096.0
    for name in ("lfdmi_default_psf_params", "lfdmi_measure_seeing"):
        assert re.search(r"\b%s\(" % name, text) and hasattr(_native.lib(), name)


def test_defaults_without_a_gpu():
    from lfd_amd import _native, psf
    p = _native.make_psf_params()
    got = {k: getattr(p, k) for k, _ in _native.PsfParamsStruct._fields_}
    assert got == R.DEFAULTS
    got.pop("pad")
    assert got == psf.PsfParams().as_dict() == psf.default_params().as_dict()
    assert (p.win, p.gap, p.ring, p.iso, p.k_peak, p.rad_max, p.sat, p.e_max, p.min_stars, p.max_used) == \
        (7, 2, 3, 12, 50.0, 16, 4096.0, 0.2, 5, 256)
    assert _native.make_psf_params(win=5).win == 5
    with pytest.raises(TypeError) as e:
        _native.make_psf_params(radius=5)
    assert str(e.value) == "unknown psf parameter 'radius'"


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import psf
    for bad in REFUSED:
        with pytest.raises(ValueError):
            psf.PsfParams(**bad).validate()
        with pytest.raises(ValueError):
            psf.as_params(bad)
    for good in TAKEN:
        assert psf.as_params(good) == good
    assert psf.as_params(None) == {} and psf.as_params(psf.PsfParams(win=2))["win"] == 2
    with pytest.raises(ValueError):
        psf.PsfParams(win=2.5).validate()
    with pytest.raises(TypeError):
        psf.as_params({"radius": 3})
    with pytest.raises(TypeError):
        psf.as_params({"pad": 0})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    rec = np.zeros(4, _native.STAR_DTYPE)
    frec = np.zeros(1, _native.STARS_FRAME_DTYPE)
    out = np.zeros(256, _native.PSF_STAR_DTYPE)
    ofr = np.zeros(1, _native.SEEING_FRAME_DTYPE)
    assert _native.lib().lfdmi_measure_seeing(None, None, _native.F32, 0, 8, 8, _native.HOST, None, _native._ptr(rec), _native.HOST,
                                              _native._ptr(frec), 4, None, _native._ptr(out), _native._ptr(ofr)) == _native.ERR_ARG


def test_rows_read_back(tmp_path):
    from lfd_amd import psf
    fr = np.zeros((), psf.FRAME_DTYPE)
    fr["status"], fr["n_cand"], fr["n_ok"], fr["n_used"] = psf.SEEING_OK, 9, 7, 6
    fr["fwhm_px"], fr["scatter"], fr["ell"] = 3.5, 0.125, 0.0625
    row = psf.format_row((94, 1, "r", 12), fr, 0.396, 1.25)
    assert row == "94 1 r 12 0 9 7 6 3.5 1.3860000000000001 1.25 0.125 0.0625"
    fr["status"], fr["n_used"] = psf.SEEING_FEW, 2
    few = psf.format_row((94, 1, "r", 13), fr, 0.396, float("nan"))
    path = tmp_path / "seeing.txt"
    path.write_text(" ".join(psf.SEEING_COLUMNS) + "\n" + row + "\n" + few + "\n")
    rows = psf.read_seeing(str(path))
    assert len(rows) == 2 and rows[0]["field"] == 12 and rows[0]["filter"] == "r" and rows[0]["seeing_arcsec"] == 1.25
    assert rows[0]["fwhm_arcsec"] == 3.5 * 0.396 and rows[1]["status"] == psf.SEEING_FEW and np.isnan(rows[1]["seeing_arcsec"])
    assert psf.SEEING_COLUMNS == ("run", "camcol", "filter", "field", "status", "n_cand", "n_ok", "n_used", "fwhm_px", "fwhm_arcsec",
                                  "seeing_arcsec", "scatter", "ell")
