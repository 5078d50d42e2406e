"""lfdmi_star, lfdmi_stars_frame and lfdmi_stars_params as Python sees them, without a GPU: the layouts against the header, the
library's defaults, and the rules ``StarsParams.validate`` applies (tests/test_gpu_stars.py holds the library to the same values
on a device: its check sits behind the context)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402

# what both sides refuse, and what both take
REFUSED = ({"k_det": 0.0}, {"k_det": -1.0}, {"k_det": float("nan")}, {"k_det": float("inf")}, {"k_edge": 0.0}, {"edge_frac": -0.1},
           {"edge_frac": 1.5}, {"edge_frac": float("nan")}, {"sep": 0}, {"sep": 9}, {"r_max": 0}, {"r_max": 33}, {"max_obj": 0},
           {"max_obj": (1 << 20) + 1})
TAKEN = ({}, {"k_det": 0.5}, {"k_edge": 10.0}, {"edge_frac": 0.0}, {"edge_frac": 1.0}, {"sep": 1}, {"sep": 8}, {"r_max": 1},
         {"r_max": 32}, {"max_obj": 1}, {"max_obj": 1 << 20})


def test_layouts():
    from lfd_amd import _native
    assert _native.STAR_DTYPE.itemsize == 32 and _native.STARS_FRAME_DTYPE.itemsize == 12
    assert list(_native.STAR_DTYPE.names) == header_struct("lfdmi_star") == list(R.FIELDS)
    assert _native.STAR_DTYPE == R.STAR_DTYPE and _native.STARS_FRAME_DTYPE == R.FRAME_DTYPE
    assert list(_native.STARS_FRAME_DTYPE.names) == header_struct("lfdmi_stars_frame")
    assert [k for k, _ in _native.StarsParamsStruct._fields_] == header_struct("lfdmi_stars_params")
    assert C.sizeof(_native.StarsParamsStruct) == 40 and _native.StarsParamsStruct.sep.offset == 24
    off = 0
    for k in _native.STAR_DTYPE.names:                    # no padding: four int32, four float32
        assert _native.STAR_DTYPE.fields[k][1] == off, k
        off += 4
    assert {"lfdmi_default_stars_params", "lfdmi_find_stars", "lfdmi_stars_catalog"} <= set(_native.SYMBOLS)
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert re.search(r"#define LFDMI_STARS_MAX_OBJ 1048576\b", text) and _native.STARS_MAX_OBJ == 1 << 20
    assert re.search(r"LFDMI_STARS_OK = 0, LFDMI_STARS_TRUNCATED = 1", text) and re.search(r"LFDMI_STAR_EXTENDED = 1, LFDMI_STAR_EDGE = 2", text)
    assert (_native.STARS_OK, _native.STARS_TRUNCATED, _native.STAR_EXTENDED, _native.STAR_EDGE) == (R.OK, R.TRUNCATED, R.EXTENDED, R.EDGE) == (0, 1, 1, 2)
    assert _native.lib().lfdmi_version() == 300
    for name in ("lfdmi_default_stars_params", "lfdmi_find_stars", "lfdmi_stars_catalog"):
        assert re.search(r"\b%s\(" % name, text) and hasattr(_native.lib(), name)


def test_defaults_without_a_gpu():
    from lfd_amd import _native, stars
    p = _native.make_stars_params()
    got = {k: getattr(p, k) for k, _ in _native.StarsParamsStruct._fields_}
    assert got == R.DEFAULTS == stars.StarsParams().as_dict() == stars.default_params().as_dict()
    assert (p.k_det, p.k_edge, p.edge_frac, p.sep, p.r_max, p.max_obj) == (5.0, 3.0, 0.02, 3, 32, 4096)
    assert _native.make_stars_params(sep=5).sep == 5
    with pytest.raises(TypeError):
        _native.make_stars_params(radius=5)


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import stars
    for bad in REFUSED:
        with pytest.raises(ValueError):
            stars.StarsParams(**bad).validate()
        with pytest.raises(ValueError):
            stars.as_params(bad)
    for good in TAKEN:
        assert stars.as_params(good) == good
    assert stars.as_params(None) == {} and stars.as_params(stars.StarsParams(sep=2))["sep"] == 2
    with pytest.raises(ValueError):
        stars.StarsParams(sep=2.5).validate()
    with pytest.raises(TypeError):
        stars.as_params({"radius": 3})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    rec = np.zeros(4, _native.STAR_DTYPE)
    frec = np.zeros(1, _native.STARS_FRAME_DTYPE)
    assert _native.lib().lfdmi_find_stars(None, None, _native.F32, 0, 8, 8, _native.HOST, None, None, _native._ptr(rec), _native.HOST,
                                          _native._ptr(frec)) == _native.ERR_ARG
    assert _native.lib().lfdmi_stars_catalog(None, _native._ptr(rec), _native.HOST, _native._ptr(frec), 1, 4, 0.396, None) == _native.ERR_ARG


def test_host_catalogue_and_rows():
    """``stars.to_catalog`` is the restatement's step 8, and a stars.txt row reads back"""
    from lfd_amd import stars
    rec = np.zeros((2, 3), R.STAR_DTYPE)
    rec[0, 0] = (5, 7, 4, 0, 1.0, 2.0, 5.25, 7.5)
    rec[0, 1] = (9, 1, 0, R.EXTENDED, 1.0, 2.0, 9.0, 1.0)
    rec[1, 0] = (0, 0, 32, R.EDGE, 1.0, 2.0, 0.0, 0.0)
    frec = np.zeros(2, R.FRAME_DTYPE)
    frec["n_found"], frec["n_out"] = [2, 5], [2, 1]
    frec["status"] = [R.OK, R.OK]
    a, b = stars.to_catalog(rec, frec, 0.396), R.to_catalog(rec, frec, 0.396)
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert a["COLC"][0, 0].tolist() == [7.0] * 5 and a["ROWC"][0, 0].tolist() == [5.0] * 5
    assert a["PETROTH90"][1, 0, 2] == np.float32(32 * 0.396) and a["NOBSERVE"].tolist() == [[1, 0, 0], [1, 0, 0]]
    assert a["NDETECT"].tolist() == [[1, 1, 1]] * 2 and a["count"].tolist() == [2, 1]
    assert stars.n_extended(rec, frec).tolist() == [1, 0]
    row = stars.format_row((94, 1, "r", 12), frec[0], 1)
    assert row == "94 1 r 12 0 2 2 1"


def test_dropin_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    with pytest.raises(ValueError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), find_stars=True, stars_params={"sep": 9})
    with pytest.raises(TypeError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), find_stars=True, stars_params={"radius": 9})
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), find_stars=True, stars_params={"sep": 2})
    assert dt.find_stars and dt.stars_params == {"sep": 2} and dt.stars_file == os.path.join(str(tmp_path), "stars.txt")
    off = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path))
    assert not off.find_stars and off.stars_params == {}
