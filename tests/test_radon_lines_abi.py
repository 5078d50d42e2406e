"""lfdmi_radon_line and lfdmi_radon_lines_params as Python sees them, without a GPU: the record's layout against the header, the
library's defaults, and the rules ``RadonLinesParams.validate`` applies (tests/test_gpu_radon_lines.py holds the library to the
same values on a device: its check sits behind the context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what both sides refuse, and what both take, with a handle of min_len = 256
REFUSED = ({"max_lines": 0}, {"max_lines": 9}, {"peel_halfwidth": -1}, {"min_seg": 0}, {"min_seg": 257})
TAKEN = ({}, {"max_lines": 1}, {"max_lines": 8}, {"peel_halfwidth": 0}, {"min_seg": 1}, {"min_seg": 256})


def header_struct(name):
    """the field names of ``typedef struct { ... } name;`` in include/lfdmi.h, in order"""
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    return names


def test_record_layout():
    from lfd_amd import _native
    assert C.sizeof(_native.RadonLine) == _native.RADON_LINE_DTYPE.itemsize == 136
    names = [k for k, _ in _native.RadonLine._fields_]
    assert names == list(_native.RADON_LINE_DTYPE.names) == header_struct("lfdmi_radon_line")
    assert names[:len(_native.RADON_DTYPE.names)] == list(_native.RADON_DTYPE.names)      # lfdmi_radon_result comes first
    for k in names:
        assert getattr(_native.RadonLine, k).offset == _native.RADON_LINE_DTYPE.fields[k][1], k
        assert getattr(_native.RadonLine, k).size == _native.RADON_LINE_DTYPE.fields[k][0].itemsize, k
    assert [k for k, _ in _native.RadonLinesParamsStruct._fields_] == header_struct("lfdmi_radon_lines_params")
    assert C.sizeof(_native.RadonLinesParamsStruct) == 12
    assert {"lfdmi_default_radon_lines_params", "lfdmi_radon_search_lines"} <= set(_native.SYMBOLS)


def test_defaults_without_a_gpu():
    from lfd_amd import _native, radon
    p = _native.make_radon_lines_params()
    assert (p.max_lines, p.peel_halfwidth, p.min_seg) == (4, 8, 64)
    assert radon.default_lines_params() == radon.RadonLinesParams() == radon.RadonLinesParams(4, 8, 64)
    assert _native.make_radon_lines_params(max_lines=2).max_lines == 2
    with pytest.raises(TypeError):
        _native.make_radon_lines_params(lines=2)
    assert _native.RADON_MAX_LINES == 8
    text = open(os.path.join(ROOT, "include", "lfdmi.h")).read()
    assert re.search(r"#define LFDMI_RADON_MAX_LINES 8\b", text)


def test_validate_refuses_what_the_library_refuses():
    from lfd_amd import radon
    for bad in REFUSED:
        with pytest.raises(ValueError):
            radon.RadonLinesParams(**bad).validate(min_len=256)
        with pytest.raises(ValueError):
            radon.as_lines_params(bad, min_len=256)
    for good in TAKEN:
        assert radon.as_lines_params(good, min_len=256) == good
        radon.RadonLinesParams(**good).validate(256)
    assert radon.as_lines_params(None) == {}
    radon.RadonLinesParams(min_seg=257).validate()                  # without a handle's min_len only the lower bound is known
    with pytest.raises(ValueError):
        radon.RadonLinesParams(max_lines=2.5).validate()
    with pytest.raises(TypeError):
        radon.as_lines_params({"halfwidth": 3})


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.RADON_LINE_DTYPE)
    nl = np.zeros(1, np.int32)
    rc = _native.lib().lfdmi_radon_search_lines(None, None, None, 0, 0, 0, None, None, _native._ptr(res), _native._ptr(nl))
    assert rc == _native.ERR_ARG


def test_dropin_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    for bad in ({"radon_lines": 0}, {"radon_lines": 9}, {"radon_lines": 2, "radon_lines_params": {"peel_halfwidth": -1}},
                {"radon_lines": 2, "radon_lines_params": {"min_seg": 300}}):
        with pytest.raises(ValueError):
            DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True, **bad)
