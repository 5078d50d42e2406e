"""lfdmi_radon_null_scheme as Python sees it, without a GPU: the exported symbol and its arguments, lfdmi_radon_peel against the
header, the scheme constants, and the Python side (``lfd_amd.radon``: ``peel_from_lines``, ``shift_scheme_for``, the checks of
``null_peaks`` and ``null_rounds`` before the device, the rows of radon_null_rounds.txt, the arguments of ``DetectTrails``)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_schemes_ref as NS  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402


def header_text():
    with open(os.path.join(ROOT, "include", "lfdmi.h")) as f:
        return f.read()


def test_symbol_is_declared_and_exported():
    from lfd_amd import _native
    assert "lfdmi_radon_null_scheme" in _native.SYMBOLS
    lib = _native.lib()
    assert getattr(lib, "lfdmi_radon_null_scheme") is not None and len(lib.lfdmi_radon_null_scheme.argtypes) == 15
    m = re.search(r"int lfdmi_radon_null_scheme\(([^;]*)\);", header_text())
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ctx", "radon", "frames", "dtype", "n", "loc", "sigma", "seeds", "K", "kind", "kind_params", "scheme", "peel", "n_peel",
                     "records"]
    assert len(lib.lfdmi_radon_null.argtypes) == 12                                    # the old entry point is what it was


def test_peel_struct_and_scheme_constants():
    from lfd_amd import _native as N
    from lfd_amd import radon
    assert header_struct("lfdmi_radon_peel") == list(N.RADON_PEEL_DTYPE.names) == ["q", "y0", "s", "width"]
    assert N.RADON_PEEL_DTYPE.itemsize == C.sizeof(N.RadonPeel) == 16
    for k in N.RADON_PEEL_DTYPE.names:
        assert getattr(N.RadonPeel, k).offset == N.RADON_PEEL_DTYPE.fields[k][1] and getattr(N.RadonPeel, k).size == 4
    text = header_text()
    assert re.search(r"LFDMI_RADON_NULL_SCRAMBLE = 0, LFDMI_RADON_NULL_SIGNFLIP = 1, LFDMI_RADON_NULL_ROWSHIFT = 2, LFDMI_RADON_NULL_COLSHIFT = 3", text)
    assert (N.RADON_NULL_SCRAMBLE, N.RADON_NULL_SIGNFLIP, N.RADON_NULL_ROWSHIFT, N.RADON_NULL_COLSHIFT) == (0, 1, 2, 3)
    assert N.RADON_NULL_SCHEMES == {"scramble": 0, "signflip": 1, "rowshift": 2, "colshift": 3}
    assert tuple(N.RADON_NULL_SCHEMES) == radon.NULL_SCHEMES == NS.SCHEMES and NS.MAX_LINES == N.RADON_MAX_LINES
    assert "tests/radon_null_schemes_ref.py" in text and " 21. Schemes." in text and " 22. Rounds." in text
    # the header states what the sign flip keeps and what each scheme does not do
    assert "M of X' is M of X exactly" in text and text.count("What it does not do") == 3
    assert lib_version_is_pinned()


def lib_version_is_pinned():
    from lfd_amd import _native
    return _native.lib().lfdmi_version() == 300


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.RADON_DTYPE)
    rc = _native.lib().lfdmi_radon_null_scheme(None, None, None, _native.F32, 0, _native.HOST, None, None, 4, 0, None, 1, None, 0, _native._ptr(res))
    assert rc == _native.ERR_ARG and not res.view(np.uint8).any()


def test_peel_from_lines_and_shift_scheme():
    from lfd_amd import _native, radon
    lines = np.zeros((3, 4), _native.RADON_LINE_DTYPE)
    lines["q"], lines["y0"], lines["s"] = [[1, 2, 3, 0]] * 3, [[-5, 6, 7, 8]] * 3, [[9, 10, 11, 12]] * 3
    nl = np.array([0, 2, 4], np.int32)
    peel = radon.peel_from_lines(lines, nl, 3)
    assert peel.dtype == _native.RADON_PEEL_DTYPE and peel.shape == (3, 3)
    assert peel["width"].tolist() == [[0, 0, 0], [1, 1, 0], [1, 1, 1]]
    assert peel[1].tolist() == [(1, -5, 9, 1), (2, 6, 10, 1), (0, 0, 0, 0)] and not peel[0].view(np.int32).any()
    assert [[{k: int(r[k]) for k in r.dtype.names} for r in row] for row in peel] == NS.peel_of(lines, nl, 3)
    wide = np.zeros((3, 4), _native.RADON_WIDE_DTYPE)
    wide["width"] = [[4, 1, 16, 2]] * 3
    assert radon.peel_from_lines(wide, nl, 4)["width"].tolist() == [[0, 0, 0, 0], [4, 1, 0, 0], [4, 1, 16, 2]]
    assert radon.peel_from_lines(lines, nl, 0).shape == (3, 0)
    for bad in (5, -1):
        with pytest.raises(ValueError):
            radon.peel_from_lines(lines, nl, bad)
    with pytest.raises(ValueError):
        radon.peel_from_lines(lines, nl[:2], 1)
    assert [radon.shift_scheme_for(q) for q in range(4)] == ["colshift", "colshift", "rowshift", "rowshift"]
    with pytest.raises(ValueError):
        radon.shift_scheme_for(4)


def test_null_peaks_and_rounds_check_their_arguments_before_the_device():
    from lfd_amd import _native, radon
    f = np.zeros((1, 40, 70), np.float32)
    peel = np.zeros((1, 1), _native.RADON_PEEL_DTYPE)
    with pytest.raises(ValueError):
        radon.null_peaks(None, f, scheme="flip")
    for scheme in ("scramble", "rowshift", "colshift"):
        with pytest.raises(ValueError):
            radon.null_peaks(None, f, scheme=scheme, peel=peel)
    with pytest.raises(ValueError):
        radon.null_peaks(None, f, scheme="signflip", peel_halfwidth=-1)
    with pytest.raises(ValueError):
        radon.null_peaks(None, f, scheme="signflip", min_seg=300)                      # above min_len
    with pytest.raises(TypeError):
        radon.null_peaks(None, f, scheme="signflip", max_width=4)                      # kind "lines" has no such field
    with pytest.raises(TypeError):
        radon.null_peaks(None, f, peel_halfwidth=2)                                    # the scramble's "lines" kind takes none
    lines = np.zeros((1, 2), _native.RADON_LINE_DTYPE)
    with pytest.raises(ValueError):
        radon.null_rounds(None, f, lines, [0], K=0)
    with pytest.raises(ValueError):
        radon.null_rounds(None, f, lines, [0], kind="band")


def test_rounds_rows_round_trip(tmp_path):
    from lfd_amd import radon
    assert radon.NULL_ROUNDS_COLUMNS == ("run", "camcol", "filter", "field", "kind", "round", "K", "null_min", "null_median", "null_max")
    null = np.array([4.5, 5.0, 4.0, 5.5, 4.25], np.float32)
    p = tmp_path / "radon_null_rounds.txt"
    p.write_text(radon.format_null_rounds_row((94, 1, "r", 101), "wide", 2, null) + "\n")
    got, = radon.read_null_rounds(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "kind": "wide", "round": 2, "K": 5, "null_min": 4.0,
                   "null_median": 4.5, "null_max": 5.5}
    # the same numbers as a radon_null.txt row of these peaks
    assert radon.format_null_rounds_row((94, 1, "r", 101), "wide", 2, null).split()[6:] == radon.format_null_row((94, 1, "r", 101), "wide", null).split()[5:]


def test_detecttrails_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    kw = {"run": 94, "camcol": 1, "filter": "r", "savepath": str(tmp_path), "radon": True}
    dt = DetectTrails(radon_null=4, **kw)
    assert dt.radon_null_scheme == "scramble" and dt.radon_null_rounds is False
    dt = DetectTrails(radon_null=4, radon_null_scheme="signflip", radon_null_rounds=True, **kw)
    assert dt.radon_null_scheme == "signflip" and dt.radon_null_rounds is True
    assert dt.radon_null_rounds_file == os.path.join(str(tmp_path), "radon_null_rounds.txt")
    with pytest.raises(ValueError):
        DetectTrails(radon_null=4, radon_null_scheme="flip", **kw)
    for scheme in ("scramble", "rowshift", "colshift"):
        with pytest.raises(ValueError):
            DetectTrails(radon_null=4, radon_null_scheme=scheme, radon_null_rounds=True, **kw)
    with pytest.raises(ValueError):
        DetectTrails(radon_null_scheme="signflip", **kw)                               # needs radon_null
    with pytest.raises(ValueError):
        DetectTrails(radon_null_rounds=True, **kw)
