"""lfdmi_radon_null as Python sees it, without a GPU: the record types it fills against the header, its constants, the exported
symbol, and the Python side of the null peaks (``lfd_amd.radon``: the false-alarm estimate, the threshold rule, the seed, the
rows of radon_null.txt and radon_fap.txt)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_ref as NR  # noqa: E402
from test_radon_lines_abi import ROOT, header_struct  # noqa: E402


def header_text():
    with open(os.path.join(ROOT, "include", "lfdmi.h")) as f:
        return f.read()


def test_record_types_and_constants():
    from lfd_amd import _native as N
    # the three kinds fill the existing records: their layouts are the header's
    assert list(N.RADON_DTYPE.names) == header_struct("lfdmi_radon_result") and N.RADON_DTYPE.itemsize == C.sizeof(N.RadonResult) == 80
    assert list(N.RADON_SHORT_DTYPE.names) == header_struct("lfdmi_radon_short") and N.RADON_SHORT_DTYPE.itemsize == C.sizeof(N.RadonShort)
    assert list(N.RADON_WIDE_DTYPE.names) == header_struct("lfdmi_radon_wide") and N.RADON_WIDE_DTYPE.itemsize == C.sizeof(N.RadonWide)
    for dt, st in ((N.RADON_DTYPE, N.RadonResult), (N.RADON_SHORT_DTYPE, N.RadonShort), (N.RADON_WIDE_DTYPE, N.RadonWide)):
        for k in dt.names:
            assert getattr(st, k).offset == dt.fields[k][1] and getattr(st, k).size == dt.fields[k][0].itemsize, k
    text = header_text()
    assert re.search(r"LFDMI_RADON_NULL_LINES = 0, LFDMI_RADON_NULL_SHORT = 1, LFDMI_RADON_NULL_WIDE = 2", text)
    assert (N.RADON_NULL_LINES, N.RADON_NULL_SHORT, N.RADON_NULL_WIDE) == (0, 1, 2)
    assert N.RADON_NULL_KINDS == {"lines": 0, "short": 1, "wide": 2} and tuple(N.RADON_NULL_KINDS) == NR.KINDS
    assert re.search(r"#define LFDMI_RADON_NULL_MAX 64\b", text) and N.RADON_NULL_MAX == NR.NULL_MAX == 64
    assert "null peaks" in text and "tests/radon_null_ref.py" in text


def test_symbol_is_declared_and_exported():
    from lfd_amd import _native
    assert "lfdmi_radon_null" in _native.SYMBOLS
    lib = _native.lib()
    assert getattr(lib, "lfdmi_radon_null") is not None and len(lib.lfdmi_radon_null.argtypes) == 12
    m = re.search(r"int lfdmi_radon_null\(([^;]*)\);", header_text())
    assert m and len(m.group(1).split(",")) == 12
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ctx", "radon", "frames", "dtype", "n", "loc", "sigma", "seeds", "K", "kind", "kind_params", "records"]


def test_the_library_refuses_without_a_context():
    from lfd_amd import _native
    res = np.zeros((1, 4), _native.RADON_DTYPE)
    rc = _native.lib().lfdmi_radon_null(None, None, None, _native.F32, 0, _native.HOST, None, None, 4, 0, None, _native._ptr(res))
    assert rc == _native.ERR_ARG


def test_the_restatement_and_the_package_agree_on_the_hash():
    from lfd_amd import radon
    for x in (0, 1, NR.GOLD64, (1 << 64) - 1):
        assert radon._splitmix64(x) == NR.splitmix64(x)


def test_false_alarm_and_threshold():
    from lfd_amd import radon
    null = np.array([4.0, 4.5, 5.0, 5.5] * 4, np.float32)
    assert radon.false_alarm(8.0, null) == 1 / 17                    # above every null peak: exactly 1 / (K + 1), never 0
    assert radon.false_alarm(5.5, null) == 5 / 17                    # a tie counts (>=)
    assert radon.false_alarm(np.float32(3.0), null) == 1.0
    assert radon.null_threshold(null) == 8.25 and radon.null_threshold(null[:2], 1.4) == 1.4 * 4.5
    for bad in ([], np.zeros(0)):
        with pytest.raises(ValueError):
            radon.false_alarm(1.0, bad)
        with pytest.raises(ValueError):
            radon.null_threshold(bad)


def test_seed_is_a_fixed_mix():
    from lfd_amd import radon
    got = {radon.null_seed(run, cc, f, fld) for run in (94, 95) for cc in (1, 2) for f in "ugriz" for fld in (11, 12)}
    assert len(got) == 40 and all(0 <= s < 1 << 64 for s in got)
    assert radon.null_seed(94, 1, "r", 101) == radon.null_seed(94, 1, 2, 101)
    assert radon.null_seed(94, 1, "u", 0) != radon.null_seed(0, 94, "u", 1)
    # the four values go through splitmix64 in turn
    x = 0
    for v in (94, 1, 2, 101):
        x = NR.splitmix64(x ^ v)
    assert radon.null_seed(94, 1, "r", 101) == x


def test_rows_round_trip(tmp_path):
    from lfd_amd import radon
    assert radon.NULL_COLUMNS == ("run", "camcol", "filter", "field", "kind", "K", "null_min", "null_median", "null_max")
    assert radon.FAP_COLUMNS == ("run", "camcol", "filter", "field", "kind", "line", "snr", "n_ge", "K", "fap")
    null = np.array([4.5, 5.0, 4.0, 5.5, 4.25], np.float32)
    meta = (94, 1, "r", 101)
    p = tmp_path / "radon_null.txt"
    p.write_text(radon.format_null_row(meta, "short", null) + "\n\n")
    got, = radon.read_null(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "kind": "short", "K": 5, "null_min": 4.0, "null_median": 4.5,
                   "null_max": 5.5}
    p = tmp_path / "radon_fap.txt"
    p.write_text(radon.format_fap_row(meta, "lines", 0, np.float32(9.5), null) + "\n" + radon.format_fap_row(meta, "lines", 1, 4.5, null) + "\n")
    a, b = radon.read_fap(p)
    assert a == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "kind": "lines", "line": 0, "snr": 9.5, "n_ge": 0, "K": 5, "fap": 1 / 6}
    assert (b["line"], b["n_ge"], b["fap"]) == (1, 3, 4 / 6)


def test_null_peaks_checks_its_arguments_before_the_device():
    from lfd_amd import radon
    f = np.zeros((1, 40, 70), np.float32)
    for kw in ({"kind": "band"}, {"K": 0}, {"K": 65}):
        with pytest.raises(ValueError):
            radon.null_peaks(None, f, **kw)
    with pytest.raises(ValueError):
        radon.null_peaks(None, f, kind="wide", max_width=3)
    with pytest.raises(TypeError):
        radon.null_peaks(None, f, kind="lines", max_width=4)          # a wide parameter is no field of RadonParams


def test_arguments_are_checked_at_construction(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    kw = {"run": 94, "camcol": 1, "filter": "r", "savepath": str(tmp_path)}
    with pytest.raises(ValueError):
        DetectTrails(radon_null=4, **kw)                                   # needs radon=True
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            DetectTrails(radon=True, radon_null=bad, **kw)
    dt = DetectTrails(radon=True, radon_null=8, **kw)
    assert dt.radon_null == 8 and dt.radon_null_file == os.path.join(str(tmp_path), "radon_null.txt")
    assert dt.radon_fap_file == os.path.join(str(tmp_path), "radon_fap.txt") and DetectTrails(**kw).radon_null is None


def test_recovery_table_gets_the_median_false_alarm():
    from lfd_amd import recovery as RC
    rows = np.zeros(5, RC.ROW_DTYPE)
    rows["peak"] = [0.1, 0.1, 0.1, 0.2, 0.2]
    rows["matched"] = [1, 0, 1, 0, 0]
    fap = [0.2, 0.9, 0.4, 0.5, 0.6]
    edges = RC.peak_edges([0.1, 0.2])
    t = RC.completeness(rows, edges, fap=fap)
    assert t[0]["median_fap"] == 0.30000000000000004 and np.isnan(t[1]["median_fap"]) and t[0]["recovered"] == 2   # recovered trails only
    assert "median_fap" not in RC.completeness(rows, edges)[0]
    head = RC.format_table(t).splitlines()[0].split()
    assert head[-1] == "median_fap" and RC.format_table(RC.completeness(rows, edges)).splitlines()[0].split()[-1] == "wilson_hi"
    assert RC.format_table(t).splitlines()[1].split()[-1] == "0.3000"
    with pytest.raises(ValueError):
        RC.run(None, np.zeros((1, 8, 8), np.float32), None, None, rows[:0], None, 1.0, null=4)    # the detector has no null
    with pytest.raises(SystemExit):
        RC.main(["--synth", "0:1", "--peaks", "0.1", "--out", "x", "--null", "4"])
