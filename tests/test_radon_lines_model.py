"""The several-lines search on the CPU (include/lfdmi.h: faint-trail search, steps 7 - 9): the dyadic path against the
transform, the numpy restatement (tests/radon_lines_ref.py) against radon_ref for its first record, two trails per frame found by
peeling, and the extent of a trail that crosses only part of the frame."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import test_radon_model as TM  # noqa: E402

TWO_PAIRS = ((115, 20), (60, 95), (3, 170), (45, 135))       # theta of the two trails' normals in degrees
TWO_PEAKS = (0.02, 0.015)
TWO_CASES = [(k, 2) for k in range(4)] + [(0, 1), (3, 1)]    # (pair, bin)
PART_PEAK = 0.03
# the largest end-point error along the line of the restatement's segment over the 16 partial trails (bin 1: 19.3 px, bin 2:
# 16.0 px), times 1.5 for another seed
PART_TOL = {1: 1.5 * 19.33, 2: 1.5 * 15.98}


@functools.lru_cache(maxsize=None)
def two_trail_plan(k):
    """INJECT records of the two full-crossing trails of frame k (frame index 0): peaks 0.02 and 0.015"""
    h, w = TM.SET_SHAPE
    tr = np.zeros(2, IR.TRAIL_DTYPE)
    for i, (deg, peak) in enumerate(zip(TWO_PAIRS[k], TWO_PEAKS)):
        th = math.radians(deg)
        x0, y0 = w / 2 + 7 * i - 10, h / 2 - 5 * i + 4
        tr[i] = (0, 0, x0 * math.cos(th) + y0 * math.sin(th), th, -np.inf, np.inf, peak)
    return tr


@functools.lru_cache(maxsize=None)
def two_trail_noise(k):
    f = np.random.default_rng(100 + k).normal(0, TM.SET_SIGMA, (1, *TM.SET_SHAPE)).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def two_trail_frame(k):
    _, table, step = TM.trail_plan()
    f = IR.inject(two_trail_noise(k).copy(), two_trail_plan(k), table, step)[0]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def two_trail_lines(k, b, halfwidth=8):
    """the restatement's (records, n_lines) of two-trail frame k at bin b, computed once"""
    return L.search_lines(two_trail_frame(k), TM.SET_SIGMA, peel_halfwidth=halfwidth, bin=b)


@functools.lru_cache(maxsize=None)
def set_lines(kind, b):
    """the restatement's (records, n_lines) per frame of test_radon_model's noise set (at the defaults) or trail set (one round:
    max_lines = 1)"""
    if kind == "noise":
        return tuple(L.search_lines(f, TM.SET_SIGMA, bin=b) for f in TM.noise_frames())
    return tuple(L.search_lines(f, TM.SET_SIGMA, max_lines=1, bin=b) for f in TM.trail_frames())


@functools.lru_cache(maxsize=None)
def partial_plan():
    """test_radon_model's 16 trails at peak 0.03 over the middle half of their crossing"""
    from lfd_amd import recovery
    tr = TM.trail_plan()[0].copy()
    tr["amplitude"] = PART_PEAK
    for i in range(len(tr)):
        ta, tb = recovery.extent(float(tr["rho"][i]), float(tr["theta"][i]), -np.inf, np.inf, TM.SET_SHAPE)
        tr["t0"][i], tr["t1"][i] = ta + (tb - ta) / 4, tb - (tb - ta) / 4
    return tr


@pytest.mark.parametrize("shape", [(9, 16), (5, 3)])
def test_sum_along_the_dyadic_path_is_the_transform(shape):
    from lfd_amd import radon
    Q = np.random.default_rng(shape[0]).integers(-9, 10, shape).astype(np.int64)
    S = R.transform(Q)
    Rr, C = shape
    P = R.pow2_at_least(C)
    cols = np.arange(C)
    for s in range(P):
        d = radon.dyadic_path(s, P)
        assert d.shape == (P,) and d[0] == 0 and d[P - 1] == s and np.array_equal(d, L.dyadic_path(s, P))
        for yi in range(Rr + P - 1):
            rows = yi - (P - 1) + d[:C]
            ok = (rows >= 0) & (rows < Rr)
            assert S[yi, s] == Q[rows[ok], cols[ok]].sum(), (yi, s)
    for bad in ((0, 3), (4, 4), (-1, 4), (0, 0)):
        with pytest.raises(ValueError):
            radon.dyadic_path(*bad)


@pytest.mark.parametrize("b", [1, 2])
def test_record_0_is_the_plain_search_and_noise_gives_no_line(b):
    for kind in ("noise", "trail"):
        for (recs, n_lines), ref in zip(set_lines(kind, b), TM.set_records(kind, b)):
            for key, want in ref.items():
                got = recs[0][key]
                assert type(got) is type(want) and (got == want or key in ("sum", "snr") and got.tobytes() == want.tobytes()), key
            assert n_lines == (kind == "trail")
    for recs, _ in set_lines("noise", b):
        assert recs[0]["found"] == 0 and recs[0]["c2"] == 0 and all(r == L.ZERO for r in recs[1:])


@pytest.mark.parametrize("k,b", TWO_CASES)
def test_two_trails_are_found_by_peeling(k, b):
    recs, n_lines = two_trail_lines(k, b)
    tr = two_trail_plan(k)
    print("pair", TWO_PAIRS[k], "bin", b, "snr", ["%.2f" % float(r["snr"]) for r in recs])
    assert n_lines == 2
    matched = set()
    for r in recs[:2]:
        errs = [TM.line_error(r, t, TM.SET_SHAPE) for t in tr]
        hit = [i for i, (a, d) in enumerate(errs) if a <= 0.5 and d <= 4.0]
        assert len(hit) == 1, errs
        matched.add(hit[0])
        assert r["found"] == 1 and r["seg_n_pix"] >= 64 and 0 <= r["c1"] <= r["c2"]
    assert matched == {0, 1}
    stop = recs[2]
    assert stop["status"] == R.OK and stop["found"] == 0 and float(stop["snr"]) < 8.0 and stop["c2"] == 0
    assert recs[3] == L.ZERO


def along(x, y, theta):
    return -x * math.sin(theta) + y * math.cos(theta)


@pytest.mark.parametrize("b", [1, 2])
def test_segment_of_a_partial_trail_ends_where_the_trail_does(b):
    tr = partial_plan()
    _, table, step = TM.trail_plan()
    frames = IR.inject(TM.noise_frames().copy(), tr, table, step)
    errs = []
    for i, f in enumerate(frames):
        recs, n_lines = L.search_lines(f, TM.SET_SIGMA, max_lines=1, bin=b)
        assert n_lines == 1
        r, th = recs[0], float(tr["theta"][i])
        lo, hi = sorted((along(r["ex1"], r["ey1"], th), along(r["ex2"], r["ey2"], th)))
        errs.append(max(abs(lo - tr["t0"][i]), abs(hi - tr["t1"][i])))
    print("bin", b, "end-point errors along the line (px)", ["%.1f" % e for e in errs])
    assert max(errs) <= PART_TOL[b]


@pytest.mark.parametrize("b", [1, 2])
def test_segment_of_a_full_crossing_covers_it(b):
    cover = []
    for f, (recs, n_lines) in zip(TM.trail_frames(), set_lines("trail", b)):
        r = recs[0]
        V, M = R.prepare(f, b, R.DEFAULTS["clip"])
        rows, Rr, C = L.line_rows(V, r["q"], r["y0"], r["s"])
        ok = (rows >= 0) & (rows < Rr)
        m = np.zeros(C, np.int64)
        m[ok] = R.orient(M, r["q"])[rows[ok], np.arange(C)[ok]]
        assert m.sum() == r["n_pix"] and m[r["c1"]:r["c2"] + 1].sum() == r["seg_n_pix"]
        cover.append((m[r["c1"]:r["c2"] + 1] > 0).sum() / (m > 0).sum())
    print("bin", b, "covered share of the columns with valid pixels", ["%.2f" % c for c in cover])
    assert min(cover) >= 0.9


def test_segment_points_agree_with_the_restatement():
    from lfd_amd import radon
    for shape, b in (((37, 50), 1), ((97, 161), 4), ((300, 70), 2)):
        hb, wb, p01, p23 = radon.working_dims(shape, b)
        for q in range(4):
            P, C = (p01, wb) if q < 2 else (p23, hb)
            for y0, s, c1, c2 in ((0, 0, 0, C - 1), (-3, P - 1, 1, C - 2), (5, P // 3, C // 2, C // 2)):
                d = L.dyadic_path(s, P)
                want = L.point_of(q, c1, y0 + int(d[c1]), shape, b) + L.point_of(q, c2, y0 + int(d[c2]), shape, b)
                assert radon.segment_points(q, y0, s, c1, c2, shape, b) == want
            # the ends of the full path are the record's line: (0, y0) and (P-1, y0 + s)
            if C == P:
                x1, y1, x2, y2, _, _ = radon.line_of(q, 2, 7, shape, b)
                assert radon.segment_points(q, 2, 7, 0, C - 1, shape, b) == (x1, y1, x2, y2)
    with pytest.raises(ValueError):
        radon.segment_points(0, 0, 0, 3, 2, (37, 50), 1)
    with pytest.raises(ValueError):
        radon.segment_points(0, 0, 0, 0, 50, (37, 50), 1)


def test_segment_rows_round_trip(tmp_path):
    from lfd_amd import radon
    rec = {"ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7, "ey2": -2.5, "seg_snr": np.float32(12.3), "seg_n_pix": 321}
    row = radon.format_segment_row((94, 1, "r", 101), 1, rec)
    assert row.split()[:5] == ["94", "1", "r", "101", "1"] and len(row.split()) == len(radon.SEGMENT_COLUMNS)
    p = tmp_path / "radon_segments.txt"
    p.write_text(row + "\n\n")
    got, = radon.read_segments(p)
    assert got == {"run": 94, "camcol": 1, "filter": "r", "field": 101, "line": 1, "ex1": 0.5, "ey1": 1.0 / 3, "ex2": 1e-7,
                   "ey2": -2.5, "seg_snr": float(np.float32(12.3)), "seg_n_pix": 321}
