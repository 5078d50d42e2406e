"""CPU checks of tests/psf_cases.py: every case holds what it is meant to under the restatement (tests/psf_ref.py), the
restatement's fixed point agrees with exact rational arithmetic on every pixel bit pattern the edge cases place, the largest
sums fit an int64 -- and plain restatements of the kernels' loops (k_psf.h) with one deliberate mistake each give another answer
on the case meant to notice it.  This is what makes the device comparison of tests/test_gpu_psf_edges.py mean something."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import psf_cases as P
import psf_ref as R

INT64_MAX = 2 ** 63 - 1


@functools.lru_cache(maxsize=None)
def statuses(name):
    """the restatement's status of every record of a case (the parameters that cut the packed list do not enter)"""
    c = P.get(name)
    sig = [None] * len(c.frames) if c.sigma is None else c.sigma
    return [R.measure_frame(c.frames[f], c.records[f], c.n_out[f], sig[f], **c.params)[2] for f in range(len(c.frames))]


STATUS_OF = {"long_lists_cut300": "long_lists", "long_lists_cut1": "long_lists"}


@pytest.mark.parametrize("name", P.NAMES)
def test_case_holds_what_it_is_meant_to(name):
    c = P.get(name)
    got = statuses(STATUS_OF.get(name, name))
    n = len(c.frames)
    assert c.frames.dtype == np.float32 and c.frames.ndim == 3 and c.records.shape[0] == n == len(c.frame_records)
    assert all(0 <= v <= c.max_obj for v in c.n_out)
    for (f, i), st in c.status.items():
        assert got[f][i] == st, (name, f, i, c.records[f, i], got[f][i], st)
    if c.every:
        assert len(c.status) == sum(c.n_out)
    out, fr = P.want(name)
    assert [int(v) for v in fr["n_ok"]] == c.n_ok and [int(v) for v in fr["n_packed"]] == c.n_packed
    n_used = c.n_packed if c.n_used == "packed" else c.n_used
    if n_used is not None:
        assert [int(v) for v in fr["n_used"]] == n_used
    for f in range(n):
        ok = [i for i, st in enumerate(got[f]) if st == R.OK]
        assert [int(v) for v in out[f]["index"][:c.n_packed[f]]] == ok[:c.n_packed[f]]
        assert not out[f][c.n_packed[f]:].view(np.uint8).any()
    # the slots past n_out would show if read: garbage in every one
    for f in range(n):
        assert all(c.records[f, k]["flags"] == -1 or c.records[f, k]["s_peak"] == P.PEAK for k in range(c.n_out[f], c.max_obj))
    assert c.max_obj > min(c.n_out)


# ---- long_lists ---------------------------------------------------------------------------------------------------------------

def test_long_lists_reach_every_round_and_stride():
    c = P.get("long_lists")
    n_out = c.n_out
    assert c.max_obj % 4 != 0 and c.max_obj == max(n_out) and 0 in n_out and 65 in n_out and 257 in n_out
    assert any(512 < v < c.max_obj for v in n_out)                                  # three rounds of the pack, beside five
    assert c.frames.shape[1:] == (64, 96) and c.params["max_used"] == 1024
    st = statuses("long_lists")
    for f, n in enumerate(n_out):
        for w0 in range(0, n - 63, 64):                                            # every whole wave of every round
            wave = st[f][w0:w0 + 64]
            first_nc = wave.index(R.NOT_CANDIDATE)
            assert R.OK in wave[first_nc:], (f, w0)                                # an OK record's place differs from its lane
            assert 0 < wave.count(R.OK) < 64
        ok = [i for i in range(n) if st[f][i] == R.OK]
        assert all(rank != i for rank, i in enumerate(ok))
        if n > 256:
            assert st[f][256] == R.OK                                              # the round after the first is not empty of OK records
    assert st[3][64] == R.OK
    assert c.n_ok[0] > 256 and c.n_ok[4] > 256 and max(c.n_ok) <= 1024
    # max_used = 300 cuts inside the second round of the long frames, and not at all in the short ones
    cut = P.get("long_lists_cut300")
    for f in (0, 4):
        ok = [i for i in range(n_out[f]) if st[f][i] == R.OK]
        assert 256 < ok[299] < ok[300] < 511 and cut.n_packed[f] == 300
    assert cut.n_packed[1] == c.n_ok[1] < 300
    one = P.get("long_lists_cut1")
    assert one.n_packed == [1, 1, 0, 1, 1] and [int(v) for v in P.want("long_lists_cut1")[0]["index"][:, 0]] == [1, 1, 0, 1, 1]
    # the shorter lists are the head of the longest packed list
    full, short = P.want("long_lists")[0], P.want("long_lists_cut300")[0]
    assert short.tobytes() == np.ascontiguousarray(full[:, :300]).tobytes()


def pack_rounds(st, max_used, carry=True):
    """k_psf_pack's walk in rounds of 256 records: the records copied out, by place.  carry=False forgets ``done += all``."""
    out, done = {}, 0
    for i0 in range(0, len(st), 256):
        ok = [i for i in range(i0, min(i0 + 256, len(st))) if st[i] == R.OK]
        for k, i in enumerate(ok):
            if done + k < max_used:
                out[done + k] = i
        if carry:
            done += len(ok)
    return [out[k] for k in sorted(out)], done


@pytest.mark.parametrize("name", list(P.LL_CUTS))
def test_pack_rounds_restated(name):
    c = P.get(name)
    out, fr = P.want(name)
    differs = 0
    for f, st in enumerate(statuses("long_lists")):
        idx, done = pack_rounds(st, c.params["max_used"])
        assert idx == [int(v) for v in out[f]["index"][:c.n_packed[f]]] and done == fr["n_ok"][f]
        differs += pack_rounds(st, c.params["max_used"], carry=False) != (idx, done)
    assert differs >= 3                                                            # every frame of more than one round


# ---- crowd_far ----------------------------------------------------------------------------------------------------------------

def crowd_strides(rec, n, i, iso, strides=None):
    """the crowding loop of k_psf_measure: lanes 0 .. 63 over j = lane, lane + 64, ...; ``strides`` stops it early"""
    near = False
    for j0 in range(0, n, 64)[:strides]:
        for j in range(j0, min(j0 + 64, n)):
            if j != i:
                near = near or max(abs(int(rec[j]["x"]) - int(rec[i]["x"])), abs(int(rec[j]["y"]) - int(rec[i]["y"]))) <= iso
    return near


def test_crowd_far_neighbours_sit_where_they_are_meant_to():
    c = P.get("crowd_far")
    rec, n, iso = c.records[0], c.n_out[0], R.DEFAULTS["iso"]
    assert n == 130 and n % 64 != 0 and c.frames.shape[1:] == P.CF_SHAPE

    def near(i):
        return [j for j in range(n) if j != i and max(abs(int(rec[j]["x"]) - int(rec[i]["x"])), abs(int(rec[j]["y"]) - int(rec[i]["y"]))) <= iso]

    assert near(3) == [64] and near(64) == [3] and near(5) == [129] and near(129) == [5]
    assert near(7) == [70] and rec[70]["flags"] != 0 and near(8) == [100] and (rec[8]["x"], rec[8]["y"]) == (rec[100]["x"], rec[100]["y"])
    dist = {i: (int(rec[j]["x"]) - int(rec[i]["x"]), int(rec[j]["y"]) - int(rec[i]["y"])) for i, j, *_ in P.CF_PAIRS}
    assert [dist[i] for i in (10, 11, 12, 13, 14, 15)] == [(12, 0), (13, 0), (0, 12), (0, 13), (12, 12), (13, 13)]
    paired = {i for p in P.CF_PAIRS for i in p[:2]}
    assert all(not near(i) for i in range(n) if i not in paired)
    # every record's square lies in the frame: nothing is clipped ahead of the crowding test
    h, w = P.CF_SHAPE
    assert all(12 <= rec[i]["x"] <= w - 13 and 12 <= rec[i]["y"] <= h - 13 for i in range(n))
    st = statuses("crowd_far")[0]
    full = [R.CROWDED if crowd_strides(rec, n, i, iso) else R.OK for i in range(n)]
    assert all(full[i] == st[i] for i in range(n) if st[i] != R.NOT_CANDIDATE)
    first = [R.CROWDED if crowd_strides(rec, n, i, iso, strides=1) else R.OK for i in range(n)]
    assert first[3] == R.OK and first[5] == R.OK and first != full               # a loop that stops after one stride is noticed


# ---- clipping -----------------------------------------------------------------------------------------------------------------

def clip(x, y, h, w, H, slack=(0, 0, 0, 0)):
    """the clip test of k_psf_measure; ``slack`` loosens one of its four comparisons"""
    return x < H - slack[0] or x > w - 1 - H + slack[1] or y < H - slack[2] or y > h - 1 - H + slack[3]


@pytest.mark.parametrize("name", ["clip_all_sides", "clip_25"])
def test_clip_cases_pin_all_four_comparisons(name):
    c = P.get(name)
    h, w = c.frames.shape[1:]
    H = P.CLIP_H
    recs = [(f, i, int(c.records[f, i]["x"]), int(c.records[f, i]["y"])) for f in range(len(c.frames)) for i in range(c.n_out[f])]
    for f, i, x, y in recs:
        assert clip(x, y, h, w, H) == (c.status[(f, i)] == R.CLIPPED)
    for k in range(4):                                                             # each comparison off by one changes a record
        slack = tuple(int(j == k) for j in range(4))
        assert any(clip(x, y, h, w, H, slack) != clip(x, y, h, w, H) for _, _, x, y in recs), k
        tight = tuple(-int(j == k) for j in range(4))
        assert any(clip(x, y, h, w, H, tight) != clip(x, y, h, w, H) for _, _, x, y in recs), k
    # the last frame holds the bottom-right legal centre as an OK record: its square ends on the last pixel of the buffer
    last = len(c.frames) - 1
    assert any(f == last and (x, y) == (w - 1 - H, h - 1 - H) and c.status[(f, i)] == R.OK for f, i, x, y in recs)
    if name == "clip_25":
        assert (h, w) == (2 * H + 1, 2 * H + 1)


# ---- fixed point --------------------------------------------------------------------------------------------------------------

def exact(bits):
    """the value of a finite float32 bit pattern as a fraction"""
    e, m = (bits >> 23) & 0xff, bits & 0x7fffff
    v = Fraction(m | (0x800000 if e else 0)) * Fraction(2) ** ((e if e else 1) - 150)
    return -v if bits >> 31 else v


def fix_exact(bits):
    return round(exact(bits) * 2 ** 30)                     # (a Fraction rounds half to even)


def psf_fix(bits, tie=True):
    """psf_fix of k_psf.h in Python integers; tie=False leaves the ties-to-even term out"""
    e = (bits >> 23) & 0xff
    m = (bits & 0x7fffff) | (0x800000 if e else 0)
    sh = (e if e else 1) - 120
    if sh >= 0:
        q = m << sh
    elif sh < -25:
        q = 0
    else:
        s = -sh
        q = (m + ((1 << (s - 1)) - 1) + (((m >> s) & 1) if tie else 0)) >> s
    return -q if bits >> 31 else q


def test_the_fraction_rounds_as_the_header_says():
    assert [round(Fraction(k, 2)) for k in (1, 3, 5, 7, -1, -3, -5, -7)] == [0, 2, 2, 4, 0, -2, -2, -4]
    assert exact(0x3f800000) == 1 and exact(0xc5800000) == -4096 and exact(1) == Fraction(1, 2 ** 149) and exact(0x00800000) == Fraction(1, 2 ** 126)


def frame_patterns(name):
    c = P.get(name)
    return sorted({int(b) for b in np.unique(c.frames.view(np.uint32))})


@pytest.mark.parametrize("name", ["fix_edges", "sat_20", "extremes_65", "extremes_70x80"])
def test_fixed_point_against_exact_arithmetic(name):
    """every pixel of the case, the placed patterns among them"""
    c = P.get(name)
    pats = frame_patterns(name)
    assert set(c.patterns) <= set(pats)
    got = R.fixed(P.from_bits(*pats))
    for b, q in zip(pats, got):
        assert int(q) == fix_exact(b) == psf_fix(b), hex(b)


def test_fix_edges_patterns_reach_every_branch():
    c = P.get("fix_edges")
    pats = set(c.patterns)
    for k in (1, 3, 5, 7):                                                         # the ties of v 2^30, both signs
        for sign in (1, -1):
            assert P.bits_of(np.float32(sign * k * 2.0 ** -31)) in pats
    assert {0x2fffffff, 0x2f800000, 0x2f000000, 0x00000001, 0x007fffff, 0x33000001, 0x80000001, 0x807fffff} <= pats
    shifts = {120 - ((b >> 23) & 0xff) for b in pats if (b >> 23) & 0xff}
    assert set(range(0, 26)) <= shifts and any(s > 25 for s in shifts)           # sh >= 0, every shift with ties, the q = 0 branch
    on_tie = [b for b in pats if (exact(b) * 2 ** 30).denominator == 2]
    assert len(on_tie) > 40 and {fix_exact(b) % 2 for b in on_tie} == {0}
    down = [b for b in on_tie if psf_fix(b, tie=False) != fix_exact(b)]            # the ties above an odd integer
    assert len(down) > 20 and {b >> 31 for b in down} == {0, 1}
    # a kernel without the tie term gives other sums for stars of the case: one pattern each, so nothing cancels
    hit = [i for i, px in c.special.items() if len(px) == 1 and px[0][2] in down]
    assert len(hit) >= 4
    out = P.want("fix_edges")[0][0]
    for i in c.unused:
        assert out[i]["index"] == i and out[i]["Q0"] <= 0 and R.shape_of(out[i]) is None
    assert {int(out[i]["Q0"]) for i in c.unused} != {0} and 0 in {int(out[i]["Q0"]) for i in c.unused}
    ring = out[c.unused[0] - 1]
    assert ring["Q_ring"] == -49 and ring["n_ring"] == 16 and ring["Q_ring"] % 16 != 0
    assert any(s["Q_ring"] < 0 and s["Q_ring"] % 16 for s in out[:len(c.special)])
    assert all((c.frames[0, cy - 2:cy + 3, cx - 2:cx + 3] != 0).all() for cx, cy in [P.patch_centre(i, P.FIX_COLS) for i in c.special])


def test_sat_edges_turn_on_the_float_of_sat():
    (frames, rec, frec), placed = P.sat_frame()
    vals = {float(abs(v)) for v, _ in placed}
    for name, sat in P.SATS.items():
        c = P.get(name)
        lim = np.float32(sat)
        assert float(lim) in vals and float(np.nextafter(lim, np.float32(np.inf))) in vals
        st = statuses(name)[0]
        for k, (v, in_ring) in enumerate(placed):
            # one ulp above is refused, the value itself is not: '>' and not '>='
            if abs(v) == lim:
                assert st[k] == R.OK
            if abs(v) == np.nextafter(lim, np.float32(np.inf)):
                assert st[k] == R.BAD_PIXEL
        assert {in_ring for (v, in_ring) in placed if abs(v) == lim} == {True, False} and {float(v) for v, _ in placed if abs(v) == lim} == {float(lim), -float(lim)}
        assert 0 < c.n_ok[0] < len(placed) or name == "sat_default"
    # 20.1 narrows upwards: a comparison in double would refuse the pixel at (float)20.1
    assert float(np.float32(20.1)) > 20.1
    assert P.get("sat_default").n_ok[0] == len(placed) - 4                         # only the four pixels one ulp above 4096


# ---- the largest sums ----------------------------------------------------------------------------------------------------------

def sums_in_python(frame, cx, cy, win, gap, ring):
    """step 3 with Python integers and exact q"""
    H, inner = win + gap + ring, win + gap
    q = {(dx, dy): fix_exact(int(frame[cy + dy, cx + dx].view(np.uint32))) for dy in range(-H, H + 1) for dx in range(-H, H + 1)}
    ring_q = [v for (dx, dy), v in q.items() if max(abs(dx), abs(dy)) > inner]
    Q_ring = sum(ring_q)
    b = abs(Q_ring) // len(ring_q) * (1 if Q_ring >= 0 else -1)
    wq = [(dx, dy, v - b) for (dx, dy), v in q.items() if max(abs(dx), abs(dy)) <= win]
    partial = [abs(v) for (dx, dy), v in q.items()]
    return (len(ring_q), Q_ring, sum(p for _, _, p in wq), sum(p * dx for dx, _, p in wq), sum(p * dy for _, dy, p in wq),
            sum(p * dx * dx for dx, _, p in wq), sum(p * dy * dy for _, dy, p in wq), sum(p * dx * dy for dx, dy, p in wq)), max(partial)


@pytest.mark.parametrize("name", list(P.EXT_LAYOUT))
def test_extreme_moments_fit_an_int64(name):
    c = P.get(name)
    out, fr = P.want(name)
    p = c.params
    assert (p["win"], p["gap"], p["ring"]) == (16, 8, 8)
    big = {}
    for f, (kind, cx, cy) in enumerate(c.layout):
        s, qmax = sums_in_python(c.frames[f], cx, cy, 16, 8, 8)
        assert qmax == 2 ** 42
        assert s == R.sums_of(np.array(c.frames[f]), cx, cy, dict(R.DEFAULTS, **p))
        assert all(abs(v) <= INT64_MAX for v in s)
        # the kernel sums the raw q and subtracts b times the window's sums afterwards: those partial sums fit as well
        assert 2 ** 42 * 33 * 33 * 256 <= INT64_MAX and 2 ** 42 * (65 * 65 - 49 * 49) <= INT64_MAX
        got = out[f, 0]
        assert (int(got["n_ring"]), int(got["Q_ring"]), *(int(got[k]) for k in ("Q0", "Qx", "Qy", "Qxx", "Qyy", "Qxy"))) == s
        big[kind] = s
    if "up" in big:
        assert big["up"][5] == big["up"][6] == P.EXT_QXX_UP == 2 ** 43 * 33 * 2992 and P.EXT_QXX_UP.bit_length() == 60
        assert big["up"][2] == 2 ** 43 * 33 * 33 and big["up"][1] == -(2 ** 42) * (65 * 65 - 49 * 49)
    if name == "extremes_65":
        assert c.frames.shape[1:] == (65, 65)
        assert abs(big["qx"][3]) == abs(big["qy"][4]) == 2 ** 42 * 33 * 272          # sum |dx| over the window, q = +-2^42
        assert abs(big["qxy"][7]) == 2 ** 43 * 136 * 136 * 2 and big["qxy_neg"][7] == -big["qxy"][7]
        assert big["down"][5] == -P.EXT_QXX_UP
    else:
        h, w = c.frames.shape[1:]
        assert c.layout[-1][1:] == (w - 1 - P.EXT_H, h - 1 - P.EXT_H)


# ---- candidates ---------------------------------------------------------------------------------------------------------------

def test_candidate_edges_floors_differ():
    c = P.get("candidate_edges")
    fl = [float(v) for v in c.floors]
    assert len(set(fl)) == 3
    for s, f in zip(P.CAND_SIGMA, c.floors):                                       # the product is no float: the narrowing is seen
        assert Fraction(float(f)) != Fraction(P.CAND_PARAMS["k_peak"]) * 3 * Fraction(float(np.float32(s)))
    st = statuses("candidate_edges")
    peaks = c.records[0]["s_peak"][:c.n_peaks]
    for f in range(3):
        for k, v in enumerate(peaks):
            if v == c.floors[f]:
                assert st[f][k] == R.OK
            if v == np.nextafter(c.floors[f], np.float32(0)):
                assert st[f][k] == R.NOT_CANDIDATE
    assert np.isnan(peaks).sum() == 1 and np.isposinf(peaks).sum() == 1
    assert len({tuple(s[:c.n_peaks]) for s in st}) == 3                            # the same records, another answer per frame
    assert {int(v) for v in c.records[0]["rad"]} >= {0, 1, 16, 17, -1} and {int(v) for v in c.records[0]["flags"]} >= {0, 1, 2, 4, -2 ** 31}
