"""The cases of tests/trail_cases.py on the CPU: every one reaches the status and the property it is there for, in the
restatement tests/trail_ref.py, and every group holds a case whose result changes when the restatement is made wrong in one of
the ways a kernel can be wrong.  This is what keeps tests/test_gpu_trail_edges.py from passing without having tested the edge."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trail_cases as TC  # noqa: E402
import trail_ref as T  # noqa: E402


def start_line(c):
    th, r = float(c["theta"]), float(c["rho"])
    return [r * math.cos(th), r * math.sin(th)], [-math.sin(th), math.cos(th)]


def oracle_mask(oracle, shape, cat):
    ones = np.ones(shape, np.float32)
    oracle.remove_stars(ones, cat, oracle.rs_params(**TC.RS))
    return ones == 0


@pytest.fixture(scope="module")
def masks(oracle):
    """the CPU oracle's remove_stars squares of the catalogue cases"""
    return {n: oracle_mask(oracle, TC.frame(n).shape, c["cat"]) for n, c in TC.CASES.items() if c["cat"] is not None}


def restated(name, masks):
    return TC.restated(name, masks.get(name))


def differs(a, b):
    (ra, pa), (rb, pb) = a, b
    for k in T.FIELDS:
        if not (ra[k] == rb[k] or (math.isnan(ra[k]) and math.isnan(rb[k]))):
            return True
    return not np.array_equal(pa, pb, equal_nan=True)


def test_frames_and_parameters_are_in_range():
    assert set(c["group"] for c in TC.CASES.values()) == set(TC.GROUPS)
    for n, c in TC.CASES.items():
        f = TC.frame(n)
        assert f.dtype == np.float32 and all(64 <= s <= 333 for s in f.shape), n
        assert c["rho"].dtype == np.float32 and c["theta"].dtype == np.float32 and c["note"], n
        p = dict(T.DEFAULTS, **c["params"])
        K = p["prof_half"] / p["prof_step"]
        assert 1 <= p["half_width"] <= 64 and 2 <= p["seg_len"] <= 64 and 0 <= p["n_iter"] <= 16, n
        assert 1 <= p["wing"] <= p["half_width"] and p["wing"] <= p["prof_half"] and K == int(K) and 1 <= K <= 512, n
        assert c["params"] != {} and any(p[k] != T.DEFAULTS[k] for k in p), n
    assert {TC.frame(n).shape[1] for n in TC.CASES} >= {65, 100, 333}
    # the corners the parameter ranges have
    P = [dict(T.DEFAULTS, **c["params"]) for c in TC.CASES.values()]
    assert {p["seg_len"] for p in P} >= {2, 3, 31, 32, 33, 63, 64}
    assert any((p["half_width"], p["seg_len"], p["wing"], p["n_iter"], T.n_bins(p)) == (1, 2, 1, 0, 3) for p in P)
    assert any((p["half_width"], p["seg_len"], p["wing"], p["n_iter"], T.n_bins(p)) == (64, 64, 64, 16, 1025) for p in P)
    assert {p["wing"] - p["half_width"] for p in P if p["half_width"] == 8} >= {-7, -1, 0}


def test_every_case_reaches_its_status(masks):
    got = {n: restated(n, masks)[0]["status"] for n in TC.CASES}
    assert got == {n: c["status"] for n, c in TC.CASES.items()}
    st = list(got.values())
    assert 3 * st.count(T.OK) >= 2 * len(st)
    for s in (T.NOT_FOUND, T.TOO_SHORT, T.TOO_FAINT):
        assert st.count(s) >= 2, s
    for n, c in TC.CASES.items():
        r, p = restated(n, masks)
        assert p.shape == (T.n_bins(c["params"]),)
        if r["status"] != T.OK:
            assert np.isnan(p).all() and math.isnan(r["fwhm"])


def test_every_case_has_its_property(masks):
    for n, c in TC.CASES.items():
        if c["prop"] is not None:
            assert c["status"] == T.OK and c["prop"](*restated(n, masks)), n


def test_length_cases_keep_or_drop_the_partial_segment(masks):
    seen = set()
    for c in TC.CASES.values():
        if "rem" not in c:
            continue
        L, rem = c["L"], c["rem"]
        h, w = TC.frame(c["name"]).shape
        _, npos, nseg = T.positions(h, w, *start_line(c), L)
        assert npos % L == rem and rem in (L // 2 - 1, L // 2, L // 2 + 1) and npos >= 2 * L
        assert c["kept"] == (rem > 0 and 2 * rem >= L) and nseg == npos // L + c["kept"]
        r, _ = restated(c["name"], masks)
        assert r["n_seg"] == nseg                      # the refit kept the length, and every segment is in the extent
        seen.add((L % 2, c["kept"], 2 * rem == L))
    assert seen >= {(0, True, True), (0, True, False), (0, False, False), (1, True, False), (1, False, False)}


def test_geometry_cases_lie_where_they_say(masks):
    C = TC.CASES
    assert float(C["theta_0"]["theta"]) == 0.0 and math.copysign(1.0, start_line(C["theta_0"])[1][0]) == -1.0   # d.x = -0.0
    assert C["theta_pi2"]["theta"] == np.float32(math.pi / 2) and start_line(C["theta_pi2"])[1][1] != 0.0
    for n, fixed in (("column_0", (0, 0.0)), ("column_last", (0, 99.0)), ("row_0", (1, 0.0))):
        f, d = start_line(C[n])
        axis, val = fixed
        assert abs(f[axis] - val) < 1e-5 and abs(d[axis]) < 1e-6, n
    for n in ("npos_2L_minus_1", "npos_2L", "refit_too_short"):
        h, w = TC.frame(n).shape
        L = C[n]["params"]["seg_len"]
        npos = T.positions(h, w, *start_line(C[n]), L)[1]
        assert npos == {"npos_2L_minus_1": 2 * L - 1, "npos_2L": 2 * L}.get(n, npos)
        if n == "refit_too_short":      # long enough at first: with no refit the same line is measured
            assert npos >= 2 * L
            r, _ = T.measure(TC.frame(n), C[n]["rho"], C[n]["theta"], **dict(C[n]["params"], n_iter=0))
            assert r["status"] == T.OK
    for n, ends in (("diagonal", ((0, 0), (332, 95))), ("anti_diagonal", ((0, 99), (99, 0)))):
        th, r = float(C[n]["theta"]), float(C[n]["rho"])
        for x, y in ends:
            assert abs(x * math.cos(th) + y * math.sin(th) - r) < 1e-3, n


def test_tie_and_bad_sample_cases_hold_what_they_say(masks):
    C = TC.CASES
    f = TC.frame("quantised_vertical")
    assert len(np.unique(f)) <= 16 and (f < 0).any() and np.signbit(f[f == 0]).any()
    z = TC.frame("signed_zeros")[:, 39:42]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all() and (TC.frame("signed_zeros")[:, :38] < 0).all()
    assert C["sigma_on_equality"]["params"]["k_sig"] * (1.4826 * 1.0) == 4.0
    # the overflow case: every pixel finite, yet samples along the start line that are inf and samples that are NaN
    o = C["overflow"]
    fo = TC.frame("overflow")
    assert np.isfinite(fo).all() and np.abs(fo).max() > 2.9e38
    fp, d = start_line(o)
    t, u = np.meshgrid(np.arange(0.0, 110.0), np.arange(-4.0, 4.5, 0.5))
    with np.errstate(all="ignore"):
        v = T.sample(fo, None, fp[0] + t * d[0] + u * d[1], fp[1] + t * d[1] - u * d[0])
    assert np.isinf(v).any() and np.isfinite(restated("overflow", masks)[1]).all()
    raw = T.sample(np.where(np.abs(fo) > 1e38, np.float32(0), fo), None, fp[0] + t * d[0] + u * d[1], fp[1] + t * d[1] - u * d[0])
    assert (np.isnan(v) & ~np.isnan(raw)).any()          # NaN from inf - inf, not from the frame's border
    # one valid sample per offset in segment 3
    c = C["one_valid_sample"]
    fp, d = start_line(c)
    ts = np.arange(24.0, 32.0)
    for uu in range(-6, 7):
        v = T.sample(TC.frame("one_valid_sample"), None, fp[0] + ts * d[0] + uu * d[1], fp[1] + ts * d[1] - uu * d[0])
        assert (~np.isnan(v)).sum() == 1


def test_mask_squares_have_the_listed_column_edges(oracle, masks):
    for w, objs in TC.MASK_OBJECTS.items():
        edges = {e for pair in TC.MASK_EDGES[w] for e in pair}
        assert edges >= {0, 31, 32, 63, 64, w - 1}
        for n in (f"mask_w{w}", f"mask_w{w}_tilted"):
            c = TC.CASES[n]
            h = TC.MASK_SHAPES[w]
            assert np.array_equal(masks[n], TC.boxes_mask(c))
            assert len(np.unique(TC.frame(n))) == h * w        # distinct values: a wrong bit moves a median or a count
            d = np.abs(TC.dist(h, w, float(c["rho"]), float(c["theta"])))
            spans = []
            for i in range(len(objs)):
                one = oracle_mask(oracle, (h, w), {k: v[i:i + 1] for k, v in c["cat"].items()})
                cols = np.flatnonzero(one.any(axis=0))
                assert (cols[0], cols[-1]) == TC.MASK_EDGES[w][i] and one[:, cols[0]:cols[-1] + 1].any(axis=0).all()
                assert d[one].min() < 0.75                      # the square crosses the line
                spans.append((cols[-1] >> 5) - (cols[0] >> 5) + 1)
            assert min(spans) == 1 and (w == 100 or max(spans) == 3)
            assert min(e[1] - e[0] + 1 for e in TC.MASK_EDGES[w]) < 32


def test_cases_whose_point_is_a_parameter_depend_on_it(masks):
    C = TC.CASES

    def again(n, **other):
        return T.measure(TC.frame(n), C[n]["rho"], C[n]["theta"], **dict(C[n]["params"], **other))

    for n, other in (("wing_1", 2), ("wing_7", 6), ("wing_8", 7)):          # the wing width reaches background and noise
        r, _ = restated(n, masks)
        q, _ = again(n, wing=other)
        assert r["n_seg"] == q["n_seg"] == 3 and (r["background"], r["noise"]) != (q["background"], q["noise"]), n
    assert again("k_sig_0", k_sig=5.0)[0]["status"] == T.TOO_FAINT          # its segments have 0 < A < 5 sd
    assert again("k_sig_huge", k_sig=5.0)[0]["status"] == T.OK
    # the flat profile is k_trail_final's TOO_FAINT: the fit has its run, and a profile window that reaches the box is measured
    assert again("flat_profile", prof_half=16.0)[0]["status"] == T.OK
    assert again("flat_profile", half_width=4, wing=1)[0]["status"] == T.TOO_FAINT     # ... where the fit's is not
    for n in ("quantised_vertical", "quantised_on_pixels", "quantised_tilted"):
        assert len(np.unique(TC.frame(n))) <= 16 and (TC.frame(n) < 0).any(), n


# ---- sensitivity: a restatement with one of a kernel's possible mistakes gives another result -------------------------------------
def upper_median(v):
    v = np.sort(np.asarray(v))
    return v[len(v) // 2] if len(v) else np.nan


def partial_needs_more_than_half(npos, L):
    return npos // L + (1 if 2 * (npos % L) > L else 0)


def last_run_wins(flags):
    best0 = bestn = cur0 = curn = 0
    for sg, f in enumerate(flags):
        if f:
            cur0 = sg if curn == 0 else cur0
            curn += 1
            if curn >= bestn:
                bestn, best0 = curn, cur0
        else:
            curn = 0
    return best0, bestn


def wings_off_by_one(md, R, wing):
    return np.concatenate([md[:wing], md[2 * R - wing:2 * R]])


WRONG = {"upper_median": ("lowmed", upper_median), "partial_rule": ("n_segments", partial_needs_more_than_half),
         "last_run": ("longest_run", last_run_wins), "wing_index": ("wing_values", wings_off_by_one)}
# the cases each mistake has to change
MUST_CHANGE = {"upper_median": {"all_max", "theta_0", "quantised_vertical", "one_valid_sample", "fwhm_zero", "mask_w100"},
               "partial_rule": {"len_L2_rem1", "len_L32_rem16", "len_L64_rem32"},
               "last_run": {"two_equal_runs"},
               "wing_index": {"wing_1", "wing_7", "wing_8", "all_max"},
               "mask_shift": {"mask_w100", "mask_w100_tilted", "mask_w333", "mask_w333_tilted"}}


def changed_by(which, masks, refs, monkeypatch):
    """the cases whose result under one mistake differs from refs, the results of the unpatched restatement"""
    with monkeypatch.context() as m:
        if which != "mask_shift":
            m.setattr(T, *WRONG[which])
        out = set()
        for n, c in TC.CASES.items():
            if not c["found"]:
                continue
            mask = masks.get(n)
            if which == "mask_shift":
                if mask is None:
                    continue
                mask = np.roll(mask, 1, axis=1)
            with np.errstate(all="ignore"):
                wrong = T.measure(TC.frame(n), c["rho"], c["theta"], star_mask=mask, **c["params"])
            if differs(wrong, refs[n]):
                out.add(n)
    return out


@pytest.fixture(scope="module")
def changed(masks):
    refs = {n: restated(n, masks) for n in TC.CASES}      # all of them, before anything is patched
    mp = pytest.MonkeyPatch()
    try:
        return {which: changed_by(which, masks, refs, mp) for which in MUST_CHANGE}
    finally:
        mp.undo()


@pytest.mark.parametrize("which", sorted(MUST_CHANGE))
def test_a_wrong_restatement_changes_the_cases_meant_for_it(changed, which):
    assert changed[which] >= MUST_CHANGE[which], MUST_CHANGE[which] - changed[which]


def test_every_group_would_catch_a_mistake(changed):
    for g in TC.GROUPS:
        names = {c["name"] for c in TC.by_group(g)}
        assert names & changed["upper_median"], g
    # and the mistakes that belong to one group are caught there
    in_group = lambda which, g: changed[which] & {c["name"] for c in TC.by_group(g)}   # noqa: E731
    assert in_group("partial_rule", "corners") and in_group("wing_index", "corners")
    assert in_group("last_run", "ties") and in_group("mask_shift", "mask")
    # the partial-segment rule differs only at 2 * rem == L
    lens = {c["name"] for c in TC.CASES.values() if "rem" in c}
    assert changed["partial_rule"] & lens == {c["name"] for c in TC.CASES.values() if "rem" in c and 2 * c["rem"] == c["L"]}


def test_the_restatement_is_itself_again(changed, masks):
    """the patches are gone: the shared results are those of the unpatched module"""
    for n in ("all_min", "two_equal_runs", "wing_7"):
        c = TC.CASES[n]
        assert not differs(T.measure(TC.frame(n), c["rho"], c["theta"], **c["params"]), restated(n, masks))
