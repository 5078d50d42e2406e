"""The defocus fit (k_def_gemm / k_def_pick) at the edges of its tiles: banks of tests/defocus_cases.py whose columns, groups
and k-steps sit on, inside and across the GEMM's tiles, row counts around the 128-row tile and the 4096-row chunk, position
independence, degenerate rows, fixed seeing, ties between bit-identical columns, and the workspace shared by banks of different
sizes.  Every fitted row is held to the acceptance rule of tests/defocus_ref.py (accept), whose only tolerance is the derived
bound e of score_bound; the inputs' conditions (cap on non-decisive rows, tile facts) are checked on the CPU in
tests/test_defocus_model.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defocus_cases as DC  # noqa: E402
import defocus_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NOT_MEASURED, GAPS, NO_NOISE, NO_MODEL = 1, 2, 3, 4


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2**31) - ai, ai)
    bi = np.where(bi < 0, np.int64(-2**31) - bi, bi)
    return np.abs(ai - bi)


def rel_same(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (a == b) | (np.abs(a - b) <= tol * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def same_fits(a, b):
    """two results bit for bit, NaN equal to NaN: (records, chi2_by_height) each"""
    (fa, ca), (fb, cb) = a, b
    assert fa.shape == fb.shape and ca.shape == cb.shape
    for k in fa.dtype.names:
        assert np.array_equal(fa[k], fb[k], equal_nan=fa[k].dtype.kind == "f"), (k, fa[k], fb[k])
    assert np.array_equal(ca, cb, equal_nan=True), (ca, cb)


def check_bank(bank, rb):
    """the criteria of test_gpu_defocus.py::test_bank_equals_the_restatement"""
    cols = bank.columns()
    assert cols.shape == rb.c32.shape
    grid = bank.grid
    assert np.array_equal(grid["valid"], rb.valid)
    assert ulp_diff(cols[rb.vcol], rb.c32[rb.vcol]).max() <= 1
    assert not cols[~rb.vcol].any()
    for k in ("dfwhm", "ofwhm", "depth"):
        assert rel_same(grid[k], [m[k] for m in rb.models], 1e-9), k
    assert np.array_equal(grid["h"], [m["h"] for m in rb.models])
    assert np.array_equal(grid["radius"], [m["R"] for m in rb.models])
    assert np.array_equal(grid["sfwhm"], [m["seeing"] for m in rb.models])


def check_fit(rb, bank, trails, prof, fit, cbh, seeing=None, rows=None):
    """the acceptance rule on every row (or on `rows`); returns the number of rows where either status was accepted"""
    J = R.judge(rb, trails, prof, seeing)
    band = 0
    for i in (range(len(prof)) if rows is None else rows):
        band += R.accept(rb, J, i, trails[i], prof[i], fit[i], cbh[i], bank.delta_chi2) == "band"
    return band, J


@pytest.fixture(scope="module")
def ctx():
    from lfd_amd import _native
    with _native.Context(0, 64, 64, 1) as c:
        yield c


def open_bank(ctx, ge):
    from lfd_amd import defocus
    return defocus.DefocusBank(ctx, **DC.bank_kwargs(ge))


@pytest.fixture(scope="module")
def two(ctx):
    """the bank of two k-steps: tiny, so the row tests cost nothing"""
    with open_bank(ctx, DC.GEOMS["two_k_steps"]) as bank:
        yield bank, DC.restated("two_k_steps")


# ---- 2. geometries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.GEOMS))
def test_geometry_bank_and_fit(ctx, name):
    rb, trails, prof = DC.fit_inputs(name)
    with open_bank(ctx, DC.GEOMS[name]) as bank:
        assert (bank.n_columns, bank.n_bins) == (rb.ncol, rb.nb)
        check_bank(bank, rb)
        fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
        band, J = check_fit(rb, bank, trails, prof, fit, cbh)
    print(name, "rows in the either-status band:", band, "NO_MODEL:", int((fit["status"] == NO_MODEL).sum()))
    assert (fit["status"] == 0).sum() >= len(prof) // 2


# ---- 3. rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 4096])
def test_row_counts(ctx, two, n):
    bank, rb = two
    trails, prof, _ = DC.make_rows(rb, n, 7 + n)
    fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
    rows = None if n <= 500 else np.sort(np.random.default_rng(n).choice(n, 500, replace=False))
    check_fit(rb, bank, trails, prof, fit, cbh, rows=rows)


def test_second_chunk_with_inactive_rows_interleaved(ctx, two):
    """4097 active rows among rows that are not fitted: the second GEMM chunk holds one row, and active row 4096 is not caller
    row 4096"""
    from lfd_amd import _native
    bank, rb = two
    N = 6400
    reason = np.zeros(N, int)                       # 0 fitted, else the status the row must get
    reason[3::7], reason[5::11], reason[8::13] = GAPS, NOT_MEASURED, NO_NOISE
    reason[4090:4102] = [0, GAPS, 0, NOT_MEASURED, 0, NO_NOISE, GAPS, 0, 0, NOT_MEASURED, NO_NOISE, 0]
    n = int(np.flatnonzero(np.cumsum(reason == 0) == 4097)[0]) + 4     # the row of the 4097th active one, then three inactive
    reason = reason[:n]
    reason[-3:] = [GAPS, NOT_MEASURED, NO_NOISE]
    active = np.flatnonzero(reason == 0)
    assert len(active) == 4097 and active[4096] > 4096 + 100 and n > 4096
    trails, prof, _ = DC.make_rows(rb, n, 11)
    for k, i in enumerate(np.flatnonzero(reason == GAPS)):
        prof[i, k % rb.nb] = np.nan
    trails["status"][reason == NOT_MEASURED] = _native.TRAIL_TOO_FAINT
    trails["noise"][reason == NO_NOISE] = 0.0
    fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
    for i in np.flatnonzero(reason):
        assert R.is_blank(fit[i], reason[i]), (i, fit[i])
        assert np.isnan(cbh[i]).all(), i
    rows = np.union1d(np.random.default_rng(5).choice(active, 480, replace=False),
                      np.concatenate([active[:4], active[4090:], active[(active > 4080) & (active < 4110)]]))
    assert len(rows) <= 520
    check_fit(rb, bank, trails, prof, fit, cbh, rows=rows)
    # the row of the second chunk, and the last of the first, are what they are alone
    for i in active[4095:]:
        same_fits((fit[i:i + 1], cbh[i:i + 1]), ctx.fit_defocus(bank, trails[i:i + 1], prof[i:i + 1], chi2_by_height=True))


@pytest.mark.parametrize("name", ["two_k_steps", "last_tile_of_one"])
def test_a_rows_result_does_not_depend_on_its_position(ctx, name):
    """the score of a row depends on that row alone: permuted, and each row alone, every result is the batch's bit for bit"""
    rb = DC.restated(name)
    trails, prof, _ = DC.make_rows(rb, 300, 21)
    with open_bank(ctx, DC.GEOMS[name]) as bank:
        fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
        assert len(np.unique(fit["column"])) > 20     # neighbouring rows differ, or a permuted row map would go unseen
        perm = np.random.default_rng(3).permutation(len(prof))
        pf, pc = ctx.fit_defocus(bank, trails[perm], prof[perm], chi2_by_height=True)
        same_fits((pf, pc), (fit[perm], cbh[perm]))
        for i in range(len(prof)):
            same_fits(ctx.fit_defocus(bank, trails[i:i + 1], prof[i:i + 1], chi2_by_height=True), (fit[i:i + 1], cbh[i:i + 1]))


def test_degenerate_rows_leave_their_tile_alone(ctx, two):
    """a constant row, a row with +Inf and a row of values near 1e18 inside one 128-row tile of ordinary rows"""
    bank, rb = two
    trails, prof, _ = DC.make_rows(rb, 128, 31)
    base = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
    const, inf, big = 5, 40, 77
    t2, p2 = trails.copy(), prof.copy()
    p2[const] = 2.75
    p2[inf, 3] = np.inf
    j = int(np.flatnonzero(rb.vcol)[9])
    rng = np.random.default_rng(32)
    p2[big] = (1e18 * (3.0 * rb.c64[j] + 0.5 + rng.normal(0.0, 0.05, rb.nb))).astype(np.float32)
    t2["noise"][big] = 0.05e18
    fit, cbh = ctx.fit_defocus(bank, t2, p2, chi2_by_height=True)
    rest = np.setdiff1d(np.arange(128), [const, inf, big])
    same_fits((fit[rest], cbh[rest]), (base[0][rest], base[1][rest]))
    J = R.judge(rb, t2, p2)
    has_allowed = ~np.isnan(J["curve"][const])
    assert has_allowed.any()
    # constant: v~ = 0, every score 0: no model, and chi2 0 wherever a height has an allowed column
    assert R.is_blank(fit[const], NO_MODEL), fit[const]
    assert np.array_equal(cbh[const][has_allowed], np.zeros(has_allowed.sum(), np.float32)) and np.isnan(cbh[const][~has_allowed]).all()
    # +Inf: v - mean(v) is NaN / -Inf, no score compares above 0: no model, chi2_by_height NaN at every height (include/lfdmi.h)
    assert R.is_blank(fit[inf], NO_MODEL), fit[inf]
    assert np.isnan(cbh[inf]).all()
    # 1e18: float32 scores near 1e19 stay finite, and the rule holds with the same relative bound
    assert J["must_ok"][big] and J["decisive"][big]
    assert np.isfinite(cbh[big][has_allowed]).all()
    R.accept(rb, J, big, t2[big], p2[big], fit[big], cbh[big], bank.delta_chi2)
    assert fit["column"][big] == j
    # and the constant row's neighbours still satisfy the rule
    check_fit(rb, bank, t2, p2, fit, cbh, rows=rest)


SEEING_CASES = [  # the seeing grid, then (given seeing, the slice index it must select; None: free)
    ([1.0, 2.0], [(np.nan, None), (0.9, 0), (1.2, 0), (1.5, 0), (1.6, 1), (2.4, 1)]),     # 1.5: half-way, the lower value
    ([2.0, 1.0], [(np.nan, None), (0.9, 1), (1.5, 1), (1.6, 0), (2.0, 0)]),               # unsorted: still the value 1.0
    ([1.0, 1.0, 2.0], [(np.nan, None), (1.1, 0), (1.0, 0), (1.5, 0), (1.9, 2)]),          # the same seeing twice: the first
]


@pytest.mark.parametrize("seeings,given", SEEING_CASES, ids=["sorted", "unsorted", "twice"])
def test_fixed_seeing_selects_the_documented_slice(ctx, seeings, given):
    ge = DC.variant("two_k_steps", seeings=seeings)
    rb = DC.restate(ge)
    trails, prof, _ = DC.make_rows(rb, 40 * len(given), 41)
    seeing = np.array([given[i % len(given)][0] for i in range(len(prof))], np.float32)
    want = [given[i % len(given)][1] for i in range(len(prof))]
    with open_bank(ctx, ge) as bank:
        fit, cbh = ctx.fit_defocus(bank, trails, prof, seeing=seeing, chi2_by_height=True)
        check_fit(rb, bank, trails, prof, fit, cbh, seeing=seeing)
    ok = np.flatnonzero(fit["status"] == 0)
    assert len(ok) >= len(prof) // 2
    per = rb.ncol // rb.n_se
    seen = set()
    for i in ok:
        if want[i] is not None:
            assert fit["column"][i] // per == want[i], (i, seeing[i], fit["column"][i])
            assert fit["seeing_arcsec"][i] == seeings[want[i]]
            seen.add((float(seeing[i]), want[i]))
    assert len(seen) == sum(w is not None for _, w in given)
    if seeings == [1.0, 1.0, 2.0]:    # free rows: of two identical slices the lower wins
        assert not ((fit["column"][ok] // per) == 1).any()


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties():
    return DC.tie_cases()


@pytest.mark.parametrize("name", ["focus_duplicates", "equal_radii", "equal_heights", "equal_seeings"])
def test_of_identical_columns_the_lowest_index_wins(ctx, ties, name):
    ge, rb, trails, prof, want = ties[name]
    with open_bank(ctx, ge) as bank:
        check_bank(bank, rb)
        fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
        band, J = check_fit(rb, bank, trails, prof, fit, cbh)
    assert J["decisive"].all() and J["must_ok"].all() and band == 0
    assert np.array_equal(fit["column"], want), (fit["column"], want)
    if name == "equal_heights":
        dchi = bank.delta_chi2
        for f, c in zip(fit, J["curve"]):
            if c[-1] > np.nanmin(c) + dchi + 1.0:     # the focus model is far from the threshold
                assert f["h_lo"] == f["h_hi"] == 100.0, f


# ---- 5. workspace reuse -----------------------------------------------------------------------------------------------------
def test_banks_of_different_sizes_share_one_workspace():
    """the fit's workspace keeps running maxima of rows, nbp, groups and heights: a small bank after a large one, and the
    reverse, use buffers whose strides differ from their capacity"""
    from lfd_amd import _native
    big, small = DC.LARGEST, "one_k_step"
    fa, fb = DC.tile_facts(DC.restated(big)), DC.tile_facts(DC.restated(small))
    assert fa["nbp"] > fb["nbp"] and fa["n_groups"] > fb["n_groups"]
    inputs = {big: DC.fit_inputs(big)[1:], small: tuple(x[:129] for x in DC.fit_inputs(small)[1:])}
    assert len(inputs[big][0]) == 300

    def fit(c, bank, name):
        return c.fit_defocus(bank, *inputs[name], chi2_by_height=True)

    fresh = {}
    for name in (big, small):
        with _native.Context(0, 64, 64, 1) as c, open_bank(c, DC.GEOMS[name]) as bank:
            fresh[name] = fit(c, bank, name)
        assert (fresh[name][0]["status"] == 0).sum() > 64
    with _native.Context(0, 64, 64, 1) as c:
        A = open_bank(c, DC.GEOMS[big])
        same_fits(fit(c, A, big), fresh[big])
        B = open_bank(c, DC.GEOMS[small])
        same_fits(fit(c, B, small), fresh[small])
        same_fits(fit(c, A, big), fresh[big])
        B.close()
        same_fits(fit(c, A, big), fresh[big])
        A.close()
    with _native.Context(0, 64, 64, 1) as c:
        B = open_bank(c, DC.GEOMS[small])
        same_fits(fit(c, B, small), fresh[small])
        A = open_bank(c, DC.GEOMS[big])
        same_fits(fit(c, A, big), fresh[big])
        same_fits(fit(c, B, small), fresh[small])
        A.close()
        B.close()
