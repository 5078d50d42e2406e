"""CPU checks of tests/rs_cases.py: the oracle's remove_stars is the literal numpy slicing, ``squares`` gives the same zeros, every
case takes the route and crosses the constant it is named for, and none is vacuous.  No device."""
import numpy as np
import pytest

import front_cases as fc
import rs_cases as R
from rs_cases import CASES, BY_NAME


def oracle_rs(oracle, c):
    return oracle.rs_params(c.filter, **c.kw)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_oracle_equals_literal_and_squares(oracle, c):
    got = oracle.remove_stars(np.array(c.frame), c.cat, oracle_rs(oracle, c))
    assert np.array_equal(got.view(np.uint32), c.literal.view(np.uint32)), c
    z = np.zeros((c.h, c.w), bool)
    for sq in c.squares():
        if sq is not None and not R.is_empty(sq):
            z[sq[0]:sq[1], sq[2]:sq[3]] = True
    assert np.array_equal(z, c.literal == 0), c
    assert (c.frame != 0).all() and np.array_equal(c.literal[~z], c.frame[~z])
    # GRAY is zero exactly on the blotted pixels (bright and dim conversion), so the stage images show the mask pixel by pixel
    pb, pd = R.dim_params()
    for dim in (False, True):
        gray = oracle.prep(np.ascontiguousarray(c.literal[::-1]), oracle.PREP_BRIGHT_THEN_DIM if dim else oracle.PREP_BRIGHT, False,
                           pd["minFlux"] if dim else 0.0, pd["addFlux"] if dim else 0.0)
        assert np.array_equal(gray == 0, z[::-1]), (c, dim)
    if z.any() and not z.all():
        # ... and with a 1 x 1 erosion so does ERODED, the one 8-bit image of the dim pass that the folded route leaves
        r = fc.reference(oracle, np.ascontiguousarray(c.literal[::-1]), pd, True)
        assert np.array_equal(r["ERODED"] == 0, z[::-1]), c


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_named_squares_seams_and_route(c):
    sq = c.squares()
    z = c.literal == 0
    assert z.any() != c.nothing, c
    for i, want in c.named.items():
        if want is None:
            assert sq[i] is None, (c, i, sq[i])
        elif want == "empty":
            assert sq[i] is not None and R.is_empty(sq[i]), (c, i, sq[i])
        else:
            assert sq[i] == want and not R.is_empty(want), (c, i, sq[i])
    for kind, i in c.seams:
        strip = z[max(0, i - 2):i + 2] if kind == "row" else z[:, max(0, i - 2):i + 2]
        assert 0 <= i <= (c.h if kind == "row" else c.w) and strip.any() and not strip.all(), (c, kind, i)
        edge = (z[i - 1] != z[i]) if (kind == "row" and 0 < i < c.h) else (z[:, i - 1] != z[:, i]) if (kind == "col" and 0 < i < c.w) else np.array([True])
        assert edge.any(), (c, kind, i)                                     # a square's edge lies exactly on the seam
    pb, pd = R.dim_params()
    rt = R.route(c.h, c.w, len(c.objs), "device", "host", "f32", c.knobs, pd, 0)
    for k, v in c.expect.items():
        assert rt[k] == v, (c, k, rt)
    # with the stage images kept the dim pass takes its own sweep: no bit planes, the fill in front
    assert not R.route(c.h, c.w, len(c.objs), "device", "host", "f32", c.knobs, pd, 1)["fold"]
    # a device catalogue with host frames: the blotted copy travels back, so the fill stays in front
    assert R.route(c.h, c.w, len(c.objs), "host", "device", "f32", c.knobs, pd, 0) == dict(rt, fold=False, side=None, back="copy back")
    assert R.route(c.h, c.w, len(c.objs), "host", "host", "be", c.knobs, pd, 0)["back"] == "untouched"


def test_the_constants_are_crossed():
    sq = {c.name: [s for s in c.squares() if s is not None] for c in CASES}
    width = lambda s: s[3] - s[2]                                           # noqa: E731
    height = lambda s: s[1] - s[0]                                          # noqa: E731
    # slices: the wrap reaches the first row / column and ends one short of the last; it cannot reach the last
    for name, ax in (("wrap_rows", 0), ("wrap_cols", 1)):
        c = BY_NAME[name]
        lo, hi = [s[2 * ax] for s in sq[name] if not R.is_empty(s)], [s[2 * ax + 1] for s in sq[name] if not R.is_empty(s)]
        assert min(lo) == 0 and max(hi) == (c.h, c.w)[ax] - 1 and R.wrapped(c.cat, c.filter, **c.rs)
        assert all(o["x" if ax == 0 else "y"] + 6 < 0 for o in c.objs)
    c = BY_NAME["slice_empty"]
    assert [o["x"] for o in c.objs[:4]] == [-3, 20, 0, -6] and c.objs[4]["x"] == c.h + 6 + 1 and c.objs[5]["x"] == c.h + 6
    assert sorted(o["x"] for o in BY_NAME["slice_exact"].objs[:4]) == [6, 34, 40, 45]          # d, len - d, len, len + d - 1
    assert BY_NAME["short_h_lt_d"].h < 20 and 20 < BY_NAME["short_h_lt_2d"].h < 40
    assert (BY_NAME["cover_all"].literal == 0).all()
    # words: [32 k, 32 k + 32), across a word boundary by one bit, three words, one bit at bit 0 and at bit 31, ending at w
    s = sq["words"]
    cols = {(a[2], a[3]) for a in s}
    assert {(32, 64), (128, 160), (31, 65), (31, 33), (63, 65), (95, 97), (127, 129), (159, 160), (0, 1)} <= cols
    assert (31 >> 5, 64 >> 5) == (0, 2) and 159 & 31 == 31
    assert {a[2] % R.NIBBLE for a in s if width(a) == 2} == {0, 1, 2, 3} and {a[2] % R.NIBBLE for a in s if width(a) == 22} >= {1, 3}
    a, b = s[12], s[13]
    union = np.zeros((100, 160), bool)
    union[a[0]:a[1], a[2]:a[3]] = True
    union[b[0]:b[1], b[2]:b[3]] = True
    ys, xs = np.nonzero(union)
    assert union.sum() < (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)                  # the union is no rectangle
    # k_rs_fill: every width around its 32- and 64-lane steps, odd and even heights on both branches
    s = sq["fill_widths"] + sq["fill_w129"]
    assert {width(a) for a in s} >= set(R.FILL_WIDTHS)
    assert {height(a) % 2 for a in s if width(a) <= 32} == {0, 1} and {height(a) % 2 for a in s if width(a) > 32} == {0, 1}
    assert {-(-width(a) // R.FILL_LANES) for a in s if width(a) > 32} == {1, 2, 3}              # trips of the c += 64 loop
    # bands: first and last rows at every phase against eight rows, in the caller's orientation and flipped (the sweep)
    c = BY_NAME["band_phases"]
    s = sq["band_phases"]
    assert c.h % 4 and c.h % 8
    for f in (lambda r: r, lambda r: c.h - 1 - r):
        assert {f(a[0]) % 8 for a in s} == set(range(8)) and {f(a[1] - 1) % 8 for a in s} == set(range(8))
    # the sorted range: a square of exactly hmax rows whose last row is a band's first, and one that ends just above it
    for name in ("range_hmax", "range_default_above_maxxy"):
        c = BY_NAME[name]
        hm = R.hmax(**c.rs)
        tall = [a for a in sq[name] if height(a) == hm]
        assert {(a[1] - 1) % R.RS_BAND_ROWS for a in tall} >= {0, R.RS_BAND_ROWS - 1} and c.h % 8 == 0, (name, tall)
    c = BY_NAME["range_default_above_maxxy"]
    assert c.kw["defaultxy"] > c.kw["maxxy"] and height(sq[c.name][3]) == 2 * c.kw["defaultxy"] and height(sq[c.name][2]) == 2 * c.kw["maxxy"]
    # the sort: rows per thread, squares sharing a first row, catalogue sizes around the blocks of 4 and of 256 objects
    assert [R.sort_rows_per_thread(h) for h in (7, 1023, 1024, 1025, 2100)] == [1, 1, 2, 2, 3]
    for h in (1023, 1024, 1025, 2100):
        firsts = {a[0] for a in sq[f"sort_h{h}"]}
        assert {0, 1, h - 1, h - 12} <= firsts and (h < 1025 or 1023 in firsts) and (h < 2100 or {2047, 2048} <= firsts), (h, sorted(firsts))
    assert len({a[0] for a in sq["sort_one_first_row"]}) == 1 and len(sq["sort_one_first_row"]) == 40
    assert sq["sort_all_stay"] == []
    assert [len(BY_NAME[f"crowd_{n}"].objs) for n in R.CROWD_SIZES] == [1, 3, 4, 5, 255, 256, 257]
    assert [R.fill_halves(n) for n in (1, 3, 4, 5)] == [(0, 1), (0, 1), (0, 1), (1, 2)] and R.fill_halves(11) == (1, 3)   # a single block: the first part is empty
    for n in (255, 256, 257):
        c = BY_NAME[f"crowd_{n}"]
        assert R.wrapped(c.cat, "r") and any(s is None for s in c.squares()) and any(s is not None and R.is_empty(s) for s in c.squares())
    # shapes
    assert BY_NAME["w4128"].w > R.RS_MAXW and BY_NAME["w4128"].w % 32 == 0 and BY_NAME["w4096"].w == R.RS_MAXW
    assert BY_NAME["w100"].w % 32 == 4 and BY_NAME["w136"].w % 32 == 8 and BY_NAME["w136"].w % 4 == 0
    assert {c.filter for c in CASES if c.row == R.CAT} == set(R.FILTERS)


def test_no_case_spills_by_design(oracle):
    """Canny sees little more than the squares' outlines: the flat frame alone leaves no edge pixel at all."""
    pb, pd = R.dim_params()
    for h, w in ((40, 160), (100, 256), (330, 416)):
        r = fc.reference(oracle, np.ascontiguousarray(R.flat(h, w)[::-1]), pd, True)
        assert not r["CANNY"].any(), (h, w)


def test_batches(oracle):
    pb, pd = fc.default_params()
    shapes = {(BY_NAME[n].h, BY_NAME[n].w) for n in R.BATCH5 if n in BY_NAME}
    assert shapes == {(40, 160)} and all(BY_NAME[n].rs == {} and BY_NAME[n].filter == "r" for n in R.BATCH5 + R.BATCH8 if n in BY_NAME)
    # counts of 0, 1 and max_obj in neighbouring frames of one batch; the frame whose images the device test fetches has squares
    counts = [0 if R.batch_cat(n) is None else len(R.batch_cat(n)["NOBSERVE"]) for n in R.BATCH5]
    assert counts == [5, 0, 1, 8, 5] and len(R.BATCH_SMALLER) == 1 and max(counts) == 8
    assert (R.literal(R.flat(40, 160), R.batch_cat(R.BATCH5[4]), "r") == 0).any() and (R.literal(R.flat(40, 160), R.batch_cat("ONE"), "r") == 0).sum() == 144
    assert [len(c["NOBSERVE"]) for _, c in R.batch8()].count(1) == 1
    assert len(R.BATCH_BIGGER) > max(counts) > len(R.BATCH_SMALLER)
    # the eight-slot batch: the bright pass decides the streak frames (blotted) and no other
    found = []
    for f, cat in R.batch8():
        lit = R.literal(f, cat, "r")
        found.append(oracle.process_bright(np.ascontiguousarray(lit), pb, flip=True)["found"])
    assert found == [1 if n == "STREAK" else 0 for n in R.BATCH8], found
    assert (R.literal(R.streak(), R.catalogue(R.BATCH8_STREAK_CAT), "r") == 0).sum() > 200
    assert all((R.literal(f, cat, "r") == 0).any() for f, cat in R.batch8())
    for n in R.CHILD_CASES + R.SPILL_CASES:
        assert BY_NAME[n].batch and not BY_NAME[n].knobs


def test_random_frames_with_wrapped_squares(oracle):
    """literal against the oracle on 300 random small frames with centres in uniform(-70, side + 70), 40 objects each; at least a
    quarter of the frames hold a wrapped square (the share is printed)."""
    rng = np.random.default_rng(2024)
    n_frames, n_wrapped, n_bad = 300, 0, 0
    for k in range(n_frames):
        h, w = int(rng.integers(8, 90)), int(rng.integers(8, 120))
        n = 40
        cat = {"ROWC": rng.uniform(-70, w + 70, (n, 5)).astype(np.float32), "COLC": rng.uniform(-70, h + 70, (n, 5)).astype(np.float32),
               "PSFMAG": rng.uniform(14, 24, (n, 5)).astype(np.float32), "PETROTH90": rng.uniform(-2, 30, (n, 5)).astype(np.float32),
               "NOBSERVE": rng.integers(1, 3, n).astype(np.int32), "NDETECT": rng.integers(1, 3, n).astype(np.int32)}
        flt = R.FILTERS[k % 5]
        kw = dict(defaultxy=int(rng.integers(2, 12)), maxxy=int(rng.integers(8, 40)))
        img = rng.normal(3, 1, (h, w)).astype(np.float32)
        img[img == 0] = 1.0
        want = R.literal(img, cat, flt, **kw)
        got = oracle.remove_stars(img.copy(), cat, oracle.rs_params(flt, **dict(R.RS_DEFAULT, **kw)))
        n_bad += not np.array_equal(got.view(np.uint32), want.view(np.uint32))
        hit = False
        for i, s in enumerate(R.squares(cat, flt, (h, w), **kw)):
            if s is not None and not R.is_empty(s):
                sel = R._selected(cat, i, flt, **dict(R.RS_DEFAULT, **kw))
                hit = hit or sel[0] + sel[2] < 0 or sel[1] + sel[2] < 0
        n_wrapped += hit
    print(f"oracle vs literal: {n_frames} frames, {n_bad} differ, {n_wrapped} hold a wrapped, non-empty square")
    assert n_bad == 0 and n_wrapped >= n_frames // 4, (n_bad, n_wrapped)


def test_every_row_of_the_table_has_a_case():
    rows = {c.row for c in CASES}
    assert len(rows) >= 8 and len(CASES) >= 40
    assert all(c.frame.size <= R.MAX_PIXELS for c in CASES) and max(c.h for c in CASES) < R.RS_SORT_MAXH
    assert [c.name for c in CASES if not c.batch] == ["sort_h7"]
