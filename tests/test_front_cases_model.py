"""CPU checks of tests/front_cases.py: the composed reference is the oracle's own pass, every case takes the route and crosses the
constant it is named for, and none is vacuous (edge pixels on both sides of every named seam, survivors of the erosion where the
case says so, rectangles where expected, the blob that must vanish does).  No device."""
import time

import numpy as np
import pytest

import front_cases as fc
from front_cases import CASES, BY_NAME

ENTRY_DIM = {"bright": False, "dim": True, "batch": True}
_refs = {}
# the route of a table row's cases where a case names none: the tile list in both modes, and per entry the default front end
ROW_ROUTE = {fc.TILE: dict(dc="tiles"), fc.REACH: dict(dc="tiles"), "workgroup of k_scan_fused": dict(dc="tiles"), fc.HOLES: dict(dc="tiles")}
ENTRY_ROUTE = {"bright": [dict(mode=0, front="prep", spec=(4, 4)), dict(mode=1, front="prep", spec=(4, 4))],
               "dim": [dict(mode=0, front="band", band_rows=12, spec=(9, 9)), dict(mode=1, front="erode", spec=(9, 9))],
               "batch": [dict(mode=0, spec=(9, 9)), dict(mode=1, front="erode", spec=(9, 9))]}


def ref(O, c, entry):
    key = (c.name, ENTRY_DIM[entry])
    if key not in _refs:
        p = c.params(entry)
        p = p[1] if entry == "batch" else p
        t0 = time.perf_counter()
        _refs[key] = fc.reference(O, c.frame, p, ENTRY_DIM[entry])
        _refs[key]["seconds"] = time.perf_counter() - t0
    return _refs[key]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_composed_reference_is_the_oracles_pass(oracle, c):
    """equ, box and found of process_bright / process_dim (want_images) and, for batch cases, detect_frame's record."""
    assert c.frame.size <= fc.MAX_PIXELS and max(c.frame.shape) <= fc.MAX_SIDE
    raw = np.ascontiguousarray(c.frame[::-1])
    for entry in c.entries:
        r = ref(oracle, c, entry)
        assert r["seconds"] < 1.0, (c, entry, r["seconds"])
        if entry == "bright":
            rec, equ, box = oracle.process_bright(raw, c.params(entry), flip=True, want_images=True)
        else:
            pd = c.params(entry)[1] if entry == "batch" else c.params(entry)
            rec, equ, box = oracle.process_dim(raw, pd, flip=True, after_bright=True, want_images=True)
        assert np.array_equal(equ, r["EQU"]) and np.array_equal(box, r["BOX"]), (c, entry)
        assert rec["detection"] == int(r["detection"]), (c, entry)
        if entry == "batch":
            pb, pd = c.params("batch")
            assert oracle.process_bright(raw, pb, flip=True)["found"] == 0          # the bright pass never decides: the dim pass runs
            assert oracle.detect_frame(raw.copy(), pb, pd) == rec, (c, rec)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_route_and_seam(c):
    h, w = c.frame.shape
    assert c.expect or c.row in ROW_ROUTE, c
    # a case without expectations of its own takes its table row's route, in every entry it runs
    for e in c.expect or [dict(ROW_ROUTE[c.row], entry=entry, **more) for entry in c.entries for more in ENTRY_ROUTE[entry]]:
        e = dict(e)
        entry, mode = e.pop("entry"), e.pop("mode")
        p = c.params(entry)
        r = fc.route(h, w, p[1] if entry == "batch" else p, entry, mode, c.knobs)
        for k, v in e.items():
            assert r[k] == v, (c, entry, mode, k, r)
    for kind, i in c.seams:
        assert 0 < i < (h if kind == "row" else w), (c, kind, i)
    if c.row == fc.TILE or c.row == fc.REACH:
        assert all(i % (fc.DCW_TH if kind == "row" else fc.CANNY_TW) == 0 for kind, i in c.seams), c
    if c.row == fc.BAND:
        br = fc.route(h, w, c.params("dim"), "dim", 0, c.knobs)["band_rows"]
        assert br in (6, 12) and all(kind == "row" and i % br == 0 for kind, i in c.seams) and -(-h // br) >= 3 and h % br in (1, 4)
    if c.row == fc.BITS:
        assert w % 64 == 32 and all(kind == "col" and i % 64 == 0 for kind, i in c.seams)
    if c.row == fc.WIDE:
        assert all(i % (fc.MORPH_TH if kind == "row" else fc.MORPH_TW) == 0 for kind, i in c.seams)
    if c.name.startswith("cellword"):
        assert [s for s in c.seams] == [("col", 64 * fc.CELL)] and w // fc.CANNY_TW > 16     # cells 63 | 64: bits 63 of word 0, 0 of word 1
    if c.name == "ballot_half":
        assert -(-w // fc.CANNY_TW) == 65 and c.seams == (("col", 64 * fc.CANNY_TW),)          # tile 64 is lane 0 of the second half
    if c.name.startswith("scan_workgroup"):
        wq = (w + 63) >> 6
        y, q = divmod(fc.SCAN_WORDS_PER_WG, wq)
        assert wq == 5 and 0 < q < wq and y < h - 2 and ("col", 64 * q) in c.seams, (y, q)     # a workgroup boundary inside a bit row


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_no_case_is_vacuous(oracle, c):
    h, w = c.frame.shape
    for entry in c.entries:
        r = ref(oracle, c, entry)
        e = r["CANNY"] != 0
        for kind, i in c.seams:
            lo, hi = (e[i - 2:i], e[i:i + 2]) if kind == "row" else (e[:, i - 2:i], e[:, i:i + 2])
            assert lo.any() and hi.any(), (c, entry, kind, i)
        if ENTRY_DIM[entry]:
            for y, x in c.survivors:
                assert r["ERODED"][y, x] != 0, (c, entry, y, x)
            for y0, y1, x0, x1 in c.vanish:
                assert (r["GRAY"][y0:y1 + 1, x0:x1 + 1] != 0).all() and not r["ERODED"][max(0, y0 - 2):y1 + 3, max(0, x0 - 2):x1 + 3].any(), (c, entry)
        if c.box_expected:
            assert r["BOX"].any() and r["n_boxes"] > 0, (c, entry)
        if c.name != "reach_none":
            assert e.any(), (c, entry)


def test_tile_counts_and_reach(oracle):
    """k_dc_tiles restated: the share cases list exactly the number of tiles they are named for, each reach case lists its
    target tile through one cell only -- the outermost of the reach -- and the dilated feature really enters that tile."""
    for c in CASES:
        if c.ntiles is not None:
            for entry in c.entries:
                r = ref(oracle, c, entry)
                src = r["ERODED"] if ENTRY_DIM[entry] else r["GRAY"]
                if entry == "bright" or c.name.startswith("reach"):
                    assert int(fc.active_tiles(src).sum()) == c.ntiles, (c, entry)
    c = BY_NAME["reach_all"]
    assert fc.active_tiles(ref(oracle, c, "dim")["ERODED"]).all()
    for side in fc.REACH_SPOTS:
        c = BY_NAME[f"reach_{side}"]
        for entry in c.entries:
            r = ref(oracle, c, entry)
            src = r["ERODED"] if ENTRY_DIM[entry] else r["GRAY"]
            ys, xs = np.nonzero(src)
            cells = {(int(y) // fc.CELL, int(x) // fc.CELL) for y, x in zip(ys, xs)}
            want = (1 if "top" in side else 3 if "bottom" in side else 2, 11 if "left" in side else 16 if "right" in side else None)
            assert len(cells) == 1, (c, entry, cells)
            (band, cell), = cells
            assert band == want[0] and (cell == want[1] if want[1] is not None else 12 <= cell <= 15), (c, entry, cells)
            act = fc.active_tiles(src)
            assert act[2, 3] and act.sum() < fc.route(80, 448, c.params("bright"), "bright", 0)["parts"]     # some shares of the list are empty
            tile = (slice(32, 48), slice(192, 256))
            assert r["CANNY"][tile].any() and r["EQU"][tile].any(), (c, entry)
            # a reach one cell shorter on that side would drop the tile
            narrowed = np.zeros_like(act)
            by, bx = -(-80 // fc.CELL), -(-448 // fc.CELL)
            marks = np.zeros((by, bx), bool)
            marks[band, cell] = True
            lo_c, hi_c, lo_b, hi_b = (12 if "left" in side else 11), (15 if "right" in side else 16), (2 if "top" in side else 1), (2 if "bottom" in side else 3)
            narrowed[2, 3] = marks[lo_b:hi_b + 1, lo_c:hi_c + 1].any()
            assert not narrowed[2, 3], (c, entry)


def test_hole_counts(oracle):
    """The ring cases hold exactly the number of holes they are named for (contours of the edge map with a hole flag), on
    either side of FRAME_HOLECAP."""
    for c in CASES:
        if c.holes is None:
            continue
        r = ref(oracle, c, "bright")
        _, flags = oracle.find_contours(r["CANNY"], oracle.RETR_CCOMP)
        assert sum(flags) == c.holes, (c, sum(flags))
        # both borders of every ring are accepted: the count of rectangles (C_NQUADS on the device) moves with every hole
        assert r["BOX"].any() and r["n_boxes"] == 2 * c.holes, (c, r["n_boxes"])
    assert {c.holes for c in CASES if c.holes} >= {fc.FRAME_HOLECAP - 1, fc.FRAME_HOLECAP, fc.FRAME_HOLECAP + 1}
    for entry in ("bright", "dim"):
        r = ref(oracle, BY_NAME["holes_island"], entry)
        cs, flags = oracle.find_contours(r["CANNY"], oracle.RETR_CCOMP)
        # the feature's outer ring (not elongated: refused), its inner ring with the island in its hole, the island's ring:
        # three holes, and the two borders each of the inner ring and of the island are accepted
        assert sum(flags) == 3 and len(cs) == 6 and r["n_boxes"] == 4 and r["BOX"].any(), (entry, len(cs), r["n_boxes"])


def test_bits_frame_has_both_kinds_of_pixels(oracle):
    """dim value == bright value + 1 next to dim value == bright value, inside the blocks of the bit-plane cases."""
    c = BY_NAME["bits_3x3"]
    pd = c.params("batch")[1]
    b = oracle.prep(c.frame, oracle.PREP_BRIGHT).astype(int)
    d = oracle.prep(c.frame, oracle.PREP_BRIGHT_THEN_DIM, False, pd["minFlux"], pd["addFlux"]).astype(int)
    on = b > 0
    assert set(np.unique((d - b)[on])) == {0, 1}
    plus, same = on & (d - b == 1), on & (d == b)
    assert (plus[:, 63] & same[:, 64]).any() or (same[:, 63] & plus[:, 64]).any()                # ... across the word boundary too


def test_every_row_of_the_table_has_a_case():
    rows = {c.row for c in CASES}
    assert len(rows) >= 11 and len(CASES) >= 60
    for name, entry in fc.SEQUENCE_CASES:
        assert entry in BY_NAME[name].entries
    assert fc.RUNCAP_CASE in BY_NAME
    w_max = max(c.frame.shape[1] for c in CASES)
    assert -(-w_max // fc.CANNY_TW) <= 128 and -(-fc.MAX_SIDE // fc.CANNY_TW) <= 128            # no context reaches 129 tile columns
