"""The inputs of tests/test_gpu_radon_tiles.py on the CPU: from the restatement alone (tests/radon_lines_ref.py) and from the
launch arithmetic of the host code, every case of tests/radon_tile_cases.py lands on the path of the kernels it is there for --
the number of lines, their orientation pairs, segments that end at, start beyond and lie across column 1024 (and 2048), peels
that change the next round's line, and the tiling facts (slope chunks, RAD_Y blocks, partial records, plane sizes, peel grids).
Also: the restatement's transform, whose diagonal is read as a strided view, against the gather it replaced."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_ref as R  # noqa: E402
import radon_tile_cases as TC  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_radon_model as TM  # noqa: E402

TILE = TC.RADL_TILE
COLUMNS = {
    "second": lambda r, C: r["c1"] >= TILE,
    "straddle": lambda r, C: r["c1"] < TILE <= r["c2"],
    "third": lambda r, C: r["c2"] >= 2 * TILE,
    "last": lambda r, C: r["c2"] == C - 1,
}
# the tiling facts each case is there for, as predicates over launch_facts(): p = the orientation pair of the long axis
FACTS = {
    "W1024": lambda f, p: p["C"] == TILE and p["tiles"] == 1 and p["n"] == 512 and p["chunks"] == 16 and f["peel_vec"] == 8,
    "W1025": lambda f, p: p["C"] == TILE + 1 and p["tiles"] == 2 and p["n"] == 1024 and p["chunks"] == 32 and f["peel_vec"] == 1
    and f["peel_grid"][0] == 5 and p["partials"] > TC.RAD_THREADS,
    "W1025_tie": lambda f, p: p["C"] == TILE + 1 and p["chunks"] == 32 and p["partials"] > TC.RAD_THREADS,
    "W1032_tie": lambda f, p: p["y_blocks"] > 2 and p["partials"] > TC.RAD_THREADS,
    "W1032": lambda f, p: f["peel_vec"] == 8 and p["y_blocks"] > 2 and p["partials"] > TC.RAD_THREADS and p["plane"] > 1 << 22
    and f["frame_elems"] > 1 << 23 and f["pairs"][1]["C"] > 2 * TC.RAD_TT,
    "T1032": lambda f, p: p is f["pairs"][1] and p["C"] == 1032 and p["P"] == 2048 and f["peel_vec"] == 8
    and f["peel_grid"] == (1, 129),
    "W2056": lambda f, p: p["P"] == 4096 and p["tiles"] == 3 and f["peel_vec"] == 8 and f["peel_grid"][0] == 2
    and p["C"] > TC.PEEL_BLOCK and p["plane"] > 1 << 22,
}


def transform_by_gather(Q):
    """radon_ref.transform as it was first written: the right strip's diagonal through an index array"""
    Q = np.asarray(Q)
    Rr, C = Q.shape
    P = R.pow2_at_least(C)
    rows = Rr + P - 1
    F = np.zeros((P, rows, 1), Q.dtype)
    F[:C, P - 1:P - 1 + Rr, 0] = Q.T
    yi = np.arange(rows)[:, None]
    n = 1
    while n < P:
        A = F[0::2]
        B = np.concatenate([F[1::2], np.zeros((P // (2 * n), n + 1, n), Q.dtype)], axis=1)
        t = np.arange(n)[None, :]
        out = np.empty((P // (2 * n), rows, 2 * n), Q.dtype)
        out[:, :, 0::2] = A + B[:, yi + t, t]
        out[:, :, 1::2] = A + B[:, yi + t + 1, t]
        F = out
        n *= 2
    return F[0, :rows, :]


def test_transform_by_view_equals_the_gather_bit_for_bit():
    """on the frames of the existing model tests: the trail set at bins 1 and 2 in all orientations, the brute-force test's
    integer arrays, dirty noise and the smallest frame"""
    arrays = []
    for b in (1, 2):
        V, M = R.prepare(TM.trail_frames()[3], b, R.DEFAULTS["clip"])
        arrays += [R.orient(X, q) for X in (V, M) for q in range(4)]
    for shape in ((24, 32), (37, 50), (5, 3), (1, 1), (300, 70)):
        rng = np.random.default_rng(shape[0])
        arrays += [rng.integers(-9, 10, shape).astype(np.float32), (rng.random(shape) < 0.8).astype(np.int64)]
        arrays += list(R.prepare(TG.dirty_noise(shape, 7), 1, 0.125)) if shape[0] > 1 else []
    for Q in arrays:
        a, b = R.transform(Q), transform_by_gather(Q)
        assert a.dtype == b.dtype == Q.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_lands_on_its_path(name):
    c = TC.CASES[name]
    facts = TC.launch_facts(name)
    h, w = TC.shape(name)
    pair = int(h > w)
    p = facts["pairs"][pair]
    assert FACTS[name](facts, p), facts
    assert c["lines"]["max_lines"] == 3 and c["lines"]["peel_halfwidth"] in (1, 2) and c["params"]["bin"] == 1
    assert c["lines"]["min_seg"] <= c["params"]["min_len"]
    out = TC.records(name)
    assert len(out) == len(c["expect"]["pairs"]) == len(c["sigma"])
    found = []
    for i, ((recs, n_lines), pairs) in enumerate(zip(out, c["expect"]["pairs"])):
        print(name, "frame", i, "n_lines", n_lines,
              [(r["q"], r["y0"], r["s"], "%.2f" % float(r["snr"]), r["c1"], r["c2"], r["seg_n_pix"]) for r in recs])
        assert n_lines == len(pairs)
        assert [r["q"] >> 1 for r in recs[:n_lines]] == list(pairs)
        for r in recs[:n_lines]:
            assert r["status"] == R.OK and r["found"] == 1 and r["seg_n_pix"] >= c["lines"]["min_seg"]
            assert r["n_pix"] >= c["params"]["min_len"] and 0 <= r["c1"] <= r["c2"] < p["C"]
            if c["params"]["threshold"] == 8.0:
                assert float(r["snr"]) >= 8.0
        for a, b in zip(recs[:n_lines], recs[1:n_lines]):          # the peel mattered: the next round's line is another one
            assert (a["q"], a["y0"], a["s"]) != (b["q"], b["y0"], b["s"])
        found += recs[:n_lines]
    for cond in c["expect"]["columns"]:
        assert any(COLUMNS[cond](r, p["C"]) for r in found), cond
    # a segment in the second tile alone needs room for min_seg cells there
    assert ("second" in c["expect"]["columns"]) == (p["C"] >= TILE + c["lines"]["min_seg"]) or name.endswith("_tie")
    assert ("third" in c["expect"]["columns"]) == (p["C"] > 2 * TILE)
    assert len({r["q"] for r in found}) >= (1 if name.endswith("_tie") else 2)       # both orientations of the pair


@pytest.mark.parametrize("name,seed", [("W1024", 1024), ("W1032", 1032), ("T1032", 1034)])
def test_the_noise_alone_stays_below_the_threshold(name, seed):
    """the case's noise without its streaks, at the case's min_len (8 in two of them): nothing passes 8.0"""
    c = TC.CASES[name]
    rec = R.search(TG.dirty_noise(TC.shape(name), seed), c["sigma"][0], **c["params"])
    print(name, "noise snr %.2f" % float(rec["snr"]))
    assert rec["status"] == R.OK and rec["found"] == 0 and float(rec["snr"]) < 8.0


@pytest.mark.parametrize("name,min_blocks", [("W1025_tie", 1), ("W1032_tie", 4)])
def test_tie_frames_are_decided_by_the_tie_rule(name, min_blocks):
    """every round's best score is shared by many lines, so the lowest (q, s, y) is what the record holds; in W1032_tie the
    equal scores sit in several workgroups' partial records of the last level (rows RAD_Y apart, slopes 2 RAD_TT apart)"""
    c = TC.CASES[name]
    (recs, n_lines), = TC.records(name)
    C = TC.shape(name)[1]
    assert n_lines == 3
    assert [(r["q"], r["s"], r["c1"], r["c2"]) for r in recs] == [(0, 0, 0, C - 1)] * 3
    assert len({TG.f32_bits(r["snr"]) for r in recs}) == 1 and [r["y0"] for r in recs] == sorted(r["y0"] for r in recs)
    V, M = R.prepare(TC.frames(name)[0], 1, 0.125)
    S, N = R.transform(V), R.transform(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = (S / (c["sigma"][0] * np.sqrt(N.astype(np.float32)))).astype(np.float32)
    best = np.argwhere((snr == recs[0]["snr"]) & (N >= c["params"]["min_len"]))
    # the last level's workgroup of output (y, s): rows from -(P - 1) in steps of RAD_Y, 2 RAD_TT output slopes each
    blocks = {(int(y) // TC.RAD_Y, int(s) // (2 * TC.RAD_TT)) for y, s in best}
    print(name, "tied lines", len(best), "in", len(blocks), "partial records")
    assert len(best) > 1 and len(blocks) >= min_blocks
    assert len({b[0] for b in blocks}) >= min(2, min_blocks) and len({b[1] for b in blocks}) >= min(2, min_blocks)


def test_plain_record_is_record_zero():
    for name in ("W1024",):
        for f, ref, sg in zip(TC.frames(name), TC.plain(name), TC.CASES[name]["sigma"]):
            assert TG.same_record(R.search(f, sg, **TC.CASES[name]["params"]), ref) is None
