"""The frames and parameters of tests/test_gpu_radon_tiles.py, shared with the CPU test of their conditions in
tests/test_radon_tiles_model.py.  Every case is a thin frame whose long axis crosses a tiling constant of the faint-trail
search's kernels (DESIGN.md lists them); `reaches` names what the case is there for and `expect` what the restatement has to
find in it for the case to land there.  All frames are searched at bin 1, so the working arrays are the frames themselves."""
import functools

import numpy as np

import radon_lines_ref as L
import radon_ref as R
import test_gpu_radon as TG

# the kernels' constants as the cases see them (lfd_amd/csrc/radon/k_radon.h, k_radon_lines.h)
RAD_TT, RAD_Y, RAD_THREADS, RADL_TILE, RADL_ROWS, PEEL_BLOCK = 32, 128, 256, 1024, 8, 2048
TIE_SIGMA = 1.0 / 64


def run(f, along, a_lo, a_hi, b_lo, b_hi, amp, add=True):
    """a straight run of the flipped frame: cells a = a_lo .. a_hi of the long axis (along = "x" or "y"), the other
    coordinate going from b_lo to b_hi; amp is added to the pixel, or written over it"""
    h, w = f.shape
    a = np.arange(a_lo, a_hi + 1)
    b = np.rint(b_lo + (a - a_lo) * ((b_hi - b_lo) / max(1, a_hi - a_lo))).astype(int)
    x, y = (a, b) if along == "x" else (b, a)
    if add:
        f[h - 1 - y, x] += np.float32(amp)
    else:
        f[h - 1 - y, x] = np.float32(amp)
    return f


def w1024():
    f = TG.dirty_noise((12, 1024), 1024)
    run(f, "x", 0, 1023, 1, 3, 0.06)            # the whole tile, rising
    run(f, "x", 300, 700, 6, 7, 0.06)           # inside it
    run(f, "x", 800, 1023, 11, 10, 0.08)        # falling, to the tile's last column
    return f[None]


def w1025():
    f = TG.dirty_noise((12, 1025), 1025)
    run(f, "x", 0, 1024, 3, 1, 0.06)            # the first tile and the one column of the second, falling
    run(f, "x", 900, 1024, 6, 7, 0.08)          # ends in the second tile's only column
    run(f, "x", 200, 500, 10, 11, 0.06)         # rising out of the frame
    return f[None]


def w1025_tie():
    return TG.tie_frame((12, 1025))[None]


def w1032_tie():
    return np.full((1, 136, 1032), 1.0 / 32, np.float32)     # every full crossing of every slope and row scores alike


def w1032():
    a = TG.dirty_noise((136, 1032), 1032)
    run(a, "x", 0, 1031, 10, 110, 0.06)         # across every RAD_Y block of the last level
    run(a, "x", 900, 1031, 60, 35, 0.08)        # falling, over column 1024
    run(a, "x", 300, 600, 20, 5, 0.06)          # falling, first tile only
    b = TG.dirty_noise((136, 1032), 1033)
    b[:8] = 0.0                                 # rows y = 128 .. 135 masked: a line along them counts only what is written there
    run(b, "x", 0, 1031, 120, 30, 0.06)         # falling
    run(b, "x", 900, 1031, 20, 25, 0.08)        # over column 1024
    run(b, "x", 1024, 1031, 132, 132, 0.11, add=False)   # eight cells, all of them in the second tile ...
    b[:8, 1023] = -0.05                         # ... and a negative column before them: the segment starts at 1024
    return np.stack([a, b])


def t1032():
    f = TG.dirty_noise((1032, 16), 1034)
    f[:, 12:] = 0.0                             # columns x = 12 .. 15 masked
    run(f, "y", 0, 1031, 1, 6, 0.06)            # orientation 2, across all 129 row blocks of the peel
    run(f, "y", 900, 1031, 10, 9, 0.08)         # orientation 3, over working column 1024
    run(f, "y", 1024, 1031, 14, 14, 0.11, add=False)     # eight cells, all of them in the second tile ...
    f[1032 - 1 - 1023, 12:] = -0.05             # ... and a negative row before them: the segment starts at 1024
    return f[None]


def w2056():
    f = TG.dirty_noise((8, 2056), 2056)
    run(f, "x", 0, 2055, 0, 2, 0.06)            # three tiles of the extent, two column blocks of the peel
    run(f, "x", 900, 1150, 4, 4, 0.08)          # over column 1024
    run(f, "x", 1040, 1220, 7, 7, 0.08)         # second tile only
    return f[None]


def case(make, reaches, sigma, min_len, min_seg, halfwidth, expect, threshold=8.0):
    return {"make": make, "reaches": reaches, "sigma": np.asarray(sigma, np.float32),
            "params": {"bin": 1, "min_len": min_len, "threshold": threshold},
            "lines": {"max_lines": 3, "peel_halfwidth": halfwidth, "min_seg": min_seg}, "expect": expect}


# expect: per frame, the orientation pair (0: q = 0, 1; 1: q = 2, 3) of every line the restatement has to find, and the column
# conditions some record of the case has to meet ("second": c1 >= 1024, "straddle": c1 < 1024 <= c2, "last": c2 = C - 1,
# "third": c2 >= 2048).  A segment in the second tile alone needs C >= 1024 + min_seg, so W1024 and W1025 cannot have one.
CASES = {
    "W1024": case(w1024, "C = RADL_TILE exactly; levels to n = 512, 16 slope chunks; 16-byte peel", [0.025], 128, 32, 1,
                  {"pairs": [(0, 0, 0)], "columns": ("last",)}),
    "W1025": case(w1025, "C one past a tile; P = 2048, last level n = 1024 with 32 chunks; scalar peel, five workgroups in x",
                  [0.025], 128, 32, 1, {"pairs": [(0, 0, 0)], "columns": ("straddle", "last")}),
    "W1025_tie": case(w1025_tie, "equal scores across the partial records and the tiles of W1025", [TIE_SIGMA], 128, 32, 1,
                      {"pairs": [(0, 0, 0)], "columns": ("straddle", "last")}, threshold=-1e30),
    "W1032_tie": case(w1032_tie, "equal scores in many partial records: other RAD_Y blocks, other slope chunks", [TIE_SIGMA], 1032, 32,
                      1, {"pairs": [(0, 0, 0)], "columns": ("straddle", "last")}, threshold=-1e30),
    "W1032": case(w1032, "16-byte peel; several RAD_Y blocks; the second frame's planes past 2^23 elements; over 256 partial "
                  "records per orientation", [0.025, 0.025], 8, 8, 2,
                  {"pairs": [(0, 0, 0), (0, 0, 0)], "columns": ("second", "straddle", "last")}),
    "T1032": case(t1032, "tall: orientations 2, 3 have C = 1032, P = 2048; 16-byte peel over 129 row blocks; extent by columns of V",
                  [0.025], 8, 8, 1, {"pairs": [(1, 1, 1)], "columns": ("second", "straddle", "last")}),
    "W2056": case(w2056, "P = 4096; 16-byte peel with two workgroups in x; extent over three tiles", [0.025], 1024, 32, 1,
                  {"pairs": [(0, 0, 0)], "columns": ("second", "straddle", "third", "last")}),
}


@functools.lru_cache(maxsize=None)
def frames(name):
    """the frames of a case [n, h, w]: built once, shared, never changed"""
    f = np.ascontiguousarray(CASES[name]["make"](), np.float32)
    f.setflags(write=False)
    return f


def shape(name):
    return frames(name).shape[1:]


@functools.lru_cache(maxsize=None)
def records(name):
    """the restatement's (records, n_lines) of every frame of a case, computed once"""
    c = CASES[name]
    return tuple(L.search_lines(f, c["sigma"][i], **c["params"], **c["lines"]) for i, f in enumerate(frames(name)))


@functools.lru_cache(maxsize=None)
def plain(name):
    """the restatement's plain search of every frame of a case: record 0 of records() without its segment"""
    return tuple({k: recs[0][k] for k in TG.INT_FIELDS + TG.F32_FIELDS + TG.F64_FIELDS} for recs, _ in records(name))


def launch_facts(name):
    """how the kernels tile a case, restated from the host code (lfd_amd/csrc/radon/radon.hip): per orientation pair the last
    level's input width n, its slope chunks, its RAD_Y blocks and partial records; the plane elements of a frame; the peel's
    vector width and grid; the extent's tiles per pair"""
    h, w = shape(name)
    out = {"pairs": [], "peel_vec": 8 if w % 8 == 0 else 1}
    elems = 0
    for Rr, C in ((h, w), (w, h)):
        P = R.pow2_at_least(C)
        n = P // 2
        tt = min(RAD_TT, n)
        yblocks = -(-(Rr + P - 1) // RAD_Y)
        out["pairs"].append({"R": Rr, "C": C, "P": P, "n": n, "chunks": n // tt, "y_blocks": yblocks,
                             "partials": yblocks * (P // (2 * tt)), "plane": (Rr + P - 1) * P, "tiles": -(-C // RADL_TILE)})
        elems += 2 * (-(-((Rr + P - 1) * P) // 64) * 64)
    out["frame_elems"] = elems
    out["peel_grid"] = (-(-w // (RAD_THREADS * out["peel_vec"])), -(-h // RADL_ROWS))
    return out
