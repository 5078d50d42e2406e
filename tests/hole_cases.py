"""Frames for the hole-pruning tests of k_frame_contours (tests/test_gpu_hole_prune.py): plateaus on a blank frame, whose
Canny edges are closed rings -- every plateau is an edge component with one hole (its inside), roundish or elongated."""
import numpy as np

import front_cases as fc

C_NKEYS, C_NSLOTS, C_NHOLES, C_NHOLES_PRUNED = 0, 1, 20, 21     # LFDMI_COUNTERS slots the tests read


def f_mixed(h, w, seed):
    """Squares (roundish holes), bars (slits), a nested ring, an elongated ring with an island, a square at the right and one at
    the bottom edge of the frame, and features across column 64 / 128 / 192 / 256 (the words of the bit rows)."""
    f = fc.blank(h, w, seed)
    A = fc.AMPS
    y, i = 3, 0
    while y + 12 < h:
        x = 3 + (i % 3) * 5
        while x + 14 < w:
            kind = (i + x // 7) % 4
            if kind == 0:
                fc.box(f, y, y + 4, x, x + 4, A[i % 4])                 # a square: one roundish hole
                x += 14
            elif kind == 1:
                fc.box(f, y + 2, y + 2, x, x + 21, A[(i + 1) % 4])      # a bar: dilated, a 25 x 4 ring with a slit inside
                x += 31
            elif kind == 2:
                fc.box(f, y, y + 7, x, x + 9, A[(i + 2) % 4])           # a plateau with a higher one inside: nested rings
                fc.box(f, y + 3, y + 4, x + 3, x + 6, A[(i + 3) % 4] + 30.0)
                x += 19
            else:
                fc.box(f, y, y + 1, x, x + 8, A[(i + 3) % 4])           # an L: a hole that is neither
                fc.box(f, y, y + 7, x, x + 1, A[(i + 3) % 4])
                x += 18
            i += 1
        y += 14
    fc.box(f, h - 5, h - 1, 8, 12, A[0])                              # reaches the last row
    fc.box(f, 20, 24, w - 3, w - 1, A[1])                             # reaches the last column
    return f


def f_island(h, w, seed):
    """Hollow frames with islands inside: an elongated one (kept) and a square one (rejected), beside squares."""
    f = fc.blank(h, w, seed)
    A = fc.AMPS
    fc.hollow(f, 4, 27, 6, w - 8, 5, A[1])
    fc.box(f, 15, 16, 30, w - 40, A[3])                               # a long island
    fc.hollow(f, 34, 59, 50, 75, 5, A[2])
    fc.box(f, 45, 47, 61, 63, A[0])                                   # a small island
    for k in range(6):
        fc.box(f, 36 + (k % 2) * 10, 41 + (k % 2) * 10, 90 + 12 * k, 95 + 12 * k, A[k % 4])
    return f


def f_slit_in_blob(h, w, seed):
    """A square plateau in two levels, the step three columns from its right side: the edge component is the square's ring
    with a wall across it, its outer border a square (rejected), the hole left of the wall a square too, the hole right of
    the wall a slit -- the frame's only acceptable rectangle is that hole border's."""
    f = fc.blank(h, w, seed)
    fc.box(f, 8, 51, 40, 86, fc.AMPS[0])
    fc.box(f, 8, 51, 87, 88, fc.AMPS[3])
    return f


def f_many(h=400, w=1440, n=1600):
    """n features on the pitch of front_cases.f_rings, bars and 3 x 3 squares in turn: more holes than the hole table of
    k_frame_contours holds, half of them elongated (kept), half roundish (rejected)."""
    per = w // fc.RING_PITCH_X
    f = fc.blank(h, w, 77)
    for i in range(n):
        y, x = 4 + fc.RING_PITCH_Y * (i // per), 6 + fc.RING_PITCH_X * (i % per)
        if (i + i // per) % 2:
            f[y, x:x + fc.RING_LEN] = fc.AMPS[i % 4]
        else:
            f[y - 1:y + 2, x + 4:x + 7] = fc.AMPS[i % 4]
    return f


FRAMES = {
    "mixed_64x192": lambda: f_mixed(64, 192, 31),
    "mixed_130x257": lambda: f_mixed(130, 257, 32),
    "island_64x192": lambda: f_island(64, 192, 33),
    "slit_in_blob_64x192": lambda: f_slit_in_blob(64, 192, 34),
    "slit_in_blob_130x257": lambda: f_slit_in_blob(130, 257, 35),
}
