"""lfdmi_streak_search where k_streak_search re-tiles: working arrays one tile wide and tall, minus one, exact and plus one (in
cells and in anchors), the best segment anchored at the last anchor of a tile, the first of the next and the last one of the
array, a best segment that lies in its anchor's halo, and equal patterns in two tiles, whose tie crosses workgroups.  All at
bin 1, so the working arrays are the flipped frames; every record equals tests/streak_ref.py in every field."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_cases as SC  # noqa: E402
import streak_ref as S  # noqa: E402
from test_gpu_radon import dirty_noise  # noqa: E402
from test_gpu_streak import check, same_record  # noqa: E402

pytestmark = pytest.mark.gpu

L = 8
PAR = {"bin": 1, "length": L, "max_streaks": 1}


def tile():
    from lfd_amd import streaks
    tr, tc = streaks.tile()
    assert (tr, tc) == (16, 64)                                       # the cases below are laid out for these
    return tr, tc


def segment_frame(shape, keys, amp=SC.AMP):
    """a floor of BG with the segments (q, s, r0, c0) written in AMP"""
    f = np.full(shape, SC.BG, np.float32)
    for q, s, r0, c0 in keys:
        cells = [(r0 + S.off(i, s, L), c0 + i) for i in range(L)]
        SC.put(f, cells if q == 0 else [(c, r) for r, c in cells], amp)
    return f


def key_of(rec):
    return tuple(int(rec[k]) for k in ("q", "s", "r0", "c0"))


def test_sizes_around_one_tile(gpu_ctx):
    from lfd_amd import streaks
    tr, tc = tile()
    sizes = [(tr + dh, tc + dw) for dh in (-1, 0, 1) for dw in (-1, 0, 1)]
    sizes += [(tr + dh, tc + L - 1 + dw) for dh in (-1, 1) for dw in (-1, 0, 1)]       # tc - 1, tc, tc + 1 anchors along a row
    sizes += [(tc + L - 1 + d, 7) for d in (-1, 0, 1)]                                # q = 1 only, its anchors around a tile
    for k, shape in enumerate(sizes):
        frames = np.stack([dirty_noise(shape, 100 + k), dirty_noise(shape, 200 + k)])
        dev, n = streaks.search_frames(gpu_ctx, frames, threshold=3.0, **dict(PAR, max_streaks=2))
        check(frames, dev, n, None, threshold=3.0, **dict(PAR, max_streaks=2))


@pytest.mark.parametrize("q", [0, 1])
def test_best_segment_at_the_seams_of_the_tiles(gpu_ctx, q):
    from lfd_amd import streaks
    tr, tc = tile()
    R, C = 2 * tr + 3, 2 * tc + 5                                    # working rows and columns: 35 x 133
    shape = (R, C) if q == 0 else (C, R)
    keys = [(q, 0, tr - 1, tc - 1), (q, 0, tr, tc), (q, 2, tr - 1, tc), (q, -2, tr, tc - 1), (q, 0, R - 1, C - L), (q, -3, R - 1, C - L),
            (q, 3, R - 4, C - L), (q, 0, 0, 0), (q, L - 2, 0, C - L), (q, -(L - 2), R - 1, 0)]
    frames = np.stack([segment_frame(shape, [k]) for k in keys])
    dev, n = streaks.search_frames(gpu_ctx, frames, sigma=SC.SIGMA, **PAR)
    for i, k in enumerate(keys):
        assert key_of(dev[i, 0]) == k, (k, key_of(dev[i, 0]))
        assert same_record(dev[i, 0], SC.expected(k)) is None
    check(frames, dev, n, SC.SIGMA, **PAR)


def test_best_segment_in_the_halo(gpu_ctx):
    """anchored in a tile's corner cell, every other cell of the segment lies outside the tile's own anchors: above and to the
    right (s = 7 from the last row and column), and below (s = -7 from the first row of the second tile row)"""
    from lfd_amd import streaks
    tr, tc = tile()
    shape = (2 * tr + 3, 2 * tc + 9)
    keys = [(0, 7, tr - 1, tc - 1), (0, -7, tr, tc - 1), (0, 7, tr - 1, 2 * tc - 1), (0, -7, tr, 0)]
    frames = np.stack([segment_frame(shape, [k]) for k in keys])
    dev, n = streaks.search_frames(gpu_ctx, frames, sigma=SC.SIGMA, **PAR)
    for i, k in enumerate(keys):
        assert key_of(dev[i, 0]) == k
        assert same_record(dev[i, 0], SC.expected(k)) is None
    check(frames, dev, n, SC.SIGMA, **PAR)


def test_equal_patterns_in_two_tiles_tie_across_workgroups(gpu_ctx):
    from lfd_amd import streaks
    tr, tc = tile()
    shape = (2 * tr + 3, 2 * tc + 5)
    cases = [([(0, 2, 3, 5), (0, 2, 3 + tr, 5 + tc)], (0, 2, 3, 5)),                  # the lower r0 wins
             ([(0, 2, 3 + tr, 5), (0, 2, 3, 5 + tc)], (0, 2, 3, 5 + tc)),             # r0 before c0
             ([(0, 2, 3, 5 + tc), (0, -2, 3 + tr, 5)], (0, -2, 3 + tr, 5)),           # s before r0
             ([(0, 0, 20, 70), (1, 0, 100, 3)], (0, 0, 20, 70))]                      # q before everything
    frames = np.stack([segment_frame(shape, keys) for keys, _ in cases])
    dev, n = streaks.search_frames(gpu_ctx, frames, sigma=SC.SIGMA, **PAR)
    for i, (_, want) in enumerate(cases):
        assert key_of(dev[i, 0]) == want, (want, key_of(dev[i, 0]))
        assert same_record(dev[i, 0], SC.expected(want)) is None
    check(frames, dev, n, SC.SIGMA, **PAR)
    flat = np.full((1, *shape), 1.0 / 64, np.float32)                 # every segment of every tile scores alike
    dev, n = streaks.search_frames(gpu_ctx, flat, sigma=SC.SIGMA, **PAR)
    assert key_of(dev[0, 0]) == (0, -(L - 1), L - 1, 0)
    check(flat, dev, n, SC.SIGMA, **PAR)
