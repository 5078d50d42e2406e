"""The rounds of lfdmi_streak_search (include/lfdmi.h: short-streak search, step 7) against tests/streak_ref.py: two and three
streaks, max_streaks 1, 2 and 8, frames of one call that stop at different rounds (the continuing frames are compacted), a
crossing pair whose second streak loses its middle to the first peel, record 0 against the max_streaks = 1 call, and a call
that splits into chunks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_ref as S  # noqa: E402
from test_gpu_streak import check, plant  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (90, 120)
PAR = {"bin": 1, "length": 16, "peel_halfwidth": 3, "clip": 0.5}      # (the planted pixels stay below the clip)
# (x0, y0, dx, dy, steps, amplitude) of the flipped frame: L cells long, so that a peel leaves no piece behind, and far enough
# apart that no peel touches the next one
STREAKS = ((10, 12, 1.0, 0.25, 16, 0.10), (70, 20, 0.3, 1.0, 16, 0.09), (20, 70, 1.0, -0.4, 16, 0.08))


def frame(seed, n_streaks):
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 0.025, SHAPE).astype(np.float32)
    for st in STREAKS[:n_streaks]:
        plant(f, *st)
    return f


@pytest.mark.parametrize("max_streaks", [1, 2, 8])
def test_two_and_three_streaks(gpu_ctx, max_streaks):
    from lfd_amd import streaks
    frames = np.stack([frame(1, 2), frame(2, 3)])
    dev, n = streaks.search_frames(gpu_ctx, frames, max_streaks=max_streaks, **PAR)
    check(frames, dev, n, None, max_streaks=max_streaks, **PAR)
    assert dev.shape == (2, max_streaks) and n.tolist() == [min(2, max_streaks), min(3, max_streaks)]
    one, n1 = streaks.search_frames(gpu_ctx, frames, max_streaks=1, **PAR)
    assert one[:, 0].tobytes() == dev[:, 0].tobytes() and n1.tolist() == [1, 1]      # record 0 does not depend on max_streaks


def test_frames_stop_at_different_rounds(gpu_ctx):
    """the frames of later rounds are those still going, compacted: 3, 0, 1, 3, 0 and 2 streaks in one call"""
    from lfd_amd import streaks
    counts = (3, 0, 1, 3, 0, 2)
    frames = np.stack([frame(10 + i, c) for i, c in enumerate(counts)])
    dev, n = streaks.search_frames(gpu_ctx, frames, max_streaks=4, **PAR)
    check(frames, dev, n, None, max_streaks=4, **PAR)
    assert n.tolist() == list(counts)
    for i, c in enumerate(n.tolist()):                                # the stopping record, then zeros
        if c < 4:
            assert dev[i, c]["found"] == 0 and dev[i, c + 1:].tobytes() == bytes((3 - c) * streaks.STREAK_DTYPE.itemsize)


def test_crossing_pair(gpu_ctx):
    """two streaks through one point: the first peel takes the second one's middle, and what is left of it is still searched"""
    from lfd_amd import streaks
    rng = np.random.default_rng(5)
    f = rng.normal(0, 0.025, SHAPE).astype(np.float32)
    plant(f, 47, 45, 1.0, 0.0, 16, 0.12)                              # along x through (55, 45)
    plant(f, 55, 37, 0.0, 1.0, 16, 0.10)                              # along y through (55, 45)
    dev, n = streaks.search_frames(gpu_ctx, f[None], max_streaks=4, **PAR)
    check(f[None], dev, n, None, max_streaks=4, **PAR)
    assert n[0] >= 2 and (dev[0, 0]["q"], dev[0, 1]["q"]) == (0, 1)
    assert dev[0, 1]["n_pix"] < 16                                    # its cells under the first footprint count no more


def test_a_call_that_chunks(gpu_ctx):
    from lfd_amd import streaks
    counts = (1, 2, 0, 3, 1)
    frames = np.stack([frame(30 + i, c) for i, c in enumerate(counts)])
    whole, n_whole = streaks.search_frames(gpu_ctx, frames, max_streaks=3, **PAR)
    try:
        gpu_ctx.debug_unit_limits(stage_bytes=2 * frames[0].nbytes)   # two host frames at a time
        dev, n = streaks.search_frames(gpu_ctx, frames, max_streaks=3, **PAR)
        assert gpu_ctx.debug_unit_split()["chunks"] == 3
        gpu_ctx.debug_unit_limits(cell_bytes=8 * SHAPE[0] * SHAPE[1])   # one frame's binned cells at a time
        dev1, n1 = streaks.search_frames(gpu_ctx, frames, max_streaks=3, **PAR)
        assert gpu_ctx.debug_unit_split()["chunks"] == 5
    finally:
        gpu_ctx.debug_unit_limits(forget=True)
    assert dev.tobytes() == whole.tobytes() == dev1.tobytes() and n.tolist() == n_whole.tolist() == n1.tolist()
    check(frames, dev, n, None, max_streaks=3, **PAR)
