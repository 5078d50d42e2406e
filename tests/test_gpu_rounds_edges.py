"""lfdmi_detect_rounds at its edges: which frames continue (first only, last only, alternating, all, none, n = 1), n = 9 on a
context of 4 frames in flight (round 0 and a later round both chunk), the cap on a three-streak frame, a 373 x 509 frame
(h * w % 4 == 1, width no multiple of the tile) in slot 0 and in a later slot, hand-placed streaks whose bands are near-vertical,
horizontal, through a corner, of zero width and wider than a tile (the detector finds none at theta = 0 exactly).  The gather is checked through the next round's records against the
composition of public calls (tests/rounds_gpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_cases as RC  # noqa: E402
import rounds_gpu as RG  # noqa: E402

from lfd_amd import _native, synth  # noqa: E402

pytestmark = pytest.mark.gpu
WITH, EMPTY = (0, 2), ()


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, *RC.SHAPE, 4)
    yield c
    c.close()


def check(ctx, frames, cats, device=False, **kw):
    import torch
    pb, pd, rs, _ = RG.params()
    want = RG.composed(ctx, frames, cats, **kw)
    arg = torch.from_numpy(frames.copy()).cuda() if device else frames.copy()
    got = ctx.detect_rounds(arg, pb, pd, synth.pack_catalogs(cats) if cats is not None else None, rs if cats is not None else None, **kw)
    print(got[1].tolist(), got[2].tolist())
    assert RG.same(got, want)
    return got


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["first", "last", "alternating", "all", "none", "one"])
def test_which_frames_continue(ctx, layout, device):
    lay = {"first": [WITH, EMPTY, EMPTY], "last": [EMPTY, EMPTY, WITH], "alternating": [WITH, EMPTY, WITH, EMPTY, WITH],
           "all": [WITH, (0,), WITH], "none": [EMPTY, EMPTY], "one": [WITH]}[layout]
    frames, cats = RC.frames(lay)
    rec, nf, dup = check(ctx, frames, cats, device, max_trails=3, half=RC.HALF)
    assert [int(v) > 0 for v in nf] == [bool(w) for w in lay]


def test_nine_frames_on_four_in_flight(ctx):
    frames, cats = RC.frames([WITH, (0,), EMPTY, WITH, (2,), WITH, (0, 1), WITH, WITH])
    rec, nf, dup = check(ctx, frames, cats, True, max_trails=3, half=RC.HALF)
    assert int((nf > 0).sum()) > 4                             # (a later round had more frames than the context takes at once)


def test_the_cap_stops_a_three_streak_frame(ctx):
    frames, cats = RC.frames([(0, 1, 2)])
    rec, nf, dup = check(ctx, frames, cats, max_trails=2, half=RC.HALF)
    assert nf.tolist() == [2] and rec.shape == (1, 2)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_an_odd_frame_in_slot_0_and_in_a_later_slot(device):
    h, w = 373, 509
    assert h * w % 4 == 1
    rng = np.random.default_rng(11)
    frames = (rng.integers(-32768, 32768, (4, h, w)).astype(np.float64) / 65536.0 * 0.1).astype(np.float32)
    for i, streak in enumerate(((250, 180, 1, -1), None, (200, 150, 8, -1), (250, 180, 1, -1))):
        if streak is not None:
            RC.add_streak(frames[i], *streak, 2.0)
    c = _native.Context(0, h, w, 4)
    try:
        rec, nf, dup = check(c, frames, None, device, max_trails=3, half=12.0)
        assert nf[0] > 0 and nf[1] == 0 and nf[3] > 0           # frame 3 goes to slot 1 or 2: another 16 B phase than its source
    finally:
        c.close()


@pytest.mark.parametrize("name", list(RC.BANDS))
def test_hand_placed_bands(ctx, name):
    """The bright streaks of ``rounds_cases.BANDS``, which the detector finds in round 0 (checked on the oracle in
    tests/test_rounds_model.py): round 1 then gathers with a band that is near-vertical, horizontal (nrm.x = 0), through a
    corner of the frame, of zero width, or wider than a tile, and its records must equal the composition's."""
    img, cat, half = RC.band_frame(name)
    for device in (False, True):
        rec, nf, dup = check(ctx, img[None], [cat], device, max_trails=3, half=half)
        assert int(nf[0]) >= 1                                  # round 1 ran: the gather saw this band
        assert round(float(np.degrees(rec[0, 0]["theta"]))) == RC.BANDS[name][2]
