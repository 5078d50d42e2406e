"""lfdmi_streak_search on the device against the numpy restatement of its definition (tests/streak_ref.py): every integer field
and every bit of the float32 and float64 fields; shapes that are no multiple of the bin, every bin and length, the hand cases
of tests/streak_cases.py, big-endian frames, host, pinned and device frames, a per-frame sigma, the refusals, and one
composition with the masks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_cases as SC  # noqa: E402
import streak_ref as S  # noqa: E402
from test_gpu_radon import dirty_noise  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "found", "q", "s", "r0", "c0", "n_pix")
F32_FIELDS = ("sum", "snr")
F64_FIELDS = ("x1", "y1", "x2", "y2", "rho", "theta")


def same_record(dev, ref):
    for k in INT_FIELDS:
        if int(dev[k]) != int(ref[k]):
            return f"{k}: device {int(dev[k])} != restatement {int(ref[k])}"
    for k in F32_FIELDS:
        if np.float32(dev[k]).tobytes() != np.float32(ref[k]).tobytes():
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in F64_FIELDS:
        if np.float64(dev[k]).tobytes() != np.float64(ref[k]).tobytes():
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    return None


def check(frames, dev, n_dev, sigma=None, **params):
    """every record of every frame, and the counts"""
    bad = []
    for i, f in enumerate(frames):
        sg = S.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[i % np.size(sigma)]
        recs, n = S.rounds(f, sg, **params)
        if n != int(n_dev[i]):
            bad.append((i, f"n_streaks: device {int(n_dev[i])} != restatement {n}"))
        for k, r in enumerate(recs):
            msg = same_record(dev[i, k], r)
            if msg:
                bad.append((i, k, msg))
    assert not bad, bad[:5]


def plant(f, x0, y0, dx, dy, n, amp):
    """add ``amp`` along n unit steps of (dx, dy) from (x0, y0) of the flipped frame"""
    h, w = f.shape
    for t in range(n):
        x, y = int(round(x0 + t * dx)), int(round(y0 + t * dy))
        if 0 <= x < w and 0 <= y < h:
            f[h - 1 - y, x] += np.float32(amp)
    return f


def batch(shape, seed, b, L):
    """dirty noise, the same with a streak of about L b px along x and one along y, and a flat frame of ties"""
    h, w = shape
    n = L * b
    f0 = dirty_noise(shape, seed)
    f1 = plant(dirty_noise(shape, seed + 1), max(0, w // 2 - n // 2), h // 3, 1.0, 0.3, min(n, w), 0.09)
    f2 = plant(dirty_noise(shape, seed + 2), w // 3, max(0, h // 2 - n // 2), -0.2, 1.0, min(n, h), 0.09)
    f3 = np.full(shape, 1.0 / 64, np.float32)
    f3[::3, ::2] = 2.0 / 64
    return np.stack([f0, f1, f2, f3])


CASES = [((70, 90), 1, 8), ((70, 90), 2, 16), ((70, 90), 4, 8), ((131, 77), 1, 32), ((131, 77), 2, 32), ((131, 77), 4, 16),
         ((200, 300), 1, 64), ((200, 300), 2, 32), ((200, 300), 4, 32), ((200, 300), 2, 64), ((131, 77), 1, 16)]


@pytest.mark.parametrize("shape,b,L", CASES, ids=["%dx%d-bin%d-L%d" % (*s, b, L) for s, b, L in CASES])
def test_records_equal_the_restatement(gpu_ctx, shape, b, L):
    from lfd_amd import streaks
    frames = batch(shape, shape[0] + 7 * b + L, b, L)
    keep = frames.copy()
    sigma = np.array([0.025, 0.03, 0.02, 1.0 / 64], np.float32)
    par = {"bin": b, "length": L, "max_streaks": 2, "threshold": 6.0}
    dev, n = streaks.search_frames(gpu_ctx, frames, sigma=sigma, **par)
    assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))              # only read
    assert dev.shape == (4, 2) and dev.dtype == streaks.STREAK_DTYPE and n.dtype == np.int32
    check(frames, dev, n, sigma, **par)
    assert (dev["pad"] == 0).all()


def test_planted_streaks_are_what_is_found(gpu_ctx):
    """the batch's streaks stand above its noise, so the comparison above is about them"""
    from lfd_amd import streaks
    frames = batch((131, 77), 1, 1, 32)
    dev, n = streaks.search_frames(gpu_ctx, frames, bin=1, length=32, max_streaks=1)
    assert dev["found"][:3, 0].tolist() == [0, 1, 1] and dev["q"][1:3, 0].tolist() == [0, 1] and n.tolist()[:3] == [0, 1, 1]


def test_hand_cases(gpu_ctx):
    from lfd_amd import streaks
    for name, f in SC.hand_frames():
        dev, n = streaks.search_frames(gpu_ctx, f[None], sigma=SC.SIGMA, bin=1, length=8, max_streaks=2, peel_halfwidth=1)
        recs, n_ref = S.rounds(f, SC.SIGMA, bin=1, length=8, max_streaks=2, peel_halfwidth=1)
        for k in range(2):
            assert same_record(dev[0, k], recs[k]) is None, (name, k, same_record(dev[0, k], recs[k]))
        assert int(n[0]) == n_ref, name
    f, key = SC.diagonal()
    dev, _ = streaks.search_frames(gpu_ctx, f[None], sigma=SC.SIGMA, bin=1, length=8, max_streaks=1)
    assert (int(dev[0, 0]["q"]), int(dev[0, 0]["s"]), int(dev[0, 0]["r0"]), int(dev[0, 0]["c0"])) == key
    assert same_record(dev[0, 0], SC.expected(key)) is None
    dev, _ = streaks.search_frames(gpu_ctx, SC.half_valid(3)[None], sigma=SC.SIGMA, bin=1, length=8)
    assert dev.shape == (1, 4) and dev[0, 0]["status"] == streaks.NONE
    assert dev[0, 1:].tobytes() == bytes(3 * streaks.STREAK_DTYPE.itemsize)           # later records are all zero
    z = dev[0, 0].copy()
    z["status"] = 0
    assert z.tobytes() == bytes(streaks.STREAK_DTYPE.itemsize)                        # every other field is 0


def test_big_endian_pinned_and_device_frames(gpu_ctx):
    import torch
    from lfd_amd import _native, streaks
    frames = batch((70, 90), 5, 2, 16)
    par = {"bin": 2, "length": 16, "max_streaks": 2, "threshold": 6.0}
    want, n_want = streaks.search_frames(gpu_ctx, frames, **par)
    check(frames, want, n_want, None, **par)
    got, n = streaks.search_frames(gpu_ctx, frames.astype(">f4"), **par)
    assert got.tobytes() == want.tobytes() and n.tolist() == n_want.tolist()
    t = torch.from_numpy(frames).cuda()
    got, n = streaks.search_frames(gpu_ctx, t, **par)
    assert got.tobytes() == want.tobytes() and n.tolist() == n_want.tolist()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), frames.view(np.uint32))
    buf = _native.PinnedBuffer(gpu_ctx, frames.nbytes)
    try:
        pin = buf.array.view(np.float32).reshape(frames.shape)
        pin[...] = frames
        got, n = streaks.search_frames(gpu_ctx, pin, pinned=True, **par)
        assert got.tobytes() == want.tobytes() and n.tolist() == n_want.tolist()
    finally:
        buf.close()


def test_refusals(gpu_ctx):
    from lfd_amd import _native
    f = np.zeros((1, 16, 16), np.float32)
    import test_streak_abi as TA
    for bad in TA.REFUSED:                                            # the library draws the line where ``streaks.as_params`` does
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.streak_search(f, **bad)
        assert e.value.code == _native.ERR_ARG, bad
    for good in TA.TAKEN:
        rec, n = gpu_ctx.streak_search(f, **good)
        assert rec[0, 0]["status"] == _native.STREAK_NONE and n[0] == 0, good
    for sg in (0.0, -1.0, float("nan")):
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.streak_search(f, sigma=sg)
        assert e.value.code == _native.ERR_ARG
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.streak_search(np.zeros((1, 7, 16), np.float32), bin=4)                # h below 2 bin
    assert e.value.code == _native.ERR_ARG
    for shape, b in (((2, 4097), 1), ((8193, 4), 2), ((4, 16385), 4)):                # h or w above 4096 bin: r0, c0 take 12 bits
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.streak_search(np.zeros((1, *shape), np.float32), bin=b, length=8)
        assert e.value.code == _native.ERR_ARG, shape
    rec, n = gpu_ctx.streak_search(np.zeros((1, 2, 4096), np.float32), bin=1, length=8)     # the widest frame that is taken
    assert rec[0, 0]["status"] == _native.STREAK_NONE and n[0] == 0


def test_found_streak_feeds_the_masks(gpu_ctx):
    """inject a 64 px streak, find it, mask it with fill = zero, and search again: nothing is left within L b / 2 px of it"""
    import inject_ref as IR
    from lfd_amd import inject as I
    from lfd_amd import masks, streaks
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (1, 160, 200)).astype(np.float32)
    th = np.radians(115.0)
    x0, y0 = 100.0, 80.0
    tr = np.zeros(1, IR.TRAIL_DTYPE)
    tr[0] = (0, 0, x0 * np.cos(th) + y0 * np.sin(th), th, -32.0 + (-x0 * np.sin(th) + y0 * np.cos(th)),
             32.0 + (-x0 * np.sin(th) + y0 * np.cos(th)), 0.06)
    table, step = I.gaussian_table(1.5)
    frames = IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    rec, n = streaks.search_frames(gpu_ctx, frames)
    assert n[0] >= 1 and rec[0, 0]["found"] == 1
    c, s = np.cos(th), np.sin(th)
    for x, y in ((rec[0, 0]["x1"], rec[0, 0]["y1"]), (rec[0, 0]["x2"], rec[0, 0]["y2"])):
        assert abs(x * c + y * s - tr[0]["rho"]) <= 32.0
    segs = streaks.segments(rec, n)
    assert len(segs) == int(n[0]) and segs.dtype == masks.SEGMENT_DTYPE and (segs["half"] == masks.half_width(float("nan"))).all()
    out = frames.copy()
    gpu_ctx.mask_trails(out, segs, fill="zero")
    rec2, n2 = streaks.search_frames(gpu_ctx, out)
    check(out, rec2, n2)
    for k in range(int(n2[0])):
        mx, my = 0.5 * (rec2[0, k]["x1"] + rec2[0, k]["x2"]), 0.5 * (rec2[0, k]["y1"] + rec2[0, k]["y2"])
        t = -mx * s + my * c
        near = abs(mx * c + my * s - tr[0]["rho"]) <= 32.0 and tr[0]["t0"] - 32.0 <= t <= tr[0]["t1"] + 32.0
        assert not near, (k, rec2[0, k])
