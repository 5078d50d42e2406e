"""lfdmi_stack_profiles on the device against the numpy restatement (tests/stack_ref.py), bit for bit and with nothing left out:
every field of every record, the rows, the raw sums and counts, NaN positions and the sign of zero -- over both major axes and
slope signs, segments that leave the frame, dirty pixels on the band, the three bin steps, both byte orders, host, pinned and
device frames, many segments per call, and a row through the defocus fit."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import stack_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = {"prof_half": 10.0, "wing": 3, "min_cols": 16, "max_shift": 4.0}


def bits64(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def same(i, dev, row, A, N, ref):
    """None, or how segment i's device result differs from the restatement's (rec, row, A, N)"""
    rrec, rrow, rA, rN = ref
    for k in S.INT_FIELDS:
        if int(dev[k]) != int(rrec[k]):
            return f"segment {i}: {k}: device {int(dev[k])} != restatement {int(rrec[k])}"
    for k in S.F64_FIELDS:
        a, b = float(dev[k]), float(rrec[k])
        if not (math.isnan(a) and math.isnan(b)) and bits64(a) != bits64(b):
            return f"segment {i}: {k}: device {a!r} != restatement {b!r}"
    if not np.array_equal(np.isnan(row), np.isnan(rrow)):
        return f"segment {i}: NaN positions of the row differ"
    ok = ~np.isnan(rrow)
    if not np.array_equal(row[ok].view(np.uint32), rrow[ok].view(np.uint32)):
        return f"segment {i}: row differs at bins {np.nonzero(row.view(np.uint32) != rrow.view(np.uint32))[0][:5]}"
    if not np.array_equal(A.view(np.uint32), rA.view(np.uint32)):
        return f"segment {i}: sums differ at {np.argwhere(A.view(np.uint32) != rA.view(np.uint32))[:5].tolist()}"
    if not np.array_equal(N, rN) or N.dtype != np.int32:
        return f"segment {i}: counts differ at {np.argwhere(N != rN)[:5].tolist()}"
    return None


def check(frames, segs, dev, sigma=None, **params):
    """a whole call (records, rows, sums, counts) against the restatement; returns its records"""
    rec, rows, A, N = dev
    frames = np.asarray(frames)
    assert rec.shape == (len(segs),) and rows.shape == (len(segs), S.n_bins(params)) and A.shape == N.shape == (len(segs), 2, rows.shape[1])
    bad, refs = [], []
    for i, s in enumerate(segs):
        sg = S.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[int(s["frame"]) % np.size(sigma)]
        ref = S.measure(frames[int(s["frame"])], (s["x1"], s["y1"], s["x2"], s["y2"]), sg, **params)
        refs.append(ref[0])
        msg = same(i, rec[i], rows[i], A[i], N[i], ref)
        if msg:
            bad.append(msg)
    assert not bad, bad[:5]
    return refs


def trail_frame(shape, seed, x0, y0, deg, peak=0.05, sigma_px=1.5):
    """noise of sigma 0.025 with a Gaussian trail through (x0, y0) whose normal points along ``deg`` degrees"""
    from lfd_amd import inject as I
    f = np.random.default_rng(seed).normal(0, 0.025, (1, *shape)).astype(np.float32)
    th = math.radians(deg)
    table, step = I.gaussian_table(sigma_px)
    tr = IR.trail(rho=x0 * math.cos(th) + y0 * math.sin(th), theta=th, amplitude=peak)
    return IR.inject(f, [tr], I.normalise_peak(table).astype(np.float32), step)[0]


def dirty(f, seed):
    """NaN, +-inf, +-0 and pixels above the clip scattered over the frame (so also on every band)"""
    rng = np.random.default_rng(seed)
    flat = f.reshape(-1)
    for val in (np.nan, np.inf, -np.inf, 0.0, -0.0, 0.3, -0.5, 0.125, np.nextafter(np.float32(0.125), np.float32(1))):
        flat[rng.choice(flat.size, flat.size // 60, replace=False)] = val
    return f


def line_through(x0, y0, deg, shape, t0=-400.0, t1=400.0):
    """(x1, y1, x2, y2) of the line through (x0, y0) with normal angle ``deg``, from t0 to t1 along it"""
    th = math.radians(deg)
    c, s = math.cos(th), math.sin(th)
    return x0 - t0 * s, y0 + t0 * c, x0 - t1 * s, y0 + t1 * c


def segment_set(shape):
    """segments over one h x w frame (frame 0 carries a trail at 100 degrees through the middle, frame 1 at 20 degrees)"""
    from lfd_amd import stack
    h, w = shape
    mx, my = w / 2, h / 2
    rows = [
        (0, *line_through(mx + 0.8, my + 1.1, 100.3, shape)),       # x-major, rising; end points outside the frame; near the trail
        (0, *line_through(mx, my, 80, shape)),                      # x-major, falling
        (1, *line_through(mx - 0.7, my + 0.9, 19.7, shape)),        # y-major, near frame 1's trail
        (1, *line_through(mx, my, 160, shape)),                     # y-major, other slope sign
        (0, 3.0, my, w - 4.0, my),                                  # exactly horizontal, integer end points
        (1, mx + 0.25, 2.5, mx + 0.25, h - 3.5),                    # exactly vertical
        (0, 5.0, 5.0, 85.0, 85.0),                                  # |dx| = |dy|: x-major by the tie rule
        (1, 90.0, 6.0, 10.0, 86.0),                                 # |dx| = |dy|, falling
        (0, 2.0, 3.0, w - 2.0, 9.0),                                # the band leaves the frame below ...
        (0, 2.0, h - 2.0, w - 2.0, h - 6.0),                        # ... and above
        (1, 2.5, 4.0, 7.0, h - 4.0),                                # ... and to the left (y-major)
        (0, 37.5, my - 3, 71.2, my + 4),                            # starts and ends mid-block, the midpoint inside a block
        (1, mx, 33.0, mx + 5, 95.9),                                # the same, y-major
        (0, 70.0, 20.0, 6.4, 31.0),                                 # given right to left
        (0, mx, my, mx, my),                                        # BAD_SEGMENT: coincident
        (1, math.nan, 0.0, 50.0, 50.0),                             # BAD_SEGMENT: not finite
        (0, 10.0, 10.0, 20.0, 12.0),                                # TOO_SHORT
        (1, -300.0, 10.0, -100.0, 50.0),                            # TOO_SHORT: no column in the frame
    ]
    return stack.segments(rows)


def two_frames(shape):
    h, w = shape
    return np.stack([dirty(trail_frame(shape, 11 + h, w / 2, h / 2, 100), 5), dirty(trail_frame(shape, 12 + h, w / 2, h / 2, 20), 6)])


@pytest.mark.parametrize("step", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("shape", [(97, 130), (130, 97)], ids=["97x130", "130x97"])
def test_segments_equal_the_restatement(gpu_ctx, shape, step):
    frames = two_frames(shape)
    keep = frames.copy()
    segs = segment_set(shape)
    sigma = np.array([0.025, 0.03], np.float32)
    for n_iter in (0, 2):
        kw = dict(SMALL, step=step, n_iter=n_iter)
        dev = gpu_ctx.stack_profiles(frames, segs, sigma=sigma, raw=True, **kw)
        refs = check(frames, segs, dev, sigma, **kw)
        assert [r["status"] for r in refs[-4:]] == [S.BAD_SEGMENT, S.BAD_SEGMENT, S.TOO_SHORT, S.TOO_SHORT]
        assert all(r["status"] in (S.OK, S.TOO_FAINT) for r in refs[:-4])
        assert max(r["n_pass"] for r in refs) == n_iter + 1 and (n_iter == 0 or min(r["n_pass"] for r in refs[:-4]) == 1)
    assert refs[0]["status"] == S.OK and refs[2]["status"] == S.OK and abs(refs[0]["shift"]) > 0.4       # the trails, refined
    assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))                      # only read
    plain = gpu_ctx.stack_profiles(frames, segs, sigma=sigma, **kw)
    assert np.array_equal(plain[0].tobytes(), dev[0].tobytes()) and np.array_equal(plain[1].view(np.uint32), dev[1].view(np.uint32))


def test_defaults_clip_and_byte_orders_from_host_pinned_and_device(gpu_ctx):
    import torch
    from lfd_amd import _native
    shape = (97, 130)
    frames = two_frames(shape)
    segs = segment_set(shape)[:8]
    host = gpu_ctx.stack_profiles(frames, segs, raw=True, min_cols=16)                       # the default band: 2 * 24 px of 97
    check(frames, segs, host, min_cols=16)
    noclip = gpu_ctx.stack_profiles(frames, segs, raw=True, min_cols=16, clip=np.inf)
    check(frames, segs, noclip, min_cols=16, clip=np.inf)
    assert not np.array_equal(noclip[3], host[3])

    def equal(got):
        return all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(got, host))
    be = frames.astype(">f4")
    assert equal(gpu_ctx.stack_profiles(be, segs, raw=True, min_cols=16))
    assert np.array_equal(be.view(np.uint32), frames.astype(">f4").view(np.uint32))
    pin = gpu_ctx.pinned_buffer(frames.nbytes)
    pv = pin.array.view("<f4").reshape(frames.shape)
    pv[:] = frames
    assert equal(gpu_ctx.stack_profiles(pv, segs, raw=True, pinned=True, min_cols=16))
    pb = pin.array.view(">f4").reshape(frames.shape)
    pb[:] = frames
    assert equal(gpu_ctx.stack_profiles(pb, segs, raw=True, pinned=True, min_cols=16))
    pin.close()
    dev = torch.from_numpy(frames).cuda()
    assert equal(gpu_ctx.stack_profiles(dev, segs, raw=True, min_cols=16))
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), frames.view(np.uint32))
    dev_be = torch.from_numpy(be.view(np.uint8).reshape(2, -1).copy()).cuda()
    assert equal(gpu_ctx.stack_profiles(_native.DeviceFrames(dev_be.data_ptr(), (2, *shape)), segs, raw=True, min_cols=16))
    assert np.array_equal(dev_be.cpu().numpy().reshape(-1), be.view(np.uint8).reshape(-1))


def test_many_segments_none_and_a_frame_without_one(gpu_ctx):
    from lfd_amd import _native, stack
    shape = (130, 97)
    frames = np.concatenate([two_frames(shape), dirty(trail_frame(shape, 3, 40, 70, 140), 9)[None]])
    rng = np.random.default_rng(300)
    rows = []
    for i in range(300):                                                  # frame 1 gets none
        x0, y0, deg = rng.uniform(5, shape[1] - 5), rng.uniform(5, shape[0] - 5), rng.uniform(0, 180)
        rows.append(((0, 2)[i % 2], *line_through(x0, y0, deg, shape, -rng.uniform(3, 200), rng.uniform(3, 200))))
    segs = stack.segments(rows)
    kw = dict(SMALL, n_iter=1)
    refs = check(frames, segs, gpu_ctx.stack_profiles(frames, segs, raw=True, **kw), **kw)
    assert {r["status"] for r in refs} == {S.OK, S.TOO_FAINT, S.TOO_SHORT}
    rec, rows_, A, N = gpu_ctx.stack_profiles(frames, segs[:0], raw=True, **kw)
    assert rec.shape == (0,) and rows_.shape == (0, S.n_bins(kw)) and A.shape == (0, 2, S.n_bins(kw))
    for bad in ({"step": 0.7}, {"wing": 10}, {"n_iter": -1}, {"prof_half": 40.0}, {"min_cols": 1}, {"clip": 0.0}):
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.stack_profiles(frames, segs[:2], **dict(SMALL, **bad))
        assert e.value.code == _native.ERR_ARG
    for kwargs in ({"sigma": 0.0}, {"sigma": [0.02, -1.0, 0.02]}):
        with pytest.raises(_native.NativeError):
            gpu_ctx.stack_profiles(frames, segs[:2], **SMALL, **kwargs)
    wrong = segs[:2].copy()
    wrong["frame"][1] = 3
    with pytest.raises(_native.NativeError):
        gpu_ctx.stack_profiles(frames, wrong, **SMALL)
    check(frames, segs[:3], gpu_ctx.stack_profiles(frames, segs[:3], raw=True, **kw), **kw)   # the context stays usable


def test_calls_in_flight_refuse_the_measurement():
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (97, 130)
    frames = two_frames(shape)
    with _native.Context(0, *shape, 2) as ctx:
        pb, pd, _ = default_params()
        dev = torch.zeros((2, *shape), dtype=torch.float32, device="cuda")
        pend = ctx.detect_batch_begin(dev, pb, pd)
        with pytest.raises(_native.NativeError) as e:
            ctx.stack_profiles(frames, segment_set(shape)[:2], **SMALL)
        assert e.value.code == _native.ERR_ARG
        pend.result()
        ctx.stack_profiles(frames, segment_set(shape)[:2], **SMALL)


def test_one_full_crossing_of_an_sdss_frame_and_its_defocus_fit(gpu_ctx):
    from lfd_amd import _native, defocus, stack
    shape = (1489, 2048)
    frame = trail_frame(shape, 7, 1000.0, 700.0, 110.0, peak=0.05, sigma_px=2.0)[None]
    segs = stack.segments([(0, *line_through(1000.8, 701.0, 110.1, shape, -3000.0, 3000.0))])
    dev = gpu_ctx.stack_profiles(frame, segs, raw=True)
    ref = check(frame, segs, dev)[0]
    assert ref["status"] == S.OK and ref["n_col"] == 2048 and ref["n_pass"] == 3 and 3.0 <= ref["fwhm"] <= 5.5
    rec, rows = dev[:2]
    trails = stack.to_trails(rec)
    with defocus.DefocusBank(gpu_ctx, heights=[80.0, 100.0, 150.0], radii=[0.0, 1.0], seeings=[1.0, 1.4, 1.8, 2.2], prof_half=24.0,
                             prof_step=0.5, wing=8) as bank:
        assert bank.n_bins == rows.shape[1]
        fit = gpu_ctx.fit_defocus(bank, trails, rows)
    assert fit["status"][0] == _native.DEFOCUS_OK and fit["amplitude"][0] > 0
