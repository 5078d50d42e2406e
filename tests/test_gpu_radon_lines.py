"""lfdmi_radon_search_lines on the device against the numpy restatement of steps 7 - 9 (tests/radon_lines_ref.py): every integer
field, the float32 bits of sum, snr, seg_sum and seg_snr and n_lines exactly, the doubles to 1e-12; frames that leave at
different rounds through a handle of two slots, the rest of the search's contract, the CPU test's two-trail frames and
DetectTrails(radon=True, radon_lines=K) end to end."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_radon_lines_abi as TA  # noqa: E402
import test_radon_lines_model as TL  # noqa: E402
import test_radon_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = TG.INT_FIELDS + ("c1", "c2", "seg_n_pix")
F32_FIELDS = TG.F32_FIELDS + ("seg_sum", "seg_snr")
F64_FIELDS = TG.F64_FIELDS + ("ex1", "ey1", "ex2", "ey2")


def same_line(dev, ref):
    for k in INT_FIELDS:
        if int(dev[k]) != int(ref[k]):
            return f"{k}: device {int(dev[k])} != restatement {int(ref[k])}"
    for k in F32_FIELDS:
        if TG.f32_bits(dev[k]) != TG.f32_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in F64_FIELDS:
        a, b = float(dev[k]), float(ref[k])
        if abs(a - b) > 1e-12 * abs(b):
            return f"{k}: device {a!r} != restatement {b!r}"
    return None if int(dev["pad"]) == 0 else "pad is not zero"


def check_lines(frames, dev, dev_n, sigma=None, **params):
    """every record of every frame against the restatement; returns the restatement's n_lines"""
    bad, counts = [], []
    for i, f in enumerate(frames):
        sg = R.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[i % np.size(sigma)]
        recs, n_lines = L.search_lines(f, sg, **params)
        counts.append(n_lines)
        if int(dev_n[i]) != n_lines:
            bad.append((i, f"n_lines: device {int(dev_n[i])} != restatement {n_lines}"))
        for k, ref in enumerate(recs):
            msg = same_line(dev[i, k], ref)
            if msg:
                bad.append((i, k, msg))
    assert not bad, bad[:5]
    return counts


SHAPES = [((5, 3), 1, 0), ((5, 3), 1, 1), ((37, 50), 1, 3), ((37, 50), 2, 3), ((97, 161), 4, 8), ((70, 300), 1, 2), ((300, 70), 1, 2)]


@pytest.mark.parametrize("shape,b,halfwidth", SHAPES, ids=["%dx%d-bin%d-hw%d" % (*s, b, hw) for s, b, hw in SHAPES])
def test_lines_equal_the_restatement(gpu_ctx, shape, b, halfwidth):
    from lfd_amd import _native
    frames = TG.batch(shape, seed=shape[0] + b)
    keep = frames.copy()
    min_len = max(1, min(shape) // (2 * b))
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02], np.float32)
    kw = {"max_lines": 3, "peel_halfwidth": halfwidth, "min_seg": max(1, min_len // 2)}
    # a threshold the streak and the integer frame pass for a round or more, the noise mostly not
    with _native.Radon(gpu_ctx, shape, max_frames=4, bin=b, min_len=min_len, threshold=4.0) as r:
        dev, dev_n = r.search_lines(frames, sigma=sigma, **kw)
        assert dev.shape == (4, 3) and dev.dtype == _native.RADON_LINE_DTYPE and dev_n.dtype == np.int32
        assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))          # only read
        counts = check_lines(frames, dev, dev_n, sigma, bin=b, min_len=min_len, threshold=4.0, **kw)
        assert max(counts) >= 1                                                      # (a frame was peeled and searched again)
        assert np.array_equal(r.search(frames, sigma=sigma), dev[:, 0][list(_native.RADON_DTYPE.names)])


def streak(f, x0, y0, dx, dy, amp=0.06):
    """adds a streak through (x0, y0) of the flipped frame along (dx, dy)"""
    h, w = f.shape
    t = np.linspace(-2 * (h + w), 2 * (h + w), 16 * (h + w))
    x, y = np.rint(x0 + t * dx).astype(int), np.rint(y0 + t * dy).astype(int)
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    pts = np.unique(np.stack([h - 1 - y[ok], x[ok]]), axis=1)
    f[pts[0], pts[1]] += np.float32(amp)
    return f


FIVE_SHAPE = (64, 64)
FIVE_PARAMS = {"bin": 1, "min_len": 52}              # below one crossing of 64 cells less two peeled bands (Wb = 64: 16-byte peel)
FIVE_SIGMA = np.array([0.025, 0.025, 0.03, 1.0 / 64, 0.02], np.float32)


def five_frames():
    """frames that leave at different rounds: dirty noise; one streak; three streaks that peak in orientations 0, 2 and 1
    (shallow, steep, descending); small integers (ties); one bright row on an otherwise invalid frame, whose peel leaves no
    candidate"""
    rng = np.random.default_rng(5)
    clean = rng.normal(0, 0.025, (2, *FIVE_SHAPE)).astype(np.float32)
    clean[0, 7, 9], clean[1, 30, 31], clean[1, 2, 50] = np.nan, np.inf, 0.0
    one = streak(clean[0], 32, 30, 1.0, 0.25)
    three = streak(streak(streak(clean[1], 32, 20, 1.0, 0.3, 0.05), 22, 32, 0.3, 1.0, 0.07), 32, 40, 1.0, -0.4, 0.06)
    lone = np.zeros(FIVE_SHAPE, np.float32)
    lone[20, :] = 0.05
    return np.stack([TG.dirty_noise(FIVE_SHAPE, 41), one, three, TG.tie_frame(FIVE_SHAPE), lone])


def test_frames_leave_at_different_rounds_through_three_chunks(gpu_ctx):
    from lfd_amd import _native
    frames = five_frames()
    keep = frames.copy()
    lp = {"max_lines": 4, "peel_halfwidth": 1, "min_seg": 16}
    with _native.Radon(gpu_ctx, FIVE_SHAPE, max_frames=2, threshold=8.0, **FIVE_PARAMS) as r:    # n = 5 through two slots
        plain = r.search(frames, sigma=FIVE_SIGMA)
        bytes0 = r.dims()[2]
        dev, dev_n = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))
        counts = check_lines(frames, dev, dev_n, FIVE_SIGMA, threshold=8.0, **FIVE_PARAMS, **lp)
        assert counts == [0, 1, 3, 4, 1]
        assert sorted(int(q) for q in dev["q"][2, :3]) == [0, 1, 2]                   # three orientations in one frame
        assert dev["status"][4].tolist() == [R.OK, R.NO_LINE, 0, 0] and dev["snr"][4, 1] == 0
        assert dev[4, 2] == np.zeros((), _native.RADON_LINE_DTYPE)
        # the second V, M set and the prefix arrays are counted once they exist
        px = FIVE_SHAPE[0] * FIVE_SHAPE[1]
        assert r.dims()[2] - bytes0 >= 2 * px * 6 + 2 * 65 * 8
        # record 0 is the plain search, before and after: the alternate buffers do not leak into it
        names = list(_native.RADON_DTYPE.names)
        assert np.array_equal(plain, dev[:, 0][names]) and np.array_equal(r.search(frames, sigma=FIVE_SIGMA), plain)
        again, again_n = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        assert np.array_equal(again, dev) and np.array_equal(again_n, dev_n)
    with _native.Radon(gpu_ctx, FIVE_SHAPE, max_frames=2, threshold=1e30, **FIVE_PARAMS) as r:   # nothing passes
        dev, dev_n = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        assert check_lines(frames, dev, dev_n, FIVE_SIGMA, threshold=1e30, **FIVE_PARAMS, **lp) == [0] * 5
        assert not dev[:, 1:]["status"].any() and not dev["c2"].any()


def test_every_frame_peels_to_the_end_and_ties_decide(gpu_ctx):
    from lfd_amd import _native
    frames = five_frames()
    lp = {"max_lines": 3, "peel_halfwidth": 1, "min_seg": 16}
    with _native.Radon(gpu_ctx, FIVE_SHAPE, max_frames=2, threshold=-1e30, **FIVE_PARAMS) as r:
        dev, dev_n = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        counts = check_lines(frames, dev, dev_n, FIVE_SIGMA, threshold=-1e30, **FIVE_PARAMS, **lp)
        assert counts[:4] == [3, 3, 3, 3] and counts[4] == 1                          # (the lone row has nothing left to find)
    const = np.full((1, 40, 40), 1.0 / 32, np.float32)           # every full crossing scores alike, and so do its intervals
    lp = {"max_lines": 3, "peel_halfwidth": 0, "min_seg": 40}
    with _native.Radon(gpu_ctx, (40, 40), max_frames=1, bin=1, min_len=40, threshold=-1e30) as r:
        dev, dev_n = r.search_lines(const, **lp)
        assert check_lines(const, dev, dev_n, bin=1, min_len=40, threshold=-1e30, **lp) == [3]
        assert [(int(x["q"]), int(x["s"]), int(x["c1"]), int(x["c2"])) for x in dev[0]] == [(0, 0, 0, 39)] * 3
        assert dev["y0"][0].tolist() == [0, 1, 2]


def test_dtypes_and_locations_agree_and_the_input_is_untouched():
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    frames = five_frames()
    lp = {"max_lines": 3, "peel_halfwidth": 1, "min_seg": 16}
    with _native.Context(0, 64, 64, 2) as ctx:
        r = _native.Radon(ctx, FIVE_SHAPE, max_frames=2, threshold=8.0, **FIVE_PARAMS)
        host, host_n = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        be = frames.astype(">f4")
        keep_be = be.copy()
        for got in (r.search_lines(be, sigma=FIVE_SIGMA, **lp),):
            assert np.array_equal(got[0], host) and np.array_equal(got[1], host_n)
        assert np.array_equal(be.view(np.uint32), keep_be.view(np.uint32))
        dev_frames = torch.from_numpy(frames).cuda()
        got = r.search_lines(dev_frames, sigma=FIVE_SIGMA, **lp)
        assert np.array_equal(got[0], host) and np.array_equal(got[1], host_n)
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))
        dev_be = torch.from_numpy(be.view(np.uint8).reshape(5, -1).copy()).cuda()
        got = r.search_lines(_native.DeviceFrames(dev_be.data_ptr(), (5, *FIVE_SHAPE)), sigma=FIVE_SIGMA, **lp)
        assert np.array_equal(got[0], host) and np.array_equal(got[1], host_n)
        assert np.array_equal(dev_be.cpu().numpy().reshape(-1), be.view(np.uint8).reshape(-1))
        pin = ctx.pinned_buffer(frames.nbytes)
        for order in ("<f4", ">f4"):
            pv = pin.array.view(order).reshape(frames.shape)
            pv[:] = frames
            got = r.search_lines(pv, sigma=FIVE_SIGMA, pinned=True, **lp)
            assert np.array_equal(got[0], host) and np.array_equal(got[1], host_n)
            assert np.array_equal(pv.view(np.uint32), frames.astype(order).view(np.uint32))
        pin.close()
        # the library refuses what RadonLinesParams.validate refuses (the handle's min_len is 52), and nothing runs
        from lfd_amd import radon
        for bad in TA.REFUSED[:4] + ({"min_seg": 53},):
            with pytest.raises(_native.NativeError) as e:
                r.search_lines(frames, **dict({"min_seg": 16}, **bad))
            assert e.value.code == _native.ERR_ARG
            with pytest.raises(ValueError):
                radon.RadonLinesParams(**dict({"min_seg": 16}, **bad)).validate(min_len=52)
        with pytest.raises(_native.NativeError):                     # (the default min_seg of 64 is above this handle's min_len)
            r.search_lines(frames)
        for good in ({"max_lines": 8, "min_seg": 16}, {"min_seg": 52}, {"peel_halfwidth": 0, "min_seg": 1}):
            r.search_lines(frames[:1], **good)
            radon.RadonLinesParams(**good).validate(min_len=52)
        with pytest.raises(_native.NativeError):
            r.search_lines(frames, sigma=np.array([0.02, 0.0, 0.02, 0.02, 0.02], np.float32))
        with pytest.raises(_native.NativeError):
            r.search_lines(np.zeros((1, 65, 64), np.float32))
        # refused while a detection call is pending; the context stays usable
        pb, pd, _ = default_params()
        pend = ctx.detect_batch_begin(torch.zeros((2, 64, 64), dtype=torch.float32, device="cuda"), pb, pd)
        with pytest.raises(_native.NativeError) as e:
            r.search_lines(frames, **lp)
        assert e.value.code == _native.ERR_ARG
        pend.result()
        got = r.search_lines(frames, sigma=FIVE_SIGMA, **lp)
        assert np.array_equal(got[0], host) and np.array_equal(got[1], host_n)
        one, one_n = radon.search_lines(ctx, frames[1], sigma=0.025, threshold=8.0, **FIVE_PARAMS, **lp)
        assert np.array_equal(one[0], host[1]) and one_n.tolist() == [host_n[1]]
    with pytest.raises(ValueError):                                  # the context closed its handle
        r.search_lines(frames, **lp)


def test_two_trail_model_frames_bit_for_bit(gpu_ctx):
    """the CPU test's two-trail frames at bin 2, the trails rendered by Context.inject_trails"""
    import torch
    from lfd_amd import _native
    _, table, step = TM.trail_plan()
    tr = np.concatenate([TL.two_trail_plan(k) for k in range(4)])
    tr["frame"] = np.repeat(np.arange(4), 2)
    frames = torch.from_numpy(np.concatenate([TL.two_trail_noise(k) for k in range(4)])).cuda()
    gpu_ctx.inject_trails(frames, tr, table, step)
    want = np.stack([TL.two_trail_frame(k) for k in range(4)])
    assert np.array_equal(frames.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=4, bin=2) as r:
        dev, dev_n = r.search_lines(frames, sigma=TM.SET_SIGMA)
    assert dev.shape == (4, 4) and dev_n.tolist() == [2, 2, 2, 2]
    bad = []
    for k in range(4):
        recs, n_lines = TL.two_trail_lines(k, 2)
        assert n_lines == 2
        bad += [(k, j, m) for j, m in ((j, same_line(dev[k, j], recs[j])) for j in range(4)) if m]
    assert not bad, bad[:5]


# ---- drop-in: DetectTrails(radon=True, radon_lines=K), radon.txt and radon_segments.txt ------------------------------------------
@pytest.mark.parametrize("batch", [1, 4])
def test_dropin_lines_and_segments(tmp_path, batch):
    """test_gpu_radon's three-frame tree with a second faint trail in field 101"""
    import inject_ref as IR
    from lfd_amd import inject as I, radon, synth
    from lfd_amd.detecttrails import DetectTrails
    shape = (512, 768)
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (3, *shape)).astype(np.float32)
    tr = np.zeros(3, IR.TRAIL_DTYPE)
    th, th2 = math.radians(115.0), math.radians(30.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    tr[0] = (1, 0, rho, th, -np.inf, np.inf, 0.02)
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    tr[2] = (1, 0, 400 * math.cos(th2) + 240 * math.sin(th2), th2, -np.inf, np.inf, 0.018)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, shape)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r", bz2_fields=(101,) if batch > 1 else ())
    outs = {}
    for name, kw in (("plain", {}), ("one", {"radon": True}), ("lines", {"radon": True, "radon_lines": 3})):
        d = tmp_path / name
        d.mkdir()
        dt = outs[name] = DetectTrails(run=94, camcol=1, filter="r", savepath=str(d), **kw)
        dt.process(batch=batch)
    plain, one, many = outs["plain"], outs["one"], outs["lines"]
    for dt in (one, many):
        assert TG.lines(dt.results) == TG.lines(plain.results) and open(dt.errors).read() == open(plain.errors).read()
    # radon_lines=None: today's radon.txt (the best line of field 101) and no segments file
    rows1 = radon.read_radon(one.radon_file)
    assert [r["field"] for r in rows1] == [101] and not os.path.exists(one.radon_segments_file)
    assert not os.path.exists(plain.radon_file) and not os.path.exists(plain.radon_segments_file)
    rows = radon.read_radon(many.radon_file)
    segs = radon.read_segments(many.radon_segments_file)
    assert [r["field"] for r in rows] == [101, 101] and [(s["field"], s["line"]) for s in segs] == [(101, 0), (101, 1)]
    assert TG.lines(many.radon_file)[0] == TG.lines(one.radon_file)[0]                 # peel order: the best line first
    matched = set()
    for r, s in zip(rows, segs):
        theta = math.atan2(-(r["x2"] - r["x1"]), r["y2"] - r["y1"]) % math.pi
        line = {"theta": theta, "rho": r["x1"] * math.cos(theta) + r["y1"] * math.sin(theta)}
        hit = [i for i in (0, 2) if TM.line_error(line, tr[i], shape)[0] <= 0.5 and TM.line_error(line, tr[i], shape)[1] <= 4.0]
        assert len(hit) == 1 and r["snr"] >= 8.0 and r["n_pix"] >= 256 and s["seg_n_pix"] >= 64
        matched.add(hit[0])
        for x, y in ((s["ex1"], s["ey1"]), (s["ex2"], s["ey2"])):                      # the segment's ends lie along the line
            assert abs(x * math.cos(theta) + y * math.sin(theta) - line["rho"]) <= 4.0
    assert matched == {0, 2}
