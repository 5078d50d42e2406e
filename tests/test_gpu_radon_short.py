"""lfdmi_radon_search_short on the device against the numpy restatement of steps 10 - 12 (tests/radon_short_ref.py): every
integer field, the float32 bits of sum, snr, seg_sum and seg_snr and n_lines exactly, the doubles to 1e-12, and the plain
record against radon_ref -- at the smallest shapes where the scoring levels re-tile, on constructed ties, at the edge of the
candidate rule, through chunks, dtypes and locations, and with the lines call on the same handle before and after."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_short_ref as S  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_gpu_radon_lines as TGL  # noqa: E402
import test_radon_short_abi as TA  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = TGL.INT_FIELDS + ("level", "strip", "ys", "ss")
TIE_SIGMA = 1.0 / 64


def same_short(dev, ref):
    for k in INT_FIELDS:
        if int(dev[k]) != int(ref[k]):
            return f"{k}: device {int(dev[k])} != restatement {int(ref[k])}"
    for k in TGL.F32_FIELDS:
        if TG.f32_bits(dev[k]) != TG.f32_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in TGL.F64_FIELDS:
        a, b = float(dev[k]), float(ref[k])
        if abs(a - b) > 1e-12 * abs(b):
            return f"{k}: device {a!r} != restatement {b!r}"
    return None if int(dev["pad"]) == 0 else "pad is not zero"


def check_short(frames, out, sigma=None, **params):
    """every record of every frame, n_lines and the plain record against the restatement; returns its (records, n_lines) lists"""
    dev, dev_n, plain = out
    short = {k: v for k, v in params.items() if k in S.SHORT_DEFAULTS}
    bad, all_recs, counts = [], [], []
    for i, f in enumerate(frames):
        sg = R.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[i % np.size(sigma)]
        recs, n_lines, ref_plain = S.search_short(f, sg, **params)
        all_recs.append(recs)
        counts.append(n_lines)
        if int(dev_n[i]) != n_lines:
            bad.append((i, f"n_lines: device {int(dev_n[i])} != restatement {n_lines}"))
        for k, ref in enumerate(recs):
            msg = same_short(dev[i, k], ref)
            if msg:
                bad.append((i, k, msg))
        msg = TG.same_record(plain[i], ref_plain)
        if msg:
            bad.append((i, "plain", msg))
    assert dev.shape == (len(frames), short.get("max_lines", 4)), dev.shape
    assert not bad, bad[:5]
    return all_recs, counts


def short_batch(shape, seed, b=1):
    """test_gpu_radon's batch (dirty noise twice, the tie frame, a full streak) and a frame with two short streaks"""
    f = TG.batch(shape, seed)
    h, w = shape
    two = TG.dirty_noise(shape, seed + 3)
    for x in range(w // 8, w // 8 + 40 * b):
        two[min(h - 1, h // 3 + (x - w // 8) // 3), min(w - 1, x)] += 0.1
    for x in range(w // 2, min(w, w // 2 + 48 * b)):
        two[max(0, h - 1 - h // 4 - (x - w // 2) // 5), x] += 0.08
    return np.concatenate([f, two[None]])


# (shape, bin, min_strip, max_lines, what the case is there for)
CASES = [
    ((48, 64), 1, 64, 3, "P = 64 in both pairs: no scored level"),
    ((40, 100), 1, 64, 3, "Wb = 100: P = 128, one scored level whose second strip straddles C"),
    ((70, 256), 1, 64, 3, "R = 70 below RAD_Y; P = 256 / 128: orientations 0, 1 have a level that 2, 3 lack"),
    ((70, 256), 1, 128, 1, "min_strip = 128 on the same frames; one round"),
    ((150, 128), 1, 64, 3, "Hb = 150: two row bands of a scoring level, the second partial"),
    ((75, 259), 2, 64, 3, "bin 2 with ragged last cells"),
    ((150, 517), 4, 64, 1, "bin 4 with ragged last cells"),
]


@pytest.mark.parametrize("shape,b,min_strip,max_lines,why", CASES, ids=["%dx%d-bin%d-strip%d-k%d" % (*c[0], *c[1:4]) for c in CASES])
def test_short_records_equal_the_restatement(gpu_ctx, shape, b, min_strip, max_lines, why):
    from lfd_amd import _native
    frames = short_batch(shape, seed=shape[0] + b, b=b)
    keep = frames.copy()
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02, 0.025], np.float32)
    kw = {"min_strip": min_strip, "max_lines": max_lines, "peel_halfwidth": 2, "min_seg": 16, "short_threshold": 4.5}
    min_len = max(1, min(shape) // (2 * b))
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=b, min_len=min_len) as r:      # five frames through three slots
        want_plain = r.search(frames, sigma=sigma)
        bytes0 = r.dims()[2]
        out = r.search_short(frames, sigma=sigma, plain=True, **kw)
        assert out[0].dtype == _native.RADON_SHORT_DTYPE and out[1].dtype == np.int32
        assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))          # only read
        assert np.array_equal(out[2], want_plain)                                    # bit for bit Radon.search
        assert r.dims()[2] > bytes0                                                  # the rounds' buffers are counted
        recs, counts = check_short(frames, out, sigma, bin=b, min_len=min_len, **kw)
        hb, wb = -(-shape[0] // b), -(-shape[1] // b)
        if max(R.pow2_at_least(hb), R.pow2_at_least(wb)) // 2 < min_strip:
            assert all(rr[0]["status"] == R.NO_LINE for rr in recs) and counts == [0] * 5
            assert (out[2]["status"] == R.OK).all()                                  # while plain is still filled
        else:
            assert max(counts) >= 1, why
            if max_lines > 1:
                assert max(counts) >= 2, why                                         # (a frame was peeled and searched again)
        without = r.search_short(frames, sigma=sigma, **kw)                          # plain = NULL
        assert len(without) == 2 and np.array_equal(without[0], out[0]) and np.array_equal(without[1], out[1])


def tie_frames():
    """exact ties, everything else invalid (+0): a run of 64 pixels of 1/8 in columns 0 .. 63 of one row scores alike as the
    level-64 strip 0 and as the level-128 strip 0 (N = 64 both: the other half of the wider strip is invalid); the second
    frame has the same run again in columns 128 .. 191 of another row, strips 0 and 2 of level 64"""
    a = np.zeros((24, 512), np.float32)
    a[24 - 1 - 10, 0:64] = 0.125
    b = a.copy()
    b[24 - 1 - 17, 128:192] = 0.125
    return np.stack([a, b])


def test_ties_between_levels_and_between_strips(gpu_ctx):
    from lfd_amd import _native
    frames = tie_frames()
    kw = {"max_lines": 2, "peel_halfwidth": 0, "min_seg": 8, "short_threshold": 1.0}
    with _native.Radon(gpu_ctx, frames.shape[1:], max_frames=2, bin=1, min_len=8) as r:
        out = r.search_short(frames, sigma=TIE_SIGMA, plain=True, **kw)
    recs, counts = check_short(frames, out, TIE_SIGMA, bin=1, min_len=8, **kw)
    assert counts == [1, 2]
    for rr in recs:                                         # lowest L, then q, then strip
        assert (rr[0]["level"], rr[0]["q"], rr[0]["strip"], rr[0]["ss"], rr[0]["ys"]) == (64, 0, 0, 0, 10)
        assert rr[0]["n_pix"] == 64 and float(rr[0]["snr"]) == 64.0
    assert (recs[1][1]["level"], recs[1][1]["strip"], recs[1][1]["ys"]) == (64, 2, 17) and float(recs[1][1]["snr"]) == 64.0
    # the restatement does see equal scores there: the wider level's strip 0 holds the same 64 pixels
    V, M = R.prepare(frames[0], 1, 0.125)
    N128 = [F for n, F in S.levels(M) if n == 128][0]
    S128 = [F for n, F in S.levels(V) if n == 128][0]
    assert N128[0, 10 + 511, 0] == 64 and S128[0, 10 + 511, 0] == 8.0


def test_rightmost_strip_at_the_steepest_slope(gpu_ctx):
    """the lowest parent row there is: y0 = y - s (P / L - 1) with y near -(L-1), s = L-1 in the last strip"""
    from lfd_amd import _native
    shape, Lv, P = (80, 256), 64, 256
    f = TG.dirty_noise(shape, 9)
    V = np.zeros(shape, np.float32)
    d = L.dyadic_path(Lv - 1, Lv)
    y = -(Lv // 2) + 3
    for c in range(Lv):
        if 0 <= y + d[c] < shape[0]:
            V[y + d[c], P - Lv + c] = 0.1
    f += V[::-1]
    frames = f[None]
    kw = {"max_lines": 2, "peel_halfwidth": 2, "min_seg": 16}
    with _native.Radon(gpu_ctx, shape, max_frames=1, bin=1, min_len=32) as r:
        out = r.search_short(frames, plain=True, **kw)
    recs, counts = check_short(frames, out, bin=1, min_len=32, **kw)
    top = recs[0][0]
    assert counts[0] >= 1 and (top["level"], top["strip"], top["ss"], top["ys"]) == (Lv, P // Lv - 1, Lv - 1, y)
    assert top["y0"] == y - (Lv - 1) * (P // Lv - 1) and top["y0"] < -(P // 2)
    # before the strip the parent's rows do not exist (+0, no pixels): equal scores, so the segment starts at the lowest c1
    assert top["c1"] == 0 and top["c2"] >= P - Lv and top["seg_n_pix"] <= Lv


def test_the_candidate_rule_one_pixel_either_side(gpu_ctx):
    """2 N >= L b b at L = 64, bin 1: a lone run of 31, 32 and 33 valid pixels in an otherwise invalid frame"""
    from lfd_amd import _native
    frames = np.zeros((3, 24, 128), np.float32)
    for i, npx in enumerate((31, 32, 33)):
        frames[i, 12, 5:5 + npx] = 0.0625
    kw = {"max_lines": 1, "min_seg": 8, "short_threshold": 1.0}
    with _native.Radon(gpu_ctx, (24, 128), max_frames=3, bin=1, min_len=8) as r:
        out = r.search_short(frames, plain=True, **kw)
    recs, counts = check_short(frames, out, bin=1, min_len=8, **kw)
    assert counts == [0, 1, 1]
    assert recs[0][0]["status"] == R.NO_LINE and [rr[0]["n_pix"] for rr in recs[1:]] == [32, 33]
    assert out[2]["n_pix"].tolist() == [31, 32, 33]                                  # the plain search counts them all


def test_dtypes_locations_refusals_and_the_lines_call_after(gpu_ctx):
    import torch
    from lfd_amd import _native, radon
    shape = (70, 256)
    frames = short_batch(shape, seed=71)
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02, 0.025], np.float32)
    kw = {"max_lines": 3, "peel_halfwidth": 2, "min_seg": 16, "short_threshold": 4.5}
    lp = {"max_lines": 3, "peel_halfwidth": 2, "min_seg": 16}
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=1, min_len=32) as r:
        lines0 = r.search_lines(frames, sigma=sigma, **lp)
        host = r.search_short(frames, sigma=sigma, plain=True, **kw)
        check_short(frames, host, sigma, bin=1, min_len=32, **kw)

        def same(got):
            return all(np.array_equal(a, b) for a, b in zip(got, host))
        be = frames.astype(">f4")
        assert same(r.search_short(be, sigma=sigma, plain=True, **kw))                  # LFDMI_F32_BE
        dev_frames = torch.from_numpy(frames).cuda()
        assert same(r.search_short(dev_frames, sigma=sigma, plain=True, **kw))          # device frames
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))
        dev_be = torch.from_numpy(be.view(np.uint8).reshape(5, -1).copy()).cuda()
        assert same(r.search_short(_native.DeviceFrames(dev_be.data_ptr(), (5, *shape)), sigma=sigma, plain=True, **kw))
        # the lines call and the plain call are what they were before the short calls
        lines1 = r.search_lines(frames, sigma=sigma, **lp)
        assert np.array_equal(lines0[0], lines1[0]) and np.array_equal(lines0[1], lines1[1])
        assert np.array_equal(r.search(frames, sigma=sigma), host[2])
        # the library refuses what RadonShortParams.validate refuses, and nothing runs
        for bad in TA.REFUSED:
            with pytest.raises(_native.NativeError) as e:
                r.search_short(frames, **bad)
            assert e.value.code == _native.ERR_ARG, bad
        for good in TA.TAKEN:
            r.search_short(frames[:1], **good)
        with pytest.raises(_native.NativeError):
            r.search_short(frames, sigma=np.array([0.02, 0.0, 0.02, 0.02, 0.02], np.float32))
        assert same(r.search_short(frames, sigma=sigma, plain=True, **kw))
    one = radon.search_short(gpu_ctx, frames[4], sigma=0.025, bin=1, min_len=32, **kw)
    assert np.array_equal(one[0][0], host[0][4]) and one[1].tolist() == [host[1][4]]
    # the segment helpers take the new records unchanged
    from lfd_amd import stack
    rec = host[0][4, 0]
    assert rec["found"] == 1
    pts = radon.segment_points(int(rec["q"]), int(rec["y0"]), int(rec["s"]), int(rec["c1"]), int(rec["c2"]), shape, 1)
    assert pts == (rec["ex1"], rec["ey1"], rec["ex2"], rec["ey2"])
    segs, where = stack.segments_from_radon_lines(host[0], host[1])
    assert len(segs) == len(where) == int(host[1].sum())
    k = where.index((4, 0))
    assert (segs["x1"][k], segs["y1"][k], segs["x2"][k], segs["y2"][k]) == pts


# ---- drop-in: DetectTrails(radon=True, radon_short=...), radon_short.txt -----------------------------------------------------------
def test_dropin_writes_radon_short_and_leaves_the_other_files(tmp_path):
    """test_gpu_radon_lines' three-frame tree with a short faint trail in field 101 instead of its full-length ones"""
    import inject_ref as IR
    from lfd_amd import inject as I, radon, stack, synth
    from lfd_amd.detecttrails import DetectTrails
    shape = (512, 768)
    rng = np.random.default_rng(12)
    frames = rng.normal(0, 0.025, (3, *shape)).astype(np.float32)
    tr = np.zeros(2, IR.TRAIL_DTYPE)
    th = math.radians(115.0)
    c, s = math.cos(th), math.sin(th)
    rho, tm = 384 * c + 256 * s, -384 * s + 256 * c
    tr[0] = (1, 0, rho, th, tm - 100, tm + 100, 0.04)                     # 200 px of a 768 px crossing
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)           # the detector's
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, shape)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r")
    outs = {}
    for name, kw in (("one", {"radon": True}), ("short", {"radon": True, "radon_short": True}),
                     ("both", {"radon": True, "radon_lines": 2, "radon_short": {"max_lines": 2, "min_strip": 128},
                               "radon_profiles": True})):
        d = tmp_path / name
        d.mkdir()
        dt = outs[name] = DetectTrails(run=94, camcol=1, filter="r", savepath=str(d), **kw)
        dt.process(batch=4)
    one, short, both = outs["one"], outs["short"], outs["both"]
    # the default leaves no radon_short.txt; with it every other file is byte for byte what it was
    assert not os.path.exists(one.radon_short_file)
    for name in ("results", "errors", "radon_file"):
        assert open(getattr(short, name)).read() == open(getattr(one, name)).read(), name
    assert not os.path.exists(short.radon_segments_file)
    rows = radon.read_short(short.radon_short_file)
    assert [(r["field"], r["line"]) for r in rows] == [(101, 0)]
    r = rows[0]
    assert r["snr"] >= 8.5 and r["level"] in (64, 128, 256) and r["n_pix"] >= r["level"] * 2 and r["seg_n_pix"] >= 32
    lo, hi = sorted((-r["ex1"] * s + r["ey1"] * c, -r["ex2"] * s + r["ey2"] * c))
    assert abs(lo - (tm - 100)) <= 34 and abs(hi - (tm + 100)) <= 34, (lo, hi, tm)
    for x, y in ((r["ex1"], r["ey1"]), (r["ex2"], r["ey2"])):                         # the segment lies along the trail
        assert abs(x * c + y * s - rho) <= 6.0
    assert len(open(short.radon_short_file).read().split()) == len(radon.SHORT_COLUMNS)
    # with the lines and the profiles: rows tagged by their source, the short ones measured on the short segment
    rows2 = radon.read_short(both.radon_short_file)
    assert [(q["field"], q["line"]) for q in rows2][:1] == [(101, 0)] and all(q["level"] >= 128 for q in rows2)
    tags = [ln.split()[-1] for ln in open(both.radon_profiles_file).read().splitlines() if ln.strip()]
    assert set(tags) <= {"lines", "short"} and tags.count("short") == len(rows2)
    assert tags.count("lines") == len(radon.read_segments(both.radon_segments_file))
    prof = stack.read_profiles(both.radon_profiles_file)
    assert len(prof) == len(tags) and all(p["field"] == 101 for p in prof)


def test_recovery_matches_short_trails_by_their_parent_line(gpu_ctx):
    """quarter-length trails of peak 0.06 on 512 x 512 noise: the short search recovers them, matched by make_rows' rule"""
    from lfd_amd import inject as I, recovery as RC
    shape, n = (512, 512), 8
    frames = np.random.default_rng(31).normal(0, 0.025, (n, *shape)).astype(np.float32)
    plan = RC.shorten(RC.draw_trails(n, shape, 3, [0.06]), shape, 0.25, 3)
    table, step = I.gaussian_table(2.0)
    kw = {"radon_params": {"bin": 2}, "sigma": 0.025}
    with __import__("lfd_amd")._native.Context(0, *shape, n) as ctx:
        rows = RC.run(ctx, frames, None, None, plan, I.normalise_peak(table), step, detector="radon-short", **kw)
        full = RC.run(ctx, frames, None, None, RC.draw_trails(n, shape, 3, [0.06]), I.normalise_peak(table), step,
                      detector="radon-short", short_params={"max_lines": 1}, **kw)
    assert rows.dtype == RC.ROW_DTYPE and len(rows) == n
    assert rows["found"].all() and np.allclose(rows["length"], plan["t1"] - plan["t0"])
    assert rows["matched"].sum() >= n - 2, rows[["matched", "d_rho", "d_theta"]]
    assert full["found"].all() and full["matched"].sum() >= n - 1               # a full crossing is found at level P/2
