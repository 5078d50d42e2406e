"""lfdmi_radon_search_wide on the device against the numpy restatement of steps 13 - 16 (tests/radon_wide_ref.py): every
integer field and n_lines, the float32 bits of sum, snr, seg_sum and seg_snr and every bit of the doubles, and the plain record
against Radon.search -- at the smallest shapes that cross k_radon_wide's row blocks (RADW_Y = 64), its halo above R-1, its
slope chunks (RADW_S = 64) and the small-frame route, on constructed ties, through the band's peel and extent, through chunks,
and at every refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_wide_ref as W  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_gpu_radon_lines as TGL  # noqa: E402
import test_radon_wide_abi as TA  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = TGL.INT_FIELDS + ("width", "pad", "pad2")
F64_FIELDS = TGL.F64_FIELDS + ("width_px",)
TIE_SIGMA = 1.0 / 64


def f64_bits(v):
    return int(np.asarray(v, np.float64).view(np.uint64))


def same_wide(dev, ref):
    for k in INT_FIELDS:
        if int(dev[k]) != int(ref.get(k, 0)):
            return f"{k}: device {int(dev[k])} != restatement {int(ref.get(k, 0))}"
    for k in TGL.F32_FIELDS:
        if TG.f32_bits(dev[k]) != TG.f32_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in F64_FIELDS:
        if f64_bits(dev[k]) != f64_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    return None


def same_plain(dev, ref):
    for k in TG.INT_FIELDS:
        if int(dev[k]) != int(ref[k]):
            return f"{k}: device {int(dev[k])} != restatement {int(ref[k])}"
    for k in TG.F32_FIELDS:
        if TG.f32_bits(dev[k]) != TG.f32_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in TG.F64_FIELDS:
        if f64_bits(dev[k]) != f64_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    return None


def check_wide(frames, out, sigma=None, **params):
    """every record of every frame, n_lines and the plain record against the restatement; returns its (records, n_lines) lists"""
    dev, dev_n, plain = out
    bad, all_recs, counts = [], [], []
    for i, f in enumerate(frames):
        sg = R.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[i % np.size(sigma)]
        recs, n_lines, ref_plain = W.search_wide(f, sg, **params)
        all_recs.append(recs)
        counts.append(n_lines)
        if int(dev_n[i]) != n_lines:
            bad.append((i, f"n_lines: device {int(dev_n[i])} != restatement {n_lines}"))
        for k, ref in enumerate(recs):
            msg = same_wide(dev[i, k], ref)
            if msg:
                bad.append((i, k, msg))
        msg = same_plain(plain[i], ref_plain)
        if msg:
            bad.append((i, "plain", msg))
    assert dev.shape == (len(frames), params.get("max_lines", 4)), dev.shape
    assert not bad, bad[:5]
    return all_recs, counts


def paint_band(f, q, y0, s, k, amp):
    """adds amp to the cells of lines y0 .. y0+k-1 of slope s of orientation q (bin 1) that lie in the frame"""
    Q = R.orient(f[::-1], q)                               # a view: row 0 of V is the buffer's last row
    Rr, C = Q.shape
    d = L.dyadic_path(s, R.pow2_at_least(C))[:C]
    cols = np.arange(C)
    for u in range(k):
        rows = y0 + u + d
        ok = (rows >= 0) & (rows < Rr)
        Q[rows[ok], cols[ok]] += np.float32(amp)


# 200 x 96 at bin 1: orientations 0, 1 have R = 200, P = 128 (row y is plane row y + 127: k_radon_wide's row blocks start at
# y = -127, -63, 1, 65, 129, 193; slope chunks at 0, 64), orientations 2, 3 have R = 96, P = 256 (blocks from y = -255 in steps
# of 64: .. -63, 1, 65; chunks at 0, 64, 128, 192).  (q, y0, s, k) of the band painted into each frame, and what it is there for
BANDS = [
    ((0, 57, 10, 16), "16 lines astride the row-block edge at y = 65"),
    ((1, 196, 3, 4), "the top rows: wider bands there read the halo's +0 past R - 1 and tie with this one"),
    ((0, -40, 100, 2), "wholly at negative y"),
    ((0, 20, 64, 1), "one line at the slope-chunk edge s = 64"),
    ((2, -67, 127, 8), "8 lines astride the block edge at y = -63 of the P = 256 pair, beside the chunk edge s = 128"),
    ((3, 60, 191, 4), "the last slope of a chunk in the flipped tall orientation, clipped by the frame's edge"),
]
BAND_SHAPE = (200, 96)


def band_frames():
    frames = []
    for i, ((q, y0, s, k), _) in enumerate(BANDS):
        f = TG.dirty_noise(BAND_SHAPE, 40 + i)
        paint_band(f, q, y0, s, k, 0.05)
        frames.append(f)
    return np.stack(frames)


def test_bands_at_the_block_chunk_and_frame_edges(gpu_ctx):
    from lfd_amd import _native
    frames = band_frames()
    keep = frames.copy()
    sigma = np.array([0.025, 0.03, 0.02, 0.025, 1.0 / 64, 0.025], np.float32)
    kw = {"max_width": 16, "max_lines": 2, "peel_halfwidth": 2, "min_seg": 16, "wide_threshold": 6.0}
    with _native.Radon(gpu_ctx, BAND_SHAPE, max_frames=4, bin=1, min_len=16) as r:      # six frames through four slots: chunks
        want_plain = r.search(frames, sigma=sigma)
        bytes0 = r.dims()[2]
        out = r.search_wide(frames, sigma=sigma, plain=True, **kw)
        assert out[0].dtype == _native.RADON_WIDE_DTYPE and out[1].dtype == np.int32
        assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))          # only read
        assert np.array_equal(out[2], want_plain)                                    # bit for bit Radon.search
        assert r.dims()[2] > bytes0                                                  # the call's buffers are counted
        recs, counts = check_wide(frames, out, sigma, bin=1, min_len=16, **kw)
        without = r.search_wide(frames, sigma=sigma, **kw)                           # plain = NULL
        assert len(without) == 2 and np.array_equal(without[0], out[0]) and np.array_equal(without[1], out[1])
        assert np.array_equal(r.search(frames, sigma=sigma), want_plain)             # and the plain call is what it was
    # the painted band is the frame's first record, at its own width
    for rr, ((q, y0, s, k), why) in zip(recs, BANDS):
        top = rr[0]
        assert top["found"] == 1 and (top["q"], top["width"]) == (q, k), why
        assert abs(top["y0"] - y0) <= 3 and abs(top["s"] - s) <= 4, why     # (noise may tilt the best band by a few slopes)
    assert sorted({rr[0]["width"] for rr in recs}) == [1, 2, 4, 8, 16]
    assert min(counts) >= 1


SMALL = [((24, 40), 1, 4), ((5, 3), 1, 1), ((37, 50), 2, 4)]


@pytest.mark.parametrize("shape,b,min_len", SMALL, ids=["%dx%d-bin%d" % (*s, b) for s, b, _ in SMALL])
def test_small_frames_take_the_scalar_last_level(gpu_ctx, shape, b, min_len):
    """24 x 40: P = 64 for orientations 0, 1 (the 16-byte last level, one slope chunk) and P = 32 for 2, 3 (P/2 < 32: the scalar
    one, a workgroup of 32 slopes); 5 x 3: P = 4 and 8; 37 x 50 at bin 2: P = 32 in both pairs"""
    from lfd_amd import _native
    frames = TG.batch(shape, seed=shape[0] + b)
    if shape[0] >= 24:
        paint_band(frames[1], 2, -3, 9, 4, 0.05)
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02], np.float32)
    kw = {"max_width": 16, "max_lines": 3, "peel_halfwidth": 1, "min_seg": min_len, "wide_threshold": 4.5}
    with _native.Radon(gpu_ctx, shape, max_frames=4, bin=b, min_len=min_len) as r:
        want_plain = r.search(frames, sigma=sigma)
        out = r.search_wide(frames, sigma=sigma, plain=True, **kw)
        assert np.array_equal(out[2], want_plain)
    recs, counts = check_wide(frames, out, sigma, bin=b, min_len=min_len, **kw)
    assert all(rr[0]["status"] == R.OK for rr in recs)


def test_tie_rule_across_partial_records(gpu_ctx):
    """a constant frame: every band of one width and pixel count scores alike, in every orientation, row block and slope
    chunk, so the record is the lowest (k, q, s, y) among equals in every round.  The threshold of -1e30 is the handle's (the
    plain record's ``found``): wide_threshold has to be positive and stays at 8, which every round's score of 91.2 passes, so
    all three rounds run"""
    from lfd_amd import _native
    shape = (70, 130)
    frames = np.full((1, *shape), 1.0 / 32, np.float32)
    kw = {"max_width": 16, "max_lines": 3, "peel_halfwidth": 0, "min_seg": 8}
    with _native.Radon(gpu_ctx, shape, max_frames=1, bin=1, min_len=40, threshold=-1e30) as r:
        out = r.search_wide(frames, sigma=TIE_SIGMA, plain=True, **kw)
        assert np.array_equal(out[2], r.search(frames, sigma=TIE_SIGMA))
    recs, counts = check_wide(frames, out, TIE_SIGMA, bin=1, min_len=40, threshold=-1e30, **kw)
    assert counts == [3]
    top = recs[0][0]
    assert (top["width"], top["q"], top["s"], top["n_pix"]) == (16, 0, 0, 16 * 130)
    # the restatement does see equal scores there
    V, M = R.prepare(frames[0], 1, 0.125)
    S, N = R.transform(R.orient(V, 0)), R.transform(R.orient(M, 0))
    k, B, Cn = list(W.bands(S, N, 16))[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = (B / (np.float32(TIE_SIGMA) * np.sqrt(Cn.astype(np.float32)))).astype(np.float32)
    assert k == 16 and (snr[Cn == 16 * 130] == top["snr"]).sum() > 64              # (more than one workgroup's worth)


def test_max_width_1_is_search_lines(gpu_ctx):
    from lfd_amd import _native
    shape = (97, 161)
    frames = TG.batch(shape, seed=11)
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02], np.float32)
    lp = {"max_lines": 3, "peel_halfwidth": 3, "min_seg": 16}
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=2, min_len=24, threshold=4.5) as r:
        lines, nl = r.search_lines(frames, sigma=sigma, **lp)
        wide, wn, plain = r.search_wide(frames, sigma=sigma, plain=True, max_width=1, wide_threshold=4.5, **lp)
        again, _ = r.search_lines(frames, sigma=sigma, **lp)
    assert np.array_equal(nl, wn) and nl.max() >= 2
    for k in _native.RADON_LINE_DTYPE.names:
        assert np.ascontiguousarray(wide[k]).tobytes() == np.ascontiguousarray(lines[k]).tobytes(), k
    assert np.array_equal(wide["width"], (lines["n_pix"] > 0).astype(np.int32))
    assert np.array_equal(again, lines)
    check_wide(frames, (wide, wn, plain), sigma, bin=2, min_len=24, threshold=4.5, max_width=1, wide_threshold=4.5, **lp)


def test_two_crossing_trails_of_different_widths(gpu_ctx):
    """the band's peel and extent: an 8-cell band and a crossing 2-cell band that leaves the frame through its top edge (its
    upper line is clipped before the other), three rounds"""
    from lfd_amd import _native
    shape = (120, 160)
    frames = np.stack([TG.dirty_noise(shape, 5), TG.dirty_noise(shape, 6)])
    paint_band(frames[0], 0, 40, 30, 8, 0.04)
    paint_band(frames[0], 2, 100, 100, 2, 0.07)            # R = 160, P = 128: rows 100 + d(c) pass 159 before the last column
    paint_band(frames[1], 1, 112, 20, 8, 0.05)             # R = 120: the band's upper lines leave through the top
    paint_band(frames[1], 3, -30, 90, 2, 0.07)
    kw = {"max_width": 8, "max_lines": 3, "peel_halfwidth": 3, "min_seg": 24, "wide_threshold": 6.0}
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=1, min_len=32) as r:
        out = r.search_wide(frames, plain=True, **kw)
    recs, counts = check_wide(frames, out, bin=1, min_len=32, **kw)
    assert counts == [2, 2]
    for rr in recs:
        assert sorted(x["width"] for x in rr[:2]) == [2, 8] and rr[2]["found"] == 0 and rr[2]["status"] == R.OK
        for x in rr[:2]:
            assert x["seg_n_pix"] >= 24 and x["c2"] > x["c1"]
    from lfd_amd import masks
    segs, where = masks.segments_from_radon_wide(out[0], out[1])
    assert where == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert segs["half"].tolist() == [float(out[0][i, k]["width_px"]) / 2 + 2 for i, k in where]


def test_bin_2_model_frames(gpu_ctx):
    """two of test_radon_wide_model's 372 x 512 frames (a sigma-6 trail the plain search misses) and a noise frame at the
    defaults, one slot: three chunks"""
    import test_radon_model as TM
    import test_radon_wide_model as TWM
    from lfd_amd import _native
    _, wf = TWM.wide_trail_frames()
    frames = np.stack([wf[0], wf[10], TM.noise_frames()[3]])
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=1) as r:
        out = r.search_wide(frames, sigma=TM.SET_SIGMA, plain=True)
    recs, counts = check_wide(frames, out, TM.SET_SIGMA)
    assert counts == [1, 1, 0] and out[2]["found"].tolist() == [0, 0, 0]
    assert [rr[0]["width"] for rr in recs[:2]] == [8, 8]


def test_refusals_leave_the_handle_usable(gpu_ctx):
    import torch
    from lfd_amd import _native, radon
    shape = (70, 130)
    frames = np.stack([TG.dirty_noise(shape, 21), TG.dirty_noise(shape, 22)])
    paint_band(frames[1], 0, 10, 20, 4, 0.05)
    kw = {"max_lines": 2, "peel_halfwidth": 2, "wide_threshold": 6.0}
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=1, min_len=64) as r:
        first = r.search_wide(frames, plain=True, **kw)
        check_wide(frames, first, bin=1, min_len=64, **kw)

        def same(got):
            return all(np.array_equal(a, b) for a, b in zip(got, first))
        for bad in TA.REFUSED:
            with pytest.raises(_native.NativeError) as e:
                r.search_wide(frames, **bad)
            assert e.value.code == _native.ERR_ARG, bad
            assert same(r.search_wide(frames, plain=True, **kw)), bad
        for good in TA.TAKEN:
            r.search_wide(frames[:1], **good)
        with pytest.raises(_native.NativeError) as e:
            r.search_wide(frames, sigma=np.array([0.02, 0.0], np.float32))
        assert e.value.code == _native.ERR_ARG
        with pytest.raises(_native.NativeError):
            r.search_wide(np.zeros((1, 71, 130), np.float32))
        assert same(r.search_wide(frames.astype(">f4"), plain=True, **kw))               # LFDMI_F32_BE
        dev_frames = torch.from_numpy(frames).cuda()
        assert same(r.search_wide(dev_frames, plain=True, **kw))                         # device frames, only read
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))
    one = radon.search_wide(gpu_ctx, frames[1], bin=1, min_len=64, **kw)
    assert np.array_equal(one[0][0], first[0][1]) and one[1].tolist() == [first[1][1]]
    assert first[1][1] >= 1 and first[0][1, 0]["width"] == 4
