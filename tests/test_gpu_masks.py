"""Trail masks on the device against the numpy restatement of include/lfdmi.h (tests/mask_ref.py), byte for byte: the mask
planes, the filled frames, the per-segment and per-frame counts, over the shapes at which the 64 x 16 tiling can go wrong, every
kind of segment, every fill mode and buffer location; the refusals; and the composition with the faint-trail search."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

# 1 x 1; one side of each tile edge (tiles are 64 wide, 16 high); w % 4 != 0 with partial tiles on both axes; a crop of four
# tile columns by 24 tile rows
SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (37, 130), (372, 512)]
N_FRAMES = 5          # frame 2 carries no segment, frame 3 three hundred (more than two LDS chunks of 128), frame 4 only bad ones


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hand_made(shape):
    """segments of frame 0: every direction, reach, half-width and cap the definition distinguishes"""
    h, w = shape
    inf = np.inf
    S = MR.segment
    return [
        S(0, 0.0, h // 2, w - 1.0, h // 2, half=2.0, bits=1, fill=1.0),                    # axis-aligned, centres exactly on the band edge
        S(0, w // 2, 0.0, w // 2, h - 1.0, half=1.0, cap=3.0, bits=2, fill=2.0),           # vertical, capped
        S(0, w // 3, h - 1.0, w // 3, 0.0, half=3.0, bits=2, fill=2.5),                    # vertical, downwards, integer half
        S(0, 0.0, 0.0, min(h, w) - 1.0, min(h, w) - 1.0, half=0.5, bits=4, fill=3.0),      # 45 degrees
        S(0, w - 1.0, 0.0, w - 1.0 - min(h, w), float(min(h, w)), half=0.0, bits=8, fill=4.0),   # 135 degrees, only centres on the line
        S(0, 1.0, h // 3, w - 2.0, h // 3, half=0.0, cap=0.0, bits=16, fill=5.0),          # half 0 along a row
        S(0, -10.0, h / 3.0, w + 10.0, h / 3.0 + 2.3, half=1.7, cap=inf, bits=32, fill=6.0),   # shallow, ends outside, the whole line
        S(0, w / 2.0 - 1.3, -5.0, w / 2.0 + 2.9, h + 4.0, half=2.25, cap=0.0, bits=64, fill=7.0),   # steep, ends outside
        S(0, w / 4.0, h / 4.0, w / 4.0 + 3.0, h / 4.0 + 1.0, half=1.0, cap=inf, bits=128, fill=8.0),   # a short one, the whole line
        S(0, w + 100.0, h + 100.0, w + 200.0, h + 150.0, half=3.0, bits=1),                # wholly outside: EMPTY
        S(0, -50.0, -20.0, -5.0, -3.0, half=2.0, cap=1.0, bits=1),                         # wholly outside, aimed at the frame
        S(0, 0.0, h / 2.0, w / 1.0, h / 2.0 + 1.0, half=float(h + w), bits=1, fill=9.0),   # half larger than the frame: every pixel
        S(0, 3.0, 3.0, 3.0, 3.0, half=2.0, bits=1),                                        # zero length: BAD
        S(0, np.nan, 3.0, 9.0, 3.0, half=2.0, bits=1),                                     # BAD beside good ones
        S(0, -1e5, -7e4, 2e5, 1.4e5 + 0.5 * h, half=1.5, bits=2, fill=10.0),               # end points far off the image
    ]


def random_segments(shape, frame, count, seed, short=False):
    h, w = shape
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        x1, y1 = rng.uniform(-0.3 * w - 2, 1.3 * w + 2), rng.uniform(-0.3 * h - 2, 1.3 * h + 2)
        if short:
            x2, y2 = x1 + rng.uniform(-12, 12), y1 + rng.uniform(-12, 12)
        else:
            x2, y2 = rng.uniform(-0.3 * w - 2, 1.3 * w + 2), rng.uniform(-0.3 * h - 2, 1.3 * h + 2)
        if rng.random() < 0.3:                                         # integer end points: centres on the band's edges
            x1, y1, x2, y2 = (float(round(v)) for v in (x1, y1, x2, y2))
            if (x1, y1) == (x2, y2):
                x2 += 1.0
        half = float(rng.choice([0.0, 0.5, 1.0, 2.0, 3.25, 0.7071067811865476]))
        cap = float(rng.choice([0.0, 3.0, np.inf])) if not short else float(rng.choice([0.0, 3.0]))
        out.append(MR.segment(frame, x1, y1, x2, y2, half=half, cap=cap, bits=int(rng.integers(1, 256)), fill=float(rng.integers(-50, 50)) / 4))
    return out


@functools.lru_cache(maxsize=None)
def case(shape):
    """(segments, restatement's mask, stats, counts) of a shape: computed once, shared, read-only"""
    segs = hand_made(shape) + random_segments(shape, 1, 12, 100 + shape[0]) + random_segments(shape, 0, 4, 200 + shape[1])
    segs += random_segments(shape, 3, 300, 300 + shape[0], short=shape[0] > 100)
    segs += [MR.segment(4, 1.0, 1.0, 1.0, 1.0, half=1.0), MR.segment(4, np.inf, 1.0, 2.0, 1.0, half=1.0)]
    segs = np.array(segs, MR.SEGMENT_DTYPE)
    order = np.random.default_rng(7).permutation(len(segs))           # frames interleaved: the library sorts them
    segs = segs[order]
    mask, stats, counts = MR.mask_trails(segs, (N_FRAMES, *shape))
    for a in (segs, mask, stats, counts):
        a.setflags(write=False)
    return segs, mask, stats, counts


def special_frames(shape, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 0.025, (N_FRAMES, *shape)).astype(np.float32)
    flat = f.reshape(-1)
    idx = rng.permutation(flat.size)
    q = max(1, flat.size // 8)
    flat[idx[:q]] = np.float32(-0.0)
    flat[idx[q:2 * q]] = np.inf
    flat[idx[2 * q:3 * q]] = -np.inf
    flat.view(np.uint32)[idx[3 * q:4 * q]] = np.uint32(0x7FC12345)                    # NaN with a payload
    flat.view(np.uint32)[idx[4 * q:5 * q]] = np.uint32(0xFFA00001)                    # a signalling one
    return f


def assert_equal(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} differ, first at {i}: device {got[i]!r}, restatement {want[i]!r}")


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_mask_counts_and_fill_equal_the_restatement(gpu_ctx, shape):
    segs, want_mask, want_stats, want_counts = case(shape)
    # mask only, no frames
    mask, stats, counts = gpu_ctx.mask_trails(None, segs, shape=(N_FRAMES, *shape))
    assert mask.dtype == np.uint8 and mask.shape == (N_FRAMES, *shape) and stats.dtype == MR.STAT_DTYPE and counts.dtype == np.int32
    assert_equal("mask", mask, want_mask)
    assert_equal("status", stats["status"], want_stats["status"])
    assert_equal("n_pix", stats["n_pix"], want_stats["n_pix"])
    assert_equal("frame_counts", counts, want_counts)
    assert counts[2] == 0 and counts[4] == 0 and not mask[2].any() and not mask[4].any()
    if shape[0] * shape[1] > 1:
        assert set(want_stats["status"].tolist()) == {MR.OK, MR.BAD_SEGMENT, MR.EMPTY}
    # value fill on frames of special values: the first segment's value, and no other pixel changes a bit
    frames = special_frames(shape, 5)
    want = frames.copy()
    MR.mask_trails(segs, (N_FRAMES, *shape), frames=want, fill="value")
    got = frames.copy()
    mask2, stats2, counts2 = gpu_ctx.mask_trails(got, segs, fill="value")
    assert_equal("filled frames", u32(got), u32(want))
    assert_equal("mask", mask2, want_mask)
    assert_equal("n_pix", stats2["n_pix"], want_stats["n_pix"])
    assert_equal("frame_counts", counts2, want_counts)
    assert np.array_equal(u32(got)[want_mask == 0], u32(frames)[want_mask == 0])


@pytest.mark.parametrize("fill", ["none", "zero", "nan", "value"])
def test_every_fill_mode_in_every_location(gpu_ctx, fill):
    import torch
    shape = (37, 130)
    segs, want_mask, want_stats, want_counts = case(shape)
    frames = special_frames(shape, 6)
    want = frames.copy()
    MR.mask_trails(segs, (N_FRAMES, *shape), frames=want if fill != "none" else None, fill=fill)
    if fill == "none":
        assert np.array_equal(u32(want), u32(frames))
    else:
        assert not np.array_equal(u32(want), u32(frames))
    # host
    got = frames.copy()
    mask, stats, counts = gpu_ctx.mask_trails(got, segs, fill=fill)
    assert_equal("host frames", u32(got), u32(want))
    assert_equal("host mask", mask, want_mask)
    # device frames: the mask is made on the device
    dev = torch.from_numpy(frames.copy()).cuda()
    dmask, stats, counts = gpu_ctx.mask_trails(dev, segs, fill=fill)
    assert dmask.is_cuda and dmask.dtype == torch.uint8
    assert_equal("device frames", u32(dev.cpu().numpy()), u32(want))
    assert_equal("device mask", dmask.cpu().numpy(), want_mask)
    assert_equal("n_pix", stats["n_pix"], want_stats["n_pix"])
    assert_equal("frame_counts", counts, want_counts)
    # device frames, host mask; host frames, device mask
    dev = torch.from_numpy(frames.copy()).cuda()
    hmask = np.full((N_FRAMES, *shape), 0xEE, np.uint8)
    out, _, _ = gpu_ctx.mask_trails(dev, segs, mask=hmask, fill=fill)
    assert out is hmask
    assert_equal("host mask of device frames", hmask, want_mask)
    assert_equal("device frames", u32(dev.cpu().numpy()), u32(want))
    got = frames.copy()
    dmask = torch.full((N_FRAMES, *shape), 0xEE, dtype=torch.uint8, device="cuda")
    gpu_ctx.mask_trails(got, segs, mask=dmask, fill=fill)
    assert_equal("device mask of host frames", dmask.cpu().numpy(), want_mask)
    assert_equal("host frames", u32(got), u32(want))
    # pinned frames and mask
    fb, mb = gpu_ctx.pinned_buffer(frames.nbytes), gpu_ctx.pinned_buffer(want_mask.nbytes)
    pf = fb.array.view(np.float32).reshape(frames.shape)
    pm = mb.array.view(np.uint8)[:want_mask.size].reshape(want_mask.shape)
    pf[...] = frames
    pm[...] = 0xEE
    _, stats, counts = gpu_ctx.mask_trails(pf, segs, mask=pm, fill=fill, pinned=True)
    assert_equal("pinned frames", u32(pf), u32(want))
    assert_equal("pinned mask", pm, want_mask)
    assert_equal("n_pix", stats["n_pix"], want_stats["n_pix"])
    del pf, pm
    fb.close()
    mb.close()


def test_or_onto_a_plane_of_random_bytes_and_fill_only(gpu_ctx):
    import torch
    shape = (37, 130)
    segs, want_mask, want_stats, want_counts = case(shape)
    old = np.random.default_rng(8).integers(0, 256, (N_FRAMES, *shape)).astype(np.uint8)
    want = MR.mask_trails(segs, (N_FRAMES, *shape), mask=old.copy(), clear=False)[0]
    assert np.array_equal(want, old | want_mask) and not np.array_equal(want, old)
    got = old.copy()
    out, stats, counts = gpu_ctx.mask_trails(None, segs, mask=got, clear=False)
    assert out is got
    assert_equal("ORed host mask", got, want)
    assert_equal("n_pix", stats["n_pix"], want_stats["n_pix"])                      # the counts are of this call's segments
    assert_equal("frame_counts", counts, want_counts)
    dev = torch.from_numpy(old.copy()).cuda()
    gpu_ctx.mask_trails(None, segs, mask=dev, clear=False)
    assert_equal("ORed device mask", dev.cpu().numpy(), want)
    # clear=True on the same planes
    got = old.copy()
    gpu_ctx.mask_trails(None, segs, mask=got, clear=True)
    assert_equal("cleared host mask", got, want_mask)
    dev = torch.from_numpy(old.copy()).cuda()
    gpu_ctx.mask_trails(None, segs, mask=dev)
    assert_equal("cleared device mask", dev.cpu().numpy(), want_mask)
    # fill only: no mask
    frames = special_frames(shape, 9)
    wantf = frames.copy()
    MR.mask_trails(segs, (N_FRAMES, *shape), frames=wantf, fill="zero")
    got = frames.copy()
    none, stats, counts = gpu_ctx.mask_trails(got, segs, mask=False, fill="zero")
    assert none is None
    assert_equal("filled frames", u32(got), u32(wantf))
    assert_equal("n_pix", stats["n_pix"], want_stats["n_pix"])
    assert_equal("frame_counts", counts, want_counts)
    # a single 2-d frame and plane; no segments at all
    one = np.array([MR.segment(0, 2.0, 5.0, 100.0, 20.0, half=2.0, bits=5)], MR.SEGMENT_DTYPE)
    m2, s2, c2 = gpu_ctx.mask_trails(None, one, shape=shape)
    w2, ws2, wc2 = MR.mask_trails(one, (1, *shape))
    assert m2.shape == shape and np.array_equal(m2, w2[0]) and s2.tolist() == ws2.tolist() and c2.tolist() == wc2.tolist()
    got = old.copy()
    _, s0, c0 = gpu_ctx.mask_trails(None, np.zeros(0, MR.SEGMENT_DTYPE), mask=got)
    assert not got.any() and len(s0) == 0 and c0.tolist() == [0] * N_FRAMES


def test_refusals_touch_nothing_and_name_the_call(gpu_ctx):
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (24, 70)
    n = 2
    frames = special_frames(shape, 10)[:n].copy()
    keep = frames.copy()
    mask = np.full((n, *shape), 0xA5, np.uint8)
    good = np.array([MR.segment(1, 0.0, 5.0, 69.0, 9.0, half=2.0, bits=3)], MR.SEGMENT_DTYPE)
    lib = _native.lib()

    def refused(segs=good, n_seg=None, fr=frames, dtype=_native.F32, nn=n, h=shape[0], w=shape[1], fill=_native.MASK_FILL_ZERO, m=mask,
                null_segs=False):
        p = _native.MaskParamsStruct(fill, 1)
        stats = np.full(len(segs), -7, MR.STAT_DTYPE)
        rc = lib.lfdmi_mask_trails(gpu_ctx._h, _native._ptr(fr), dtype, nn, h, w, _native.HOST, None if null_segs else _native._ptr(segs),
                                   len(segs) if n_seg is None else n_seg, C.byref(p), _native._ptr(m), _native.HOST, _native._ptr(stats), None)
        assert rc == _native.ERR_ARG
        assert "lfdmi_mask_trails" in lib.lfdmi_last_error(gpu_ctx._h).decode()
        assert np.array_equal(u32(frames), u32(keep)) and (mask == 0xA5).all()

    for f in (-1, n):
        bad = good.copy()
        bad["frame"] = f
        refused(bad)
    bad = good.copy()
    bad["bits"] = 0
    refused(bad)
    refused(fill=4)
    refused(fill=-1)
    refused(fr=None)                                                              # a fill without frames
    refused(fill=_native.MASK_FILL_NONE, m=None)                                  # neither a mask nor a fill
    refused(null_segs=True)
    refused(h=40000, w=40000)                                                     # h * w above 1e9 (refused before anything is read)
    refused(dtype=_native.F32_BE)                                                 # a fill of big-endian frames
    refused(nn=-1)
    # through the binding: the same codes as exceptions
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.mask_trails(frames.astype(">f4"), good, fill="nan")
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(ValueError):
        gpu_ctx.mask_trails(frames, good, fill="median")
    with pytest.raises(ValueError):
        gpu_ctx.mask_trails(frames, good, mask=np.zeros((n, shape[0], shape[1] + 1), np.uint8))
    with pytest.raises(TypeError):
        gpu_ctx.mask_trails(frames, good, mask=np.zeros((n, *shape), np.int8))
    with pytest.raises(ValueError):
        gpu_ctx.mask_trails(None, good)
    # big-endian frames are fine where nothing is filled
    be_mask, _, _ = gpu_ctx.mask_trails(frames.astype(">f4"), good)
    assert np.array_equal(be_mask, MR.mask_trails(good, (n, *shape))[0])
    # while a detect_batch_begin is in flight
    pb, pd, _ = default_params()
    dev = torch.from_numpy(np.random.default_rng(6).normal(0, 0.025, (2, 384, 640)).astype(np.float32)).cuda()
    with _native.Context(0, 384, 640, 2) as c2:
        pend = c2.detect_batch_begin(dev, pb, pd)
        with pytest.raises(_native.NativeError):
            c2.mask_trails(frames, good, mask=mask, fill="zero")
        pend.result()
        assert np.array_equal(u32(frames), u32(keep)) and (mask == 0xA5).all()
        got = frames.copy()
        m, _, _ = c2.mask_trails(got, good, fill="zero")
    want = frames.copy()
    wm = MR.mask_trails(good, (n, *shape), frames=want, fill="zero")[0]
    assert np.array_equal(m, wm) and np.array_equal(u32(got), u32(want))
    # and the session's context still works after every refusal
    assert np.array_equal(gpu_ctx.mask_trails(None, good, shape=(n, *shape))[0], wm)


def test_a_masked_trail_is_not_found_again(gpu_ctx):
    """inject -> search_lines -> segments_from_radon_lines -> mask_trails(fill="zero") -> search_lines: a zeroed pixel is invalid
    to the search by its own step 1, so the second search has no line where the first one's was, and it equals the restatement
    of the search on the filled frames as every search must"""
    import torch
    import test_gpu_radon_lines as TGL
    import test_radon_model as TM
    from lfd_amd import _native, masks
    n = 2
    tr, table, step = TM.trail_plan()
    tr = tr[:n].copy()
    frames = torch.from_numpy(TM.noise_frames()[:n].copy()).cuda()
    gpu_ctx.inject_trails(frames, tr, table, step)
    lp = dict(max_lines=2, peel_halfwidth=8, min_seg=64)
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=n, bin=2) as r:
        first, first_n = r.search_lines(frames, sigma=TM.SET_SIGMA, **lp)
        assert (first_n >= 1).all()
        for i in range(n):
            ang, dist = TM.line_error(first[i, 0], tr[i], TM.SET_SHAPE)
            assert ang <= 0.5 and dist <= 4.0                                     # the injected trail
        segs, where = masks.segments_from_radon_lines(first, first_n, cap=np.inf)
        assert len(segs) == int(first_n.sum()) and (segs["half"] == 10.0).all()
        before = frames.cpu().numpy()
        mask, stats, counts = gpu_ctx.mask_trails(frames, segs, fill="zero")
        filled = frames.cpu().numpy()
        want = before.copy()
        want_mask, want_stats, want_counts = MR.mask_trails(segs, (n, *TM.SET_SHAPE), frames=want, fill="zero")
        assert np.array_equal(u32(filled), u32(want)) and np.array_equal(mask.cpu().numpy(), want_mask)
        assert stats.tolist() == want_stats.tolist() and counts.tolist() == want_counts.tolist() and (counts > 0).all()
        again, again_n = r.search_lines(frames, sigma=TM.SET_SIGMA, **lp)
        for i in range(n):
            for k in range(int(again_n[i])):
                ang, dist = TM.line_error(again[i, k], tr[i], TM.SET_SHAPE)
                assert not (ang <= 1.0 and dist <= lp["peel_halfwidth"]), (i, k, ang, dist)
        TGL.check_lines(filled, again, again_n, TM.SET_SIGMA, bin=2, **lp)
