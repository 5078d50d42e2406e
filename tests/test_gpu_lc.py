"""Light curves on the device against the numpy restatement of include/lfdmi.h (tests/lc_ref.py): every integer and every bit of
every double of the segment and section records, over the shapes at which the 64 x 16 tiling can go wrong, every kind of segment
and pixel, the parameters' ends, every buffer location, with and without a mask plane; the refusals; and the composition with
the injection, the faint-trail search and the trail masks' segment builders."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

# 1 x 1; one side of each tile edge (tiles are 64 wide, 16 high); w % 4 != 0 with partial tiles on both axes; a crop of eight
# tile columns by 24 tile rows
SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (37, 130), (372, 512)]
N_FRAMES = 5          # frame 2 carries no segment, frame 3 three hundred (more than two LDS chunks of 128), frame 4 only bad ones
MAX_SEC = 256
PARAMS = dict(sec_len=8.0, min_core=4, min_sky=4)        # sec_len 8: the most sections a tile can hold


def hand_made(shape):
    """segments of frame 0: every direction, reach and band the definition distinguishes"""
    h, w = shape
    m = min(h, w)
    S = LR.segment
    c, s = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    nan, inf = np.nan, np.inf
    return [
        S(0, 0.0, h // 2, w - 1.0, h // 2, half=2.0, bg_in=3.0, bg_out=6.0),              # axis-aligned, integer ends: t * inv on the section
        S(0, w // 2, 0.0, w // 2, h - 1.0, half=1.0, bg_in=2.0, bg_out=5.0),              # boundaries, centres on half, bg_in, bg_out; vertical
        S(0, w // 3, h - 1.0, w // 3, 0.0, half=3.0, bg_in=3.0, bg_out=7.0),              # vertical, downwards, bg_in == half
        S(0, 0.0, 0.0, m - 1.0, m - 1.0, half=1.5, bg_in=2.5, bg_out=6.0),                # 45 degrees
        S(0, w - 1.0, 0.0, w - 1.0 - m, float(m), half=2.0, bg_in=4.0, bg_out=8.0),       # 135 degrees
        S(0, -10.0, h / 3.0, w + 10.0, h / 3.0 + 2.3, half=1.7, bg_in=4.0, bg_out=9.5),   # shallow, ends outside
        S(0, w / 2.0 - 1.3, -5.0, w / 2.0 + 2.9, h + 4.0, half=2.25, bg_in=3.0, bg_out=11.0),   # steep, ends outside
        S(0, w / 2 - 1000 * c, h / 2 - 1000 * s, w / 2 + 1000 * c, h / 2 + 1000 * s, half=10.0),   # a results row: 250 sections
        S(0, w + 100.0, h + 100.0, w + 200.0, h + 150.0, half=3.0),                       # wholly outside: EMPTY
        S(0, 1.0, h // 3, 17.0, h // 3, half=2.0, bg_in=2.0, bg_out=4.0),                 # t == L on the centre of pixel 17: the last section
        S(0, -1000.0, h // 2 + 1.0, 1048.0, h // 2 + 1.0, half=2.0),                      # n_sec == max_sections
        S(0, -1000.0, h // 2 + 1.0, 1049.0, h // 2 + 1.0, half=2.0),                      # one more: TOO_LONG
        S(0, 0.0, h / 2.0, w / 1.0, h / 2.0 + 1.0, half=60.0, bg_in=60.0, bg_out=64.0),   # half larger than the (small) frames
        S(0, 2.0, 2.0, 40.0, 12.0, half=2.0), S(0, 2.0, 12.0, 40.0, 2.0, half=2.0),       # two that cross inside one tile
        S(0, nan, 3.0, 9.0, 3.0), S(0, 1.0, inf, 9.0, 3.0), S(0, 1.0, 3.0, 1.5e6, 3.0), S(0, 3.0, 3.0, 3.0, 3.0),   # every BAD reason
        S(0, 1.0, 3.0, 9.0, 3.0, half=nan, bg_in=5.0, bg_out=6.0), S(0, 1.0, 3.0, 9.0, 3.0, half=inf, bg_in=5.0, bg_out=6.0),
        S(0, 1.0, 3.0, 9.0, 3.0, half=0.0, bg_in=5.0, bg_out=6.0), S(0, 1.0, 3.0, 9.0, 3.0, half=-1.0, bg_in=5.0, bg_out=6.0),
        S(0, 1.0, 3.0, 9.0, 3.0, half=2.0, bg_in=nan, bg_out=6.0), S(0, 1.0, 3.0, 9.0, 3.0, half=2.0, bg_in=3.0, bg_out=nan),
        S(0, 1.0, 3.0, 9.0, 3.0, half=2.0, bg_in=1.0, bg_out=6.0), S(0, 1.0, 3.0, 9.0, 3.0, half=2.0, bg_in=5.0, bg_out=4.0),
        S(0, 1.0, 3.0, 9.0, 3.0, half=2.0, bg_in=5.0, bg_out=64.5),
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
        if rng.random() < 0.3:                                         # integer end points: centres on the bands' edges
            x1, y1, x2, y2 = (float(round(v)) for v in (x1, y1, x2, y2))
            if (x1, y1) == (x2, y2):
                x2 += 1.0
        half = float(rng.choice([0.5, 1.0, 2.0, 3.25, 0.7071067811865476, 8.0]))
        gap = float(rng.choice([0.0, 1.0, 4.0]))
        out.append(LR.segment(frame, x1, y1, x2, y2, half=half, bg_in=half + gap, bg_out=min(half + gap + float(rng.choice([0.0, 3.0, 16.0])), 64.0)))
    return out


def special_frames(shape, seed, n=N_FRAMES, clip=0.125):
    """noise of sigma 0.025 with every kind of pixel step 1 distinguishes strewn over it"""
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 0.025, (n, *shape)).astype(np.float32)
    flat = f.reshape(-1)
    bits = flat.view(np.uint32)
    idx = rng.permutation(flat.size)
    q = max(1, flat.size // 24)
    clipf = np.float32(clip)
    kinds = [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), clipf, -clipf,
             np.nextafter(clipf, np.float32(np.inf)), -np.nextafter(clipf, np.float32(np.inf)), np.nextafter(clipf, np.float32(0))]
    for k, v in enumerate(kinds):
        flat[idx[k * q:(k + 1) * q]] = v
    k = len(kinds)
    bits[idx[k * q:(k + 1) * q]] = np.uint32(0x7FC12345)                # NaN with a payload
    bits[idx[(k + 1) * q:(k + 2) * q]] = np.uint32(0xFFA00001)          # a signalling one
    sel = idx[(k + 2) * q:(k + 3) * q]                                  # denormals of both signs, the smallest and the largest too
    bits[sel] = rng.integers(1, 0x800000, len(sel)).astype(np.uint32) | (rng.integers(0, 2, len(sel)).astype(np.uint32) << np.uint32(31))
    if len(sel) > 1:
        bits[sel[0]], bits[sel[1]] = np.uint32(1), np.uint32(0x807FFFFF)
    sel = idx[(k + 3) * q:(k + 5) * q]                                  # ties of v * 2^30 at .5: odd multiples of 2^-31
    odd = (2 * rng.integers(0, 1 << 22, len(sel)) + 1).astype(np.float64) * 2.0 ** -31
    flat[sel] = (odd * rng.choice([-1.0, 1.0], len(sel))).astype(np.float32)
    assert np.array_equal(flat[sel].astype(np.float64) * 2.0 ** 31 % 2, np.ones(len(sel)))
    return f


def plane(shape, seed, n=N_FRAMES):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, *shape)) * (rng.random((n, *shape)) < 0.3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(segments, frames, restatement's records and sections) of a shape: computed once, shared, read-only"""
    segs = hand_made(shape) + random_segments(shape, 1, 12, 100 + shape[0]) + random_segments(shape, 0, 4, 200 + shape[1])
    segs += random_segments(shape, 3, 300, 300 + shape[0], short=shape[0] > 100)
    segs += [LR.segment(4, 1.0, 1.0, 1.0, 1.0), LR.segment(4, np.inf, 1.0, 2.0, 1.0)]
    segs = np.array(segs, LR.SEGMENT_DTYPE)
    segs = segs[np.random.default_rng(7).permutation(len(segs))]        # frames interleaved: the library sorts them
    frames = special_frames(shape, 5)
    rec, sec = LR.light_curves(frames, segs, max_sections=MAX_SEC, **PARAMS)
    for a in (segs, frames, rec, sec):
        a.setflags(write=False)
    return segs, frames, rec, sec


def assert_same(what, got, want):
    """every field of two record arrays: integers equal, doubles equal in every bit"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for k in want.dtype.names:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            i = tuple(bad[0])
            raise AssertionError(f"{what}.{k}: {len(bad)} differ, first at {i}: device {got[k][i]!r}, restatement {want[k][i]!r}")
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_records_and_sections_equal_the_restatement(gpu_ctx, shape):
    segs, frames, want, want_sec = case(shape)
    rec, sec = gpu_ctx.light_curves(frames, segs, max_sections=MAX_SEC, **PARAMS)
    assert rec.dtype == LR.LC_DTYPE and sec.dtype == LR.SECTION_DTYPE and sec.shape == (len(segs), MAX_SEC)
    assert_same("sections", sec, want_sec)
    assert_same("records", rec, want)
    got = set(want["status"].tolist())
    assert {LR.BAD_SEGMENT, LR.TOO_LONG, LR.EMPTY} <= got
    on4 = segs["frame"] == 4
    assert (rec["status"][on4] == LR.BAD_SEGMENT).all() and not sec[on4].view(np.uint8).any()
    if shape[0] > 30:
        assert LR.OK in got and {LR.SEC_OK, LR.SEC_LOW, LR.SEC_EMPTY} <= set(want_sec["status"][want["status"] == LR.OK].reshape(-1).tolist())
        assert int(want["n_sec"].max()) == MAX_SEC
    # the same frames big-endian, and with a mask plane
    be, _ = gpu_ctx.light_curves(frames.astype(">f4"), segs, max_sections=MAX_SEC, **PARAMS)
    assert_same("big-endian records", be, want)
    m = plane(shape, 11)
    wm, wm_sec = LR.light_curves(frames, segs, mask=m, skip_bits=0x05, max_sections=MAX_SEC, **PARAMS)
    rec, sec = gpu_ctx.light_curves(frames, segs, mask=m, skip_bits=0x05, max_sections=MAX_SEC, **PARAMS)
    assert_same("masked sections", sec, wm_sec)
    assert_same("masked records", rec, wm)
    if shape[0] > 30:
        assert int(wm_sec["n_core"].sum()) < int(want_sec["n_core"].sum())
        assert np.array_equal(wm_sec["n_geom"], want_sec["n_geom"])                # (n_geom counts invalid pixels too)


@pytest.mark.parametrize("params", [dict(sec_len=16.0, min_core=4, min_sky=4), dict(sec_len=4096.0, min_core=1, min_sky=1), {},
                                    dict(sec_len=8.5, clip=0.05, min_core=40, min_sky=2)],
                         ids=["sec16", "sec4096", "defaults", "clip"])
def test_parameters_in_every_location(gpu_ctx, params):
    import torch
    shape = (37, 130)
    segs, frames, _, _ = case(shape)
    ms = 128 if params.get("sec_len", 32.0) > 8.5 else MAX_SEC
    sigma = np.linspace(0.02, 0.05, N_FRAMES).astype(np.float32)
    m = plane(shape, 12)
    for mask, skip in ((None, 0), (m, 0xFF), (m, 0x10), (m, 0)):
        want, want_sec = LR.light_curves(frames, segs, mask=mask, skip_bits=skip, sigma=sigma, max_sections=ms, **params)
        kw = dict(skip_bits=skip, sigma=sigma, max_sections=ms, **params)
        # host
        rec, sec = gpu_ctx.light_curves(frames, segs, mask=mask, **kw)
        assert_same("host sections", sec, want_sec)
        assert_same("host records", rec, want)
        # device: the frames and the plane are used where they are
        dev = torch.from_numpy(frames.copy()).cuda()
        dmask = None if mask is None else torch.from_numpy(mask).cuda()
        rec, sec = gpu_ctx.light_curves(dev, segs, mask=dmask, **kw)
        assert_same("device sections", sec, want_sec)
        assert_same("device records", rec, want)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), frames.view(np.uint32))     # frames are only read
        # pinned, big-endian
        fb, mb = gpu_ctx.pinned_buffer(frames.nbytes), gpu_ctx.pinned_buffer(m.nbytes)
        pf = fb.array.view(">f4")[:frames.size].reshape(frames.shape)
        pm = mb.array.view(np.uint8)[:m.size].reshape(m.shape)
        pf[...] = frames
        pm[...] = m
        rec, sec = gpu_ctx.light_curves(pf, segs, mask=None if mask is None else pm, pinned=True, **kw)
        assert_same("pinned sections", sec, want_sec)
        assert_same("pinned records", rec, want)
        del pf, pm
        fb.close()
        mb.close()
    if "sec_len" in params and params["sec_len"] == 4096.0:
        assert int(want["n_sec"].max()) == 1
    # a single 2-d frame; a scalar sigma; no segments at all
    one = np.array([LR.segment(0, 2.0, 5.0, 120.0, 20.0, half=2.0)], LR.SEGMENT_DTYPE)
    rec, sec = gpu_ctx.light_curves(frames[1], one, sigma=0.03, max_sections=32, **params)
    want, want_sec = LR.light_curves(frames[1], one, sigma=0.03, max_sections=32, **params)
    assert_same("2-d sections", sec, want_sec)
    assert_same("2-d records", rec, want)
    rec, sec = gpu_ctx.light_curves(frames, np.zeros(0, LR.SEGMENT_DTYPE), max_sections=4)
    assert rec.shape == (0,) and sec.shape == (0, 4)


def test_the_fixed_point_range_and_a_misaligned_device_buffer(gpu_ctx):
    """values of +-1024 at clip 1024 across whole sections (|q| = 2^40, the largest), and device frames that start 4 bytes off a
    16-byte boundary (the 16-byte loads are not taken)"""
    import torch
    shape = (40, 192)
    frames = np.full((2, *shape), 1024.0, np.float32)
    frames[0, :, 96:] = -1024.0
    with np.errstate(invalid="ignore"):                                  # (the signalling NaNs among the special pixels)
        frames[1] = special_frames(shape, 21, n=1, clip=1024.0)[0] * np.float32(4000.0)
    frames[1, 10:14, 20:60] = np.float32(1024.0)
    frames[1, 14:16, 20:60] = np.nextafter(np.float32(1024.0), np.float32(np.inf))
    segs = np.array([LR.segment(0, 0.0, 20.0, 191.0, 20.0, half=8.0, bg_in=10.0, bg_out=18.0),
                     LR.segment(1, 3.0, 4.0, 180.0, 33.0, half=6.0, bg_in=8.0, bg_out=20.0),
                     LR.segment(0, 5.0, 35.0, 150.0, 2.0, half=3.0)], LR.SEGMENT_DTYPE)
    kw = dict(max_sections=16, sec_len=64.0, clip=1024.0, min_core=4, min_sky=4)
    want, want_sec = LR.light_curves(frames, segs, **kw)
    assert int(want_sec[0, 0]["q_core"]) == int(want_sec[0, 0]["n_core"]) << 40 and want_sec[0, 0]["mean"] == 1024.0
    assert int(want_sec[0, 2]["q_core"]) == -(int(want_sec[0, 2]["n_core"]) << 40)
    rec, sec = gpu_ctx.light_curves(frames, segs, **kw)
    assert_same("sections", sec, want_sec)
    assert_same("records", rec, want)
    buf = torch.zeros(frames.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(frames.reshape(-1)).cuda()
    off = buf[1:].view(2, *shape)
    assert off.data_ptr() % 16 == 4
    mbuf = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    rec, sec = gpu_ctx.light_curves(off, segs, mask=mbuf[1:].view(2, *shape), skip_bits=0xFF, **kw)
    assert_same("misaligned sections", sec, want_sec)
    assert_same("misaligned records", rec, want)


def test_refusals_touch_nothing_and_name_the_call(gpu_ctx):
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (24, 70)
    n = 2
    frames = special_frames(shape, 10)[:n].copy()
    good = np.array([LR.segment(1, 0.0, 5.0, 69.0, 9.0, half=2.0)], LR.SEGMENT_DTYPE)
    lib = _native.lib()
    P = _native.LcParamsStruct

    def refused(segs=good, n_seg=None, fr=frames, dtype=_native.F32, nn=n, h=shape[0], w=shape[1], loc=_native.HOST, p=P(32.0, 0.125, 32, 32),
                sigma=None, ms=8, skip=0, null_out=False, null_sec=False, null_segs=False):
        out = np.full(len(segs), -7, np.int8).repeat(LR.LC_DTYPE.itemsize).view(LR.LC_DTYPE)
        sec = np.full(len(segs) * 8 * LR.SECTION_DTYPE.itemsize, 0xA5, np.uint8)
        rc = lib.lfdmi_light_curves(gpu_ctx._h, _native._ptr(fr), dtype, nn, h, w, loc, None, skip, None if null_segs else _native._ptr(segs),
                                    len(segs) if n_seg is None else n_seg, _native._ptr(sigma), C.byref(p), None if null_out else _native._ptr(out),
                                    None if null_sec else _native._ptr(sec), ms)
        assert rc == _native.ERR_ARG
        assert lib.lfdmi_last_error(gpu_ctx._h).decode() != ""
        assert (out.view(np.int8) == -7).all() and (sec == 0xA5).all()

    for f in (-1, n):
        bad = good.copy()
        bad["frame"] = f
        refused(bad)
    refused(dtype=_native.U8)
    refused(dtype=_native.F64)
    refused(loc=3)
    refused(nn=-1)
    refused(n_seg=-1)
    refused(h=0)
    refused(w=70000)
    refused(h=40000, w=40000)
    refused(fr=None)
    refused(null_segs=True)
    refused(null_out=True)
    refused(null_sec=True)
    refused(ms=0)
    refused(ms=_native.LC_MAX_SECTIONS + 1)
    refused(skip=256)
    refused(skip=-1)
    for p in (P(7.9, 0.125, 32, 32), P(4097.0, 0.125, 32, 32), P(float("nan"), 0.125, 32, 32), P(32.0, 0.0, 32, 32), P(32.0, -1.0, 32, 32),
              P(32.0, float("inf"), 32, 32), P(32.0, float("nan"), 32, 32), P(32.0, 1025.0, 32, 32), P(32.0, 0.125, 0, 32), P(32.0, 0.125, 32, 0)):
        refused(p=p)
    for s in ([0.025, 0.0], [0.025, -1.0], [np.nan, 0.025], [np.inf, 0.025]):
        refused(sigma=np.array(s, np.float32))
    assert "lfdmi_light_curves" in lib.lfdmi_last_error(gpu_ctx._h).decode()
    # through the binding: the same code as an exception; the Python-side checks
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.light_curves(frames, good, sec_len=4.0)
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(TypeError):
        gpu_ctx.light_curves(frames, good, section=4.0)
    with pytest.raises(ValueError):
        gpu_ctx.light_curves(frames, good, mask=np.zeros((n, shape[0], shape[1] + 1), np.uint8))
    with pytest.raises(TypeError):
        gpu_ctx.light_curves(frames, good, mask=np.zeros((n, *shape), np.int8))
    with pytest.raises(ValueError):
        gpu_ctx.light_curves(frames, good, mask=torch.zeros((n, *shape), dtype=torch.uint8, device="cuda"))
    # while a detect_batch_begin is in flight
    pb, pd, _ = default_params()
    dev = torch.from_numpy(np.random.default_rng(6).normal(0, 0.025, (2, 384, 640)).astype(np.float32)).cuda()
    want, want_sec = LR.light_curves(frames, good, max_sections=8, sec_len=16.0, min_core=4, min_sky=4)
    with _native.Context(0, 384, 640, 2) as c2:
        pend = c2.detect_batch_begin(dev, pb, pd)
        with pytest.raises(_native.NativeError):
            c2.light_curves(frames, good)
        pend.result()
        rec, sec = c2.light_curves(frames, good, max_sections=8, sec_len=16.0, min_core=4, min_sky=4)
    assert_same("sections", sec, want_sec)
    assert_same("records", rec, want)
    # and the session's context still works after every refusal
    rec, sec = gpu_ctx.light_curves(frames, good, max_sections=8, sec_len=16.0, min_core=4, min_sky=4)
    assert_same("sections", sec, want_sec)
    assert want["status"][0] == LR.OK


def test_a_trail_twice_as_bright_in_its_second_half(gpu_ctx):
    """inject two extents of amplitude ratio 2 on one line -> search_lines finds the line -> segments_from_radon_lines ->
    lightcurve.segments_from_mask_segments -> light_curves: the device's records equal the restatement's, and the brighter half's
    rate exceeds the fainter half's by more than 3 errors of the difference"""
    import torch
    import test_radon_model as TM
    from lfd_amd import _native, lightcurve, masks, recovery
    tr0, table, step = TM.trail_plan()
    tr0 = tr0[0]
    ta, tb = recovery.extent(float(tr0["rho"]), float(tr0["theta"]), -np.inf, np.inf, TM.SET_SHAPE)
    tm = 0.5 * (ta + tb)
    tr = np.array([tr0, tr0], tr0.dtype)
    tr[0]["t0"], tr[0]["t1"] = -np.inf, tm
    tr[1]["t0"], tr[1]["t1"], tr[1]["amplitude"] = np.nextafter(tm, np.inf), np.inf, 2.0 * float(tr0["amplitude"])
    frames = torch.from_numpy(TM.noise_frames()[:1].copy()).cuda()
    gpu_ctx.inject_trails(frames, tr, table, step)
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=1, bin=2) as r:
        lines, nl = r.search_lines(frames, sigma=TM.SET_SIGMA, max_lines=1, peel_halfwidth=8, min_seg=64)
    assert int(nl[0]) == 1
    ang, dist = TM.line_error(lines[0, 0], tr0, TM.SET_SHAPE)
    assert ang <= 0.5 and dist <= 4.0
    msegs, where = masks.segments_from_radon_lines(lines, nl)
    segs = lightcurve.segments_from_mask_segments(msegs)
    assert len(segs) == 1 and segs[0]["half"] == 10.0 and segs[0]["bg_in"] == 14.0 and segs[0]["bg_out"] == 30.0
    rec, sec = lightcurve.light_curves(gpu_ctx, frames, segs, sigma=TM.SET_SIGMA)
    want, want_sec = LR.light_curves(frames.cpu().numpy(), segs, sigma=TM.SET_SIGMA)
    assert_same("sections", sec, want_sec)
    assert_same("records", rec, want)
    assert rec[0]["status"] == LR.OK and rec[0]["n_ok"] >= 6
    # the sections wholly on either side of the injected break, in the injection's t (d = (-sin, cos) from the foot point)
    s = segs[0]
    L = math.hypot(s["x2"] - s["x1"], s["y2"] - s["y1"])
    ex, ey = (s["x2"] - s["x1"]) / L, (s["y2"] - s["y1"]) / L
    c, sn = math.cos(tr0["theta"]), math.sin(tr0["theta"])
    def inj_t(t):
        x, y = s["x1"] + t * ex, s["y1"] + t * ey
        return (x - tr0["rho"] * c) * -sn + (y - tr0["rho"] * sn) * c
    halves = ([], [])
    for j in range(int(rec[0]["n_sec"])):
        o = sec[0, j]
        if o["status"] != LR.SEC_OK:
            continue
        a, b = inj_t(o["t0"]), inj_t(o["t1"])
        if max(a, b) < tm - 2.0:
            halves[0].append(o)
        elif min(a, b) > tm + 2.0:
            halves[1].append(o)
    assert len(halves[0]) >= 3 and len(halves[1]) >= 3
    mean = [sum(o["n_core"] * o["rate"] for o in hv) / sum(o["n_core"] for o in hv) for hv in halves]
    err = [1.0 / math.sqrt(sum(1.0 / o["rate_err"] ** 2 for o in hv)) for hv in halves]
    print("first half %.4f +- %.4f, second half %.4f +- %.4f (truth 0.1003, 0.2005)" % (mean[0], err[0], mean[1], err[1]))
    assert mean[1] - mean[0] > 3.0 * math.hypot(err[0], err[1])
    assert float(lightcurve.variability(rec)[0]) > 3.0                                  # not a constant trail
