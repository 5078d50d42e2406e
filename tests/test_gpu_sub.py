"""Trail subtraction on the device against the numpy restatement of include/lfdmi.h (tests/sub_ref.py): every bit of every pixel,
every integer and every bit of every double of the records and every bit of the model tables, over the shapes at which the
64 x 16 tiling can go wrong, every kind of segment and pixel, the parameters' ends, every buffer location, with and without a
mask plane; that no pixel outside every band changes; apply = 0; crossings; the refusals; and the composition with the
injection, the faint-trail search and the trail masks' segment builders."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sub_ref as UR  # noqa: E402
from test_gpu_strips import assert_same, plane, random_segments, special_frames  # noqa: E402

pytestmark = pytest.mark.gpu

# 1 x 1; one side of each tile edge (tiles are 64 wide, 16 high); w % 4 != 0 with partial tiles on both axes; a crop of eight
# tile columns by 24 tile rows
SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (37, 130), (372, 512)]
N_FRAMES = 5          # frame 2 carries no segment, frame 3 three hundred (more than two LDS chunks of 128), frame 4 only bad ones
MAX_SEC = 256
MAX_CELLS = 256 * 29  # 256 sections of a half-14 band at step 1
PARAMS = dict(sec_len=8.0, wing=1.0, min_n=2, min_wing=2, smooth=2, min_sec=2)


def hand_made(shape):
    """segments of frame 0, the list of test_gpu_strips.py: every direction, reach and band the definition distinguishes"""
    h, w = shape
    m = min(h, w)
    S = UR.segment
    c, s = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    nan, inf = np.nan, np.inf
    return [
        S(0, 0.0, h // 2, w - 1.0, h // 2, half=2.0),                                     # axis-aligned, integer ends: centres on +-half
        S(0, w // 2, 0.0, w // 2, h - 1.0, half=1.0),                                     # vertical
        S(0, w // 3, h - 1.0, w // 3, 0.0, half=3.0),                                     # vertical, downwards
        S(0, 0.0, 0.0, m - 1.0, m - 1.0, half=1.5),                                       # 45 degrees
        S(0, w - 1.0, 0.0, w - 1.0 - m, float(m), half=2.0),                              # 135 degrees
        S(0, -10.0, h / 3.0, w + 10.0, h / 3.0 + 2.3, half=1.7),                          # shallow, ends outside
        S(0, w / 2.0 - 1.3, -5.0, w / 2.0 + 2.9, h + 4.0, half=2.25),                     # steep, ends outside
        S(0, w / 2 - 1000 * c, h / 2 - 1000 * s, w / 2 + 1000 * c, h / 2 + 1000 * s, half=14.0),   # a results row: 250 sections of 29 bins
        S(0, w + 100.0, h + 100.0, w + 200.0, h + 150.0, half=3.0),                       # wholly outside: EMPTY
        S(0, 1.0, h // 3, 17.0, h // 3, half=2.0),                                        # t == L on the centre of pixel 17
        S(0, -1000.0, h // 2 + 1.0, 1048.0, h // 2 + 1.0, half=14.0),                     # n_sec == max_sections, n_sec * n_off == max_cells
        S(0, -1000.0, h // 2 + 1.0, 1049.0, h // 2 + 1.0, half=2.0),                      # one section more: TOO_LONG
        S(0, -1000.0, h // 2 + 1.0, 1048.0, h // 2 + 1.0, half=14.6),                     # 31 bins, one cell row more than fits: TOO_LONG
        S(0, -1000.0, h // 2 + 1.0, 1040.0, h // 2 + 1.0, half=14.6),                     # 255 x 31 > 256 x 29: TOO_LONG
        S(0, 0.0, h / 2.0, min(w, 200) / 1.0, h / 2.0 + 1.0, half=60.0),                  # half larger than the (small) frames: 121 bins
        S(0, 2.0, 2.0, 40.0, 12.0, half=2.0), S(0, 2.0, 12.0, 40.0, 2.0, half=2.0),       # two that cross inside one tile
        S(0, 3.0, 5.0, 60.0, 9.0, half=0.5),                                              # K = 0: one bin
        S(0, nan, 3.0, 9.0, 3.0), S(0, 1.0, inf, 9.0, 3.0), S(0, 1.0, 3.0, 1.5e6, 3.0), S(0, 3.0, 3.0, 3.0, 3.0),   # every BAD reason
        S(0, 1.0, 3.0, 9.0, 3.0, half=nan), S(0, 1.0, 3.0, 9.0, 3.0, half=inf), S(0, 1.0, 3.0, 9.0, 3.0, half=0.0),
        S(0, 1.0, 3.0, 9.0, 3.0, half=-1.0), S(0, 1.0, 3.0, 9.0, 3.0, half=64.6),         # (the last: 131 bins, past MAX_OFF)
    ]


def sky_frames(shape, seed):
    """special_frames (noise with +-0, infinities, NaNs, denormals and values at the clip strewn over it) plus stars well above
    the clip and blotted squares"""
    f = special_frames(shape, seed, n=N_FRAMES).copy()
    h, w = shape
    rng = np.random.default_rng(seed + 1000)
    for k in range(N_FRAMES):
        for _ in range(max(1, h * w // 4000)):                          # (a stamp of 13 x 13: the pixels around keep their bits)
            cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
            ya, yb, xa, xb = max(0, cy - 6), min(h, cy + 7), max(0, cx - 6), min(w, cx + 7)
            yy, xx = np.mgrid[ya:yb, xa:xb]
            stamp = (0.6 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 4.5)).astype(np.float32)
            ok = np.isfinite(f[k, ya:yb, xa:xb]) & (stamp > 1e-3)
            f[k, ya:yb, xa:xb][ok] += stamp[ok]
        for _ in range(max(1, h * w // 8000)):
            cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
            f[k, max(0, cy - 3):cy + 4, max(0, cx - 3):cx + 4] = np.float32(0.0)
    return f


@functools.lru_cache(maxsize=None)
def case_inputs(shape):
    segs = hand_made(shape) + random_segments(shape, 1, 12, 100 + shape[0]) + random_segments(shape, 0, 4, 200 + shape[1])
    segs += random_segments(shape, 3, 300, 300 + shape[0], short=shape[0] > 100)
    segs += [UR.segment(4, 1.0, 1.0, 1.0, 1.0), UR.segment(4, np.inf, 1.0, 2.0, 1.0)]
    segs = np.array(segs, UR.SEGMENT_DTYPE)
    segs = segs[np.random.default_rng(7).permutation(len(segs))]        # frames interleaved: the library sorts them
    frames = sky_frames(shape, 5)
    for a in (segs, frames):
        a.setflags(write=False)
    return segs, frames


@functools.lru_cache(maxsize=None)
def case(shape):
    """(segments, frames, the restatement's cleaned frames, records and tables) of a shape: computed once, shared, read-only"""
    segs, frames = case_inputs(shape)
    clean, rec, tab = UR.subtract_trails(frames, segs, max_sections=MAX_SEC, max_cells=MAX_CELLS, **PARAMS)
    for a in (clean, rec, tab):
        a.setflags(write=False)
    return segs, frames, clean, rec, tab


def same_bits(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize == 4, what
    a, b = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} differ, first at {i}: device {got[i]!r}, restatement {want[i]!r}")


def outside_every_band(shape, segs, params, n=N_FRAMES, max_sections=MAX_SEC, max_cells=MAX_CELLS):
    """bool [n, h, w]: pixels whose centre lies in no good segment's band"""
    out = np.ones((n, *shape), bool)
    p = dict(UR.DEFAULTS, **params)
    for s in segs:
        status, g = UR.SR.geometry(s, p, max_sections, max_cells)
        if status == UR.OK:
            out[int(s["frame"])] &= ~UR.value(shape, g, np.zeros((g[-3], g[-2]), np.float32))[0]
    return out


def check(what, got, want):
    """(frames, records, tables) of the device against the restatement's"""
    same_bits(what + " frames", got[0], want[0])
    assert_same(what + " records", got[1], want[1])
    same_bits(what + " model", got[2], want[2])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_frames_records_and_model_equal_the_restatement(gpu_ctx, shape):
    import torch
    segs, frames, clean, want, tab = case(shape)
    kw = dict(max_sections=MAX_SEC, max_cells=MAX_CELLS, **PARAMS)
    host = frames.copy()
    rec, model = gpu_ctx.subtract_trails(host, segs, want_model=True, **kw)
    assert rec.dtype == UR.SUB_DTYPE and model.shape == (len(segs), MAX_CELLS) and model.dtype == np.float32
    check("host", (host, rec, model), (clean, want, tab))
    out = outside_every_band(shape, segs, PARAMS)
    assert np.array_equal(host.view(np.uint32)[out], frames.view(np.uint32)[out])
    got = set(want["status"].tolist())
    assert {UR.BAD_SEGMENT, UR.TOO_LONG, UR.EMPTY} <= got and int((want["status"] == UR.TOO_LONG).sum()) == 3
    on4 = segs["frame"] == 4
    assert (rec["status"][on4] == UR.BAD_SEGMENT).all() and not model[on4].any()
    # no good segment: the values are what they were (that such a frame is neither uploaded nor copied back is read from
    # sub.hip's chunk loop, which only walks the frames that carry one; identical bits cannot tell a copy back from none)
    assert np.array_equal(host[[2, 4]].view(np.uint32), frames[[2, 4]].view(np.uint32))
    if shape[0] > 30:
        assert UR.OK in got and int(want["n_sec"].max()) == MAX_SEC and int((want["n_sec"] * want["n_off"]).max()) == MAX_CELLS
        assert int(want["n_off"].max()) == 121 and int(want["n_pix"].max()) > 100 and (host != frames).any()
        with np.errstate(invalid="ignore"):
            inband = ~out
            assert (np.signbit(frames) & (frames == 0) & inband).any() and (np.isnan(frames) & inband).any()
            assert ((np.abs(frames) > 0.125) & np.isfinite(frames) & inband & (host != frames)).any()   # the light under a star goes too
    # the device, in place, without the tables
    dev = torch.from_numpy(frames.copy()).cuda()
    rec, none = gpu_ctx.subtract_trails(dev, segs, **kw)
    assert none is None
    got = dev.cpu().numpy()
    same_bits("device frames", got, clean)
    assert np.array_equal(got.view(np.uint32)[out], frames.view(np.uint32)[out])
    assert_same("device records", rec, want)
    # apply = 0 leaves every byte alone, native and big-endian, and returns the same records and tables
    for fr in (frames.copy(), frames.astype(">f4")):
        before = fr.tobytes()
        rec, model = gpu_ctx.subtract_trails(fr, segs, want_model=True, apply=0, **kw)
        assert fr.tobytes() == before
        assert_same("apply = 0 records", rec, want)
        same_bits("apply = 0 model", model, tab)
    dev = torch.from_numpy(frames.copy()).cuda()
    assert_same("apply = 0 on the device", gpu_ctx.subtract_trails(dev, segs, apply=0, **kw)[0], want)
    same_bits("apply = 0 device frames", dev.cpu().numpy(), frames)
    # with a mask plane
    m = plane(shape, 11)
    wm = UR.subtract_trails(frames, segs, mask=m, skip_bits=0x05, **kw)
    host = frames.copy()
    rec, model = gpu_ctx.subtract_trails(host, segs, mask=m, skip_bits=0x05, want_model=True, **kw)
    check("masked", (host, rec, model), wm)


ENDS = [dict(smooth=0, min_sec=1, step=0.5, sec_len=4.0, wing=1.0, min_n=1, min_wing=1),
        dict(smooth=2, min_sec=5, step=1.0, sec_len=32.0, wing=2.0, min_n=1, min_wing=1),
        dict(smooth=8, min_sec=17, step=8.0, sec_len=4.0, wing=8.0, min_n=1, min_wing=1),
        dict(smooth=8, min_sec=1, step=1.0, sec_len=4.0, wing=1.5, min_n=3, min_wing=4, clip=0.05),
        dict(smooth=2, min_sec=1, step=1.0, sec_len=32.0, wing=100.0)]


@pytest.mark.parametrize("params", ENDS, ids=["R0-step0.5-sec4", "R2-min5-sec32", "R8-min17-step8", "R8-min1-clip", "wing-over-half"])
def test_parameters_in_every_location(gpu_ctx, params):
    import torch
    shape = (37, 130)
    segs0, frames = case_inputs(shape)
    extra = [UR.segment(0, 2.0, 5.0, 127.0, 31.0, half=0.5), UR.segment(1, 0.0, 35.0, 129.0, 3.0, half=32.0),
             UR.segment(1, 5.0, 5.0, 139.0, 30.0, half=64.0), UR.segment(3, 0.0, 18.0, 129.0, 18.0, half=16.0),
             UR.segment(3, 65.0, 0.0, 65.0, 36.0, half=16.0)]
    segs = np.concatenate([segs0[::3], np.array(extra, UR.SEGMENT_DTYPE)])
    ms = 512 if params["sec_len"] < 8.0 else MAX_SEC
    m = plane(shape, 12)
    for mask, skip in ((None, 0), (m, 0x10)):
        kw = dict(skip_bits=skip, max_sections=ms, **params)
        want = UR.subtract_trails(frames, segs, mask=mask, **kw)
        mc = want[2].shape[1]
        host = frames.copy()
        rec, model = gpu_ctx.subtract_trails(host, segs, mask=mask, want_model=True, **kw)      # (max_cells: what the binding works out)
        check("host", (host, rec, model), want)
        dev = torch.from_numpy(frames.copy()).cuda()
        dmask = None if mask is None else torch.from_numpy(mask).cuda()
        rec, model = gpu_ctx.subtract_trails(dev, segs, mask=dmask, max_cells=mc, want_model=True, **kw)
        check("device", (dev.cpu().numpy(), rec, model), want)
        fb, mb = gpu_ctx.pinned_buffer(frames.nbytes), gpu_ctx.pinned_buffer(m.nbytes)
        pf = fb.array.view(np.float32)[:frames.size].reshape(frames.shape)
        pm = mb.array.view(np.uint8)[:m.size].reshape(m.shape)
        pf[...] = frames
        pm[...] = m
        rec, model = gpu_ctx.subtract_trails(pf, segs, mask=None if mask is None else pm, pinned=True, want_model=True, **kw)
        check("pinned", (pf, rec, model), want)
        del pf, pm
        fb.close()
        mb.close()
    rec = want[1]
    good = np.isin(rec["status"], (UR.OK, UR.EMPTY))
    if params["wing"] == 100.0:                                          # every bin is a wing bin: no model, nothing written
        assert (rec["status"][good] == UR.EMPTY).all() and not rec["n_pix"].any() and not want[2].any()
        same_bits("nothing written", want[0], frames)
    else:
        assert (rec["status"] == UR.OK).sum() >= 2 and int(rec["n_pix"].sum()) > 0
    # a single 2-d frame; no segments at all
    one = np.array([UR.segment(0, 2.0, 5.0, 120.0, 20.0, half=9.0)], UR.SEGMENT_DTYPE)
    f2 = frames[1].copy()
    rec, model = gpu_ctx.subtract_trails(f2, one, max_sections=64, want_model=True, **params)
    check("2-d", (f2, rec, model), UR.subtract_trails(frames[1], one, max_sections=64, **params))
    rec, model = gpu_ctx.subtract_trails(frames.copy(), np.zeros(0, UR.SEGMENT_DTYPE), max_sections=4, want_model=True)
    assert rec.shape == (0,) and model.shape == (0, 1)


def test_crossings_and_a_misaligned_device_buffer(gpu_ctx):
    """two and three segments that cross inside one tile, in both orders (the order is the index order, and it shows), and
    device frames that start 4 bytes off a 16-byte boundary (the four 4-byte loads and stores are taken)"""
    import torch
    shape = (40, 192)
    rng = np.random.default_rng(31)
    frames = rng.normal(0.0, 0.025, (2, *shape)).astype(np.float32)
    a, b, c = UR.segment(0, 2.0, 4.0, 60.0, 14.0, half=5.0), UR.segment(0, 2.0, 14.0, 60.0, 4.0, half=5.0), UR.segment(0, 30.0, 0.0, 31.0, 15.0, half=4.0)
    d = UR.segment(1, 3.0, 4.0, 180.0, 33.0, half=6.0)
    kw = dict(max_sections=64, sec_len=8.0, wing=1.0, min_n=1, min_wing=1, smooth=1, min_sec=1)
    cleans = []
    for order in ([a, b, c, d], [c, b, a, d], [b, a, d]):
        segs = np.array(order, UR.SEGMENT_DTYPE)
        want = UR.subtract_trails(frames, segs, **kw)
        host = frames.copy()
        rec, model = gpu_ctx.subtract_trails(host, segs, want_model=True, **kw)
        check("crossing", (host, rec, model), want)
        cleans.append(want[0])
        buf = torch.zeros(frames.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(frames.reshape(-1)).cuda()
        off = buf[1:].view(2, *shape)
        assert off.data_ptr() % 16 == 4
        rec, model = gpu_ctx.subtract_trails(off, segs, want_model=True, **kw)
        check("misaligned", (off.cpu().numpy(), rec, model), want)
        assert float(buf[0]) == 0.0
    assert not np.array_equal(cleans[0].view(np.uint32), cleans[1].view(np.uint32))     # float32 subtraction does not commute bit for bit


def test_refusals_touch_nothing_and_name_the_call(gpu_ctx):
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (24, 70)
    n = 2
    frames = special_frames(shape, 10)[:n].copy()
    keep = frames.tobytes()
    good = np.array([UR.segment(1, 0.0, 5.0, 69.0, 9.0, half=4.0)], UR.SEGMENT_DTYPE)
    lib = _native.lib()

    def P(sec_len=32.0, step=1.0, wing=6.0, clip=0.125, smooth=2, min_sec=3, min_n=8, min_wing=8, apply=1):
        return _native.SubParamsStruct(sec_len, step, wing, clip, smooth, min_sec, min_n, min_wing, apply)

    def refused(prefix="lfdmi_subtract_trails", segs=good, n_seg=None, fr=frames, dtype=_native.F32, nn=n, h=shape[0], w=shape[1], loc=_native.HOST,
                p=P(), sigma=None, ms=8, mc=128, skip=0, null=()):
        out = np.full(len(segs), -7, np.int8).repeat(UR.SUB_DTYPE.itemsize).view(UR.SUB_DTYPE)
        mod = np.full(len(segs) * 128 * 4, 0x5A, np.uint8)
        rc = lib.lfdmi_subtract_trails(gpu_ctx._h, _native._ptr(fr), dtype, nn, h, w, loc, None, skip, None if "segs" in null else _native._ptr(segs),
                                       len(segs) if n_seg is None else n_seg, _native._ptr(sigma), C.byref(p),
                                       None if "out" in null else _native._ptr(out), _native._ptr(mod), ms, mc)
        assert rc == _native.ERR_ARG
        assert lib.lfdmi_last_error(gpu_ctx._h).decode().startswith(prefix), lib.lfdmi_last_error(gpu_ctx._h).decode()
        assert (out.view(np.int8) == -7).all() and (mod == 0x5A).all() and frames.tobytes() == keep

    for f in (-1, n):
        bad = good.copy()
        bad["frame"] = f
        refused("lfdmi_subtract_trails: segment 0", bad)
    refused("lfdmi_subtract_trails takes", dtype=_native.U8)
    refused("lfdmi_subtract_trails takes", dtype=_native.F64)
    refused("lfdmi_subtract_trails changes", dtype=_native.F32_BE)       # big-endian frames with apply = 1
    refused("bad loc", loc=3)
    refused(nn=-1)
    refused(n_seg=-1)
    refused(h=0)
    refused(w=70000)
    refused(h=40000, w=40000)
    refused("lfdmi_subtract_trails: NULL", fr=None)
    for which in ("segs", "out"):
        refused("lfdmi_subtract_trails: NULL", null=(which,))
    refused("lfdmi_subtract_trails: max_sections_per_seg", ms=0)
    refused("lfdmi_subtract_trails: max_sections_per_seg", ms=_native.STRIP_MAX_SECTIONS + 1)
    refused("lfdmi_subtract_trails: max_cells_per_seg", mc=0)
    refused("lfdmi_subtract_trails: max_cells_per_seg", mc=_native.STRIP_MAX_SECTIONS * _native.STRIP_MAX_OFF + 1)
    refused("lfdmi_subtract_trails: skip_bits", skip=256)
    refused("lfdmi_subtract_trails: skip_bits", skip=-1)
    nan, inf = float("nan"), float("inf")
    for p in (P(sec_len=3.9), P(sec_len=4097.0), P(sec_len=nan), P(step=0.49), P(step=8.1), P(step=nan), P(wing=0.0), P(wing=-1.0), P(wing=inf),
              P(wing=nan), P(clip=0.0), P(clip=-1.0), P(clip=inf), P(clip=nan), P(clip=1025.0), P(smooth=-1), P(smooth=9), P(min_sec=0),
              P(min_sec=6), P(smooth=0), P(smooth=8, min_sec=18), P(min_n=0), P(min_wing=0), P(apply=2), P(apply=-1)):
        refused("lfdmi_subtract_trails: params", p=p)
    for s in ([0.025, 0.0], [0.025, -1.0], [np.nan, 0.025], [np.inf, 0.025]):
        refused("lfdmi_subtract_trails: sigma", sigma=np.array(s, np.float32))
    # through the binding: the same code as an exception; the Python-side checks
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.subtract_trails(frames, good, sec_len=3.0)
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(_native.NativeError):
        gpu_ctx.subtract_trails(frames.astype(">f4"), good)
    with pytest.raises(TypeError):
        gpu_ctx.subtract_trails(frames, good, section=4.0)
    ro = frames.copy()
    ro.setflags(write=False)
    with pytest.raises(ValueError):
        gpu_ctx.subtract_trails(ro, good)
    with pytest.raises(ValueError):
        gpu_ctx.subtract_trails(frames, good, mask=np.zeros((n, shape[0], shape[1] + 1), np.uint8))
    with pytest.raises(TypeError):
        gpu_ctx.subtract_trails(frames, good, mask=np.zeros((n, *shape), np.int8))
    with pytest.raises(ValueError):
        gpu_ctx.subtract_trails(frames, good, mask=torch.zeros((n, *shape), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.subtract_trails(frames, good, max_cells=0)
    assert frames.tobytes() == keep
    # while a detect_batch_begin is in flight
    pb, pd, _ = default_params()
    dev = torch.from_numpy(np.random.default_rng(6).normal(0, 0.025, (2, 384, 640)).astype(np.float32)).cuda()
    kw = dict(max_sections=16, sec_len=8.0, min_n=2, min_wing=2, wing=1.0)
    want = UR.subtract_trails(frames, good, **kw)
    with _native.Context(0, 384, 640, 2) as c2:
        pend = c2.detect_batch_begin(dev, pb, pd)
        with pytest.raises(_native.NativeError):
            c2.subtract_trails(frames, good)
        pend.result()
        assert frames.tobytes() == keep
        f2 = frames.copy()
        rec, model = c2.subtract_trails(f2, good, want_model=True, **kw)
        check("after the flight", (f2, rec, model), want)
    # and the session's context still works after every refusal
    f2 = frames.copy()
    rec, model = gpu_ctx.subtract_trails(f2, good, want_model=True, **kw)
    check("after the refusals", (f2, rec, model), want)
    assert want[1]["status"][0] == UR.OK


def star_frame():
    """frame 0 of the faint-trail search's noise set with sixty synth stars (sigma 1.2 px, peaks 0.2 .. 2) strewn over it"""
    import test_radon_model as TM
    from lfd_amd import synth
    f = TM.noise_frames()[0].copy()
    rng = np.random.default_rng(77)
    h, w = f.shape
    synth._add_stars(f, rng.uniform(0, h, 60), rng.uniform(0, w, 60), rng.uniform(0.2, 2.0, 60) * 2 * np.pi * 1.2 ** 2, 1.2)
    return f


def test_a_found_trail_taken_out(gpu_ctx):
    """inject a peak-0.02 trail over synth stars -> search_lines finds it -> masks.segments_from_radon_lines ->
    subtract.segments_from_mask_segments -> subtract_trails -> the second search_lines has no line there, and the star pixels
    under the band equal the restatement's cleaned frame (bit parity, no tolerance)"""
    import torch
    import test_radon_model as TM
    from lfd_amd import _native, masks, subtract
    tr0, table, step = TM.trail_plan()
    base = star_frame()
    frames = torch.from_numpy(base[None].copy()).cuda()
    gpu_ctx.inject_trails(frames, tr0[:1], table, step)
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=1, bin=2) as r:
        lines, nl = r.search_lines(frames, sigma=TM.SET_SIGMA, max_lines=1, peel_halfwidth=8, min_seg=64)
        assert int(nl[0]) == 1
        msegs, where = masks.segments_from_radon_lines(lines, nl)
        segs = subtract.segments_from_mask_segments(msegs)
        assert len(segs) == 1 and segs[0]["half"] == msegs[0]["half"] + 6.0
        before = frames.cpu().numpy()
        rec, maps = subtract.subtract_trails(gpu_ctx, frames, segs)
        clean, want, tab = UR.subtract_trails(before, segs)
        after = frames.cpu().numpy()
        same_bits("cleaned frame", after, clean)
        assert_same("records", rec, want)
        assert rec[0]["status"] == UR.OK and rec[0]["n_pix"] > 5000 and float(rec[0]["removed"]) > 0.0
        assert maps[0].shape == (int(rec[0]["n_sec"]), int(rec[0]["n_off"]))
        stars = (before[0] > 0.125) & ~outside_every_band(TM.SET_SHAPE, segs, {}, n=1)[0]
        assert int(stars.sum()) > 20 and np.array_equal(after[0][stars].view(np.uint32), clean[0][stars].view(np.uint32))
        assert (after[0][stars] != 0).all()                                # they stand, where a zero fill leaves a hole
        lines2, nl2 = r.search_lines(frames, sigma=TM.SET_SIGMA, max_lines=1, peel_halfwidth=8, min_seg=64)
    th, rho = float(lines[0, 0]["theta"]), float(lines[0, 0]["rho"])
    for k in range(int(nl2[0])):
        dth = abs(float(lines2[0, k]["theta"]) - th)
        assert not (min(dth, math.pi - dth) <= math.radians(1.0) and abs(float(lines2[0, k]["rho"]) - rho) <= 2.0), lines2[0, k]
