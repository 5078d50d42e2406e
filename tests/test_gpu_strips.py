"""Trail strips on the device against the numpy restatement of include/lfdmi.h (tests/strip_ref.py): every integer of every cell,
every bit of every double of the section and segment records and the float means, over the shapes at which the 64 x 16 tiling can
go wrong, every kind of segment and pixel, the parameters' ends, every buffer location, with and without a mask plane; the identity
with the light curves on the device; the refusals; and the composition with the injection, the faint-trail search and the trail
masks' segment builders."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402
import strip_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

# 1 x 1; one side of each tile edge (tiles are 64 wide, 16 high); w % 4 != 0 with partial tiles on both axes; a crop of eight
# tile columns by 24 tile rows
SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (37, 130), (372, 512)]
N_FRAMES = 5          # frame 2 carries no segment, frame 3 three hundred (more than two LDS chunks of 128), frame 4 only bad ones
MAX_SEC = 256
MAX_CELLS = 256 * 29  # 256 sections of a half-14 band at step 1
PARAMS = dict(sec_len=8.0, wing=1.0, min_core=2, min_wing=2, k_mom=1.0)


def hand_made(shape):
    """segments of frame 0: every direction, reach and band the definition distinguishes"""
    h, w = shape
    m = min(h, w)
    S = SR.segment
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
        S(0, 1.0, h // 3, 17.0, h // 3, half=2.0),                                        # t == L on the centre of pixel 17: the last section
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
        if rng.random() < 0.3:                                         # integer end points: centres on the band's and the bins' edges
            x1, y1, x2, y2 = (float(round(v)) for v in (x1, y1, x2, y2))
            if (x1, y1) == (x2, y2):
                x2 += 1.0
        out.append(SR.segment(frame, x1, y1, x2, y2, half=float(rng.choice([0.5, 1.0, 2.5, 3.25, 0.7071067811865476, 8.0, 14.0]))))
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
    return f


def plane(shape, seed, n=N_FRAMES):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, *shape)) * (rng.random((n, *shape)) < 0.3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_inputs(shape):
    segs = hand_made(shape) + random_segments(shape, 1, 12, 100 + shape[0]) + random_segments(shape, 0, 4, 200 + shape[1])
    segs += random_segments(shape, 3, 300, 300 + shape[0], short=shape[0] > 100)
    segs += [SR.segment(4, 1.0, 1.0, 1.0, 1.0), SR.segment(4, np.inf, 1.0, 2.0, 1.0)]
    segs = np.array(segs, SR.SEGMENT_DTYPE)
    segs = segs[np.random.default_rng(7).permutation(len(segs))]        # frames interleaved: the library sorts them
    frames = special_frames(shape, 5)
    for a in (segs, frames):
        a.setflags(write=False)
    return segs, frames


@functools.lru_cache(maxsize=None)
def case(shape):
    """(segments, frames, restatement's records, sections and cells) of a shape: computed once, shared, read-only"""
    segs, frames = case_inputs(shape)
    rec, sec, cel = SR.trail_strips(frames, segs, max_sections=MAX_SEC, max_cells=MAX_CELLS, **PARAMS)
    for a in (rec, sec, cel):
        a.setflags(write=False)
    return segs, frames, rec, sec, cel


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


def assert_all(what, got, want):
    assert_same(what + " cells", got[2], want[2])
    assert_same(what + " sections", got[1], want[1])
    assert_same(what + " records", got[0], want[0])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_cells_sections_and_records_equal_the_restatement(gpu_ctx, shape):
    from lfd_amd import strips
    segs, frames, want, want_sec, want_cel = case(shape)
    kw = dict(max_sections=MAX_SEC, max_cells=MAX_CELLS, **PARAMS)
    rec, sec, cel = gpu_ctx.trail_strips(frames, segs, **kw)
    assert rec.dtype == SR.STRIP_DTYPE and sec.shape == (len(segs), MAX_SEC) and cel.shape == (len(segs), MAX_CELLS)
    assert_all("host", (rec, sec, cel), (want, want_sec, want_cel))
    got = set(want["status"].tolist())
    assert {SR.BAD_SEGMENT, SR.TOO_LONG, SR.EMPTY} <= got and int((want["status"] == SR.TOO_LONG).sum()) == 3
    on4 = segs["frame"] == 4
    assert (rec["status"][on4] == SR.BAD_SEGMENT).all() and not sec[on4].view(np.uint8).any() and not cel[on4].view(np.uint8).any()
    if shape[0] > 30:
        assert SR.OK in got and {SR.SEC_OK, SR.SEC_LOW, SR.SEC_EMPTY} <= set(want_sec["status"][want["status"] == SR.OK].reshape(-1).tolist())
        assert int(want["n_sec"].max()) == MAX_SEC and int((want["n_sec"] * want["n_off"]).max()) == MAX_CELLS
        assert int(want["n_mom"].max()) > 0 and int(want["n_off"].max()) == 121 and int(want["n_off"].min()) == 0
    # the float means of the one-call helper, bit for bit
    r2, s2, maps = strips.trail_strips(gpu_ctx, frames, segs, **kw)
    for i in range(len(segs)):
        ns, no = (int(want[i]["n_sec"]), int(want[i]["n_off"])) if want[i]["status"] in (SR.OK, SR.EMPTY) else (0, 0)
        assert maps[i]["mean"].shape == (ns, no) and maps[i]["mean"].dtype == np.float32
        assert np.array_equal(maps[i]["mean"].view(np.uint32), SR.mean_map(want_cel[i][:ns * no]).reshape(ns, no).view(np.uint32))
        assert np.array_equal(maps[i]["n"], want_cel[i][:ns * no]["n"].reshape(ns, no))
    # the same frames big-endian, and with a mask plane
    assert_all("big-endian", gpu_ctx.trail_strips(frames.astype(">f4"), segs, **kw), (want, want_sec, want_cel))
    m = plane(shape, 11)
    wm = SR.trail_strips(frames, segs, mask=m, skip_bits=0x05, **kw)
    assert_all("masked", gpu_ctx.trail_strips(frames, segs, mask=m, skip_bits=0x05, **kw), wm)
    if shape[0] > 30:
        assert int(wm[2]["n"].sum()) < int(want_cel["n"].sum()) and np.array_equal(wm[2]["n_geom"], want_cel["n_geom"])


def ends_segments(shape):
    """the ends of the band: half 0.5 (K = 0 at step 1), 32 (129 bins at step 0.5), 64 (129 bins at step 1) and past MAX_OFF"""
    h, w = shape
    S = SR.segment
    return [S(0, 2.0, 5.0, w - 3.0, h - 6.0, half=0.5), S(1, 0.0, h - 2.0, w - 1.0, 3.0, half=32.0), S(1, 5.0, 5.0, w + 9.0, 30.0, half=64.0),
            S(0, 5.0, 5.0, w + 9.0, 30.0, half=64.25), S(1, w / 2.0, -3.0, w / 2.0 + 1.0, h + 3.0, half=64.6),
            S(3, 0.0, h // 2, w - 1.0, h // 2, half=16.0), S(3, w // 2, 0.0, w // 2, h - 1.0, half=16.0)]


@pytest.mark.parametrize("params", [dict(sec_len=4.0, step=0.5, wing=2.0, min_core=1, min_wing=1, k_mom=0.5), dict(sec_len=4096.0, step=8.0),
                                    {}, dict(sec_len=8.5, step=1.0, clip=0.05, min_core=40, min_wing=2, wing=3.0, k_mom=0.0)],
                         ids=["sec4-step0.5", "sec4096-step8", "defaults", "clip"])
def test_parameters_in_every_location(gpu_ctx, params):
    import torch
    shape = (37, 130)
    segs0, frames = case_inputs(shape)
    # (at sec_len 4 the long rows would need 500 sections: the short ones and the ends of the band are enough there)
    segs = np.concatenate([segs0[::3], np.array(ends_segments(shape), SR.SEGMENT_DTYPE)])
    ms = 512 if params.get("sec_len", 8.0) < 8.0 else MAX_SEC
    sigma = np.linspace(0.02, 0.05, N_FRAMES).astype(np.float32)
    m = plane(shape, 12)
    for mask, skip in ((None, 0), (m, 0xFF), (m, 0x10), (m, 0)):
        kw = dict(skip_bits=skip, sigma=sigma, max_sections=ms, **params)
        want = SR.trail_strips(frames, segs, mask=mask, **kw)
        mc = want[2].shape[1]
        assert_all("host", gpu_ctx.trail_strips(frames, segs, mask=mask, **kw), want)          # (max_cells: what the binding works out)
        # device: the frames and the plane are used where they are
        dev = torch.from_numpy(frames.copy()).cuda()
        dmask = None if mask is None else torch.from_numpy(mask).cuda()
        assert_all("device", gpu_ctx.trail_strips(dev, segs, mask=dmask, max_cells=mc, **kw), want)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), frames.view(np.uint32))     # frames are only read
        # pinned, big-endian
        fb, mb = gpu_ctx.pinned_buffer(frames.nbytes), gpu_ctx.pinned_buffer(m.nbytes)
        pf = fb.array.view(">f4")[:frames.size].reshape(frames.shape)
        pm = mb.array.view(np.uint8)[:m.size].reshape(m.shape)
        pf[...] = frames
        pm[...] = m
        assert_all("pinned", gpu_ctx.trail_strips(pf, segs, mask=None if mask is None else pm, pinned=True, **kw), want)
        del pf, pm
        fb.close()
        mb.close()
    rec = want[0]
    step = params.get("step", 1.0)
    ends = rec[-7:]
    assert ends[0]["K"] == (0 if step >= 1.0 else 1) and (ends[4]["status"] == SR.BAD_SEGMENT) == (step <= 1.0)   # (17 bins at step 8)
    if step == 0.5:
        assert ends[1]["n_off"] == 129 and ends[2]["status"] == SR.BAD_SEGMENT and int(rec["n_sec"].max()) > 32
    if step == 1.0:
        assert ends[2]["n_off"] == 129 and ends[3]["n_off"] == 129
    if params.get("sec_len") == 4096.0:
        assert int(rec["n_sec"].max()) == 1 and ends[2]["n_off"] == 17
    # a single 2-d frame; a scalar sigma; no segments at all
    one = np.array([SR.segment(0, 2.0, 5.0, 120.0, 20.0, half=9.0)], SR.SEGMENT_DTYPE)
    assert_all("2-d", gpu_ctx.trail_strips(frames[1], one, sigma=0.03, max_sections=64, **params),
               SR.trail_strips(frames[1], one, sigma=0.03, max_sections=64, **params))
    rec, sec, cel = gpu_ctx.trail_strips(frames, np.zeros(0, SR.SEGMENT_DTYPE), max_sections=4)
    assert rec.shape == (0,) and sec.shape == (0, 4) and cel.shape == (0, 1)


def test_the_fixed_point_range_and_a_misaligned_device_buffer(gpu_ctx):
    """values of +-1024 at clip 1024 across whole cells (|q| = 2^40, the largest), and device frames that start 4 bytes off a
    16-byte boundary (the four 4-byte loads are taken)"""
    import torch
    shape = (40, 192)
    frames = np.full((2, *shape), 1024.0, np.float32)
    frames[0, :, 96:] = -1024.0
    with np.errstate(invalid="ignore"):                                  # (the signalling NaNs among the special pixels)
        frames[1] = special_frames(shape, 21, n=1, clip=1024.0)[0] * np.float32(4000.0)
    frames[1, 10:14, 20:60] = np.float32(1024.0)
    frames[1, 14:16, 20:60] = np.nextafter(np.float32(1024.0), np.float32(np.inf))
    segs = np.array([SR.segment(0, 0.0, 20.0, 191.0, 20.0, half=8.0), SR.segment(1, 3.0, 4.0, 180.0, 33.0, half=6.0),
                     SR.segment(0, 5.0, 35.0, 150.0, 2.0, half=3.0)], SR.SEGMENT_DTYPE)
    kw = dict(max_sections=16, sec_len=64.0, clip=1024.0, wing=2.0, min_core=4, min_wing=4)
    want = SR.trail_strips(frames, segs, **kw)
    c0 = want[2][0][:17]
    assert (c0["q"] == c0["n"].astype(np.int64) << 40).all() and int(c0["n"].sum()) > 0
    assert_all("host", gpu_ctx.trail_strips(frames, segs, **kw), want)
    buf = torch.zeros(frames.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(frames.reshape(-1)).cuda()
    off = buf[1:].view(2, *shape)
    assert off.data_ptr() % 16 == 4
    mbuf = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    assert_all("misaligned", gpu_ctx.trail_strips(off, segs, mask=mbuf[1:].view(2, *shape), skip_bits=0xFF, **kw), want)


@pytest.mark.parametrize("shape", [(37, 130), (372, 512)], ids=["37x130", "372x512"])
def test_summed_over_offsets_a_strip_is_a_light_curve_on_the_device(gpu_ctx, shape):
    """two units against each other: ``trail_strips`` cells summed over b are ``light_curves``' n_geom, n_core and q_core at sec_len 8"""
    segs, frames = case_inputs(shape)
    m = plane(shape, 13)
    lsegs = np.zeros(len(segs), LR.SEGMENT_DTYPE)
    for k in ("frame", "x1", "y1", "x2", "y2", "half"):
        lsegs[k] = segs[k]
    lsegs["bg_in"], lsegs["bg_out"] = segs["half"] + 1.0, segs["half"] + 3.0
    for kw in ({}, dict(mask=m, skip_bits=0x22)):
        rec, sec, cel = gpu_ctx.trail_strips(frames, segs, max_sections=MAX_SEC, max_cells=MAX_CELLS, sec_len=8.0, **kw)
        lrec, lsec = gpu_ctx.light_curves(frames, lsegs, max_sections=MAX_SEC, sec_len=8.0, **kw)
        checked = 0
        for i in range(len(segs)):
            if rec[i]["status"] not in (SR.OK, SR.EMPTY):
                continue
            assert lrec[i]["status"] in (LR.OK, LR.EMPTY) and lrec[i]["n_sec"] == rec[i]["n_sec"], i
            ns, no = int(rec[i]["n_sec"]), int(rec[i]["n_off"])
            c = cel[i][:ns * no].reshape(ns, no)
            assert np.array_equal(c["n_geom"].sum(1), lsec[i, :ns]["n_geom"]), i
            assert np.array_equal(c["n"].sum(1), lsec[i, :ns]["n_core"]), i
            assert np.array_equal(c["q"].sum(1), lsec[i, :ns]["q_core"]), i
            checked += int(c["n_geom"].sum() > 0)
        assert checked > 20


def test_refusals_touch_nothing_and_name_the_call(gpu_ctx):
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (24, 70)
    n = 2
    frames = special_frames(shape, 10)[:n].copy()
    good = np.array([SR.segment(1, 0.0, 5.0, 69.0, 9.0, half=4.0)], SR.SEGMENT_DTYPE)
    lib = _native.lib()

    def P(sec_len=8.0, step=1.0, wing=6.0, k_mom=5.0, clip=0.125, min_core=8, min_wing=8):
        return _native.StripParamsStruct(sec_len, step, wing, k_mom, clip, min_core, min_wing, 0)

    def refused(prefix="lfdmi_trail_strips", segs=good, n_seg=None, fr=frames, dtype=_native.F32, nn=n, h=shape[0], w=shape[1], loc=_native.HOST,
                p=P(), sigma=None, ms=8, mc=128, skip=0, null=()):
        out = np.full(len(segs), -7, np.int8).repeat(SR.STRIP_DTYPE.itemsize).view(SR.STRIP_DTYPE)
        sec = np.full(len(segs) * 8 * SR.SECTION_DTYPE.itemsize, 0xA5, np.uint8)
        cel = np.full(len(segs) * 128 * SR.CELL_DTYPE.itemsize, 0x5A, np.uint8)
        rc = lib.lfdmi_trail_strips(gpu_ctx._h, _native._ptr(fr), dtype, nn, h, w, loc, None, skip, None if "segs" in null else _native._ptr(segs),
                                    len(segs) if n_seg is None else n_seg, _native._ptr(sigma), C.byref(p),
                                    None if "out" in null else _native._ptr(out), None if "sec" in null else _native._ptr(sec), ms,
                                    None if "cells" in null else _native._ptr(cel), mc)
        assert rc == _native.ERR_ARG
        assert lib.lfdmi_last_error(gpu_ctx._h).decode().startswith(prefix), lib.lfdmi_last_error(gpu_ctx._h).decode()
        assert (out.view(np.int8) == -7).all() and (sec == 0xA5).all() and (cel == 0x5A).all()

    for f in (-1, n):
        bad = good.copy()
        bad["frame"] = f
        refused("lfdmi_trail_strips: segment 0", bad)
    refused("lfdmi_trail_strips takes", dtype=_native.U8)
    refused("lfdmi_trail_strips takes", dtype=_native.F64)
    refused("bad loc", loc=3)
    refused(nn=-1)
    refused(n_seg=-1)
    refused(h=0)
    refused(w=70000)
    refused(h=40000, w=40000)
    refused("lfdmi_trail_strips: NULL", fr=None)
    for which in ("segs", "out", "sec", "cells"):
        refused("lfdmi_trail_strips: NULL", null=(which,))
    refused("lfdmi_trail_strips: max_sections_per_seg", ms=0)
    refused("lfdmi_trail_strips: max_sections_per_seg", ms=_native.STRIP_MAX_SECTIONS + 1)
    refused("lfdmi_trail_strips: max_cells_per_seg", mc=0)
    refused("lfdmi_trail_strips: max_cells_per_seg", mc=_native.STRIP_MAX_SECTIONS * _native.STRIP_MAX_OFF + 1)
    refused("lfdmi_trail_strips: skip_bits", skip=256)
    refused("lfdmi_trail_strips: skip_bits", skip=-1)
    nan, inf = float("nan"), float("inf")
    for p in (P(sec_len=3.9), P(sec_len=4097.0), P(sec_len=nan), P(step=0.49), P(step=8.1), P(step=nan), P(wing=0.0), P(wing=-1.0), P(wing=inf),
              P(wing=nan), P(k_mom=-0.5), P(k_mom=nan), P(k_mom=inf), P(clip=0.0), P(clip=-1.0), P(clip=inf), P(clip=nan), P(clip=1025.0),
              P(min_core=0), P(min_wing=0)):
        refused("lfdmi_trail_strips: params", p=p)
    for s in ([0.025, 0.0], [0.025, -1.0], [np.nan, 0.025], [np.inf, 0.025]):
        refused("lfdmi_trail_strips: sigma", sigma=np.array(s, np.float32))
    # through the binding: the same code as an exception; the Python-side checks
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.trail_strips(frames, good, sec_len=3.0)
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(TypeError):
        gpu_ctx.trail_strips(frames, good, section=4.0)
    with pytest.raises(ValueError):
        gpu_ctx.trail_strips(frames, good, mask=np.zeros((n, shape[0], shape[1] + 1), np.uint8))
    with pytest.raises(TypeError):
        gpu_ctx.trail_strips(frames, good, mask=np.zeros((n, *shape), np.int8))
    with pytest.raises(ValueError):
        gpu_ctx.trail_strips(frames, good, mask=torch.zeros((n, *shape), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.trail_strips(frames, good, max_cells=0)
    # while a detect_batch_begin is in flight
    pb, pd, _ = default_params()
    dev = torch.from_numpy(np.random.default_rng(6).normal(0, 0.025, (2, 384, 640)).astype(np.float32)).cuda()
    kw = dict(max_sections=16, min_core=4, min_wing=4, wing=1.0)
    want = SR.trail_strips(frames, good, **kw)
    with _native.Context(0, 384, 640, 2) as c2:
        pend = c2.detect_batch_begin(dev, pb, pd)
        with pytest.raises(_native.NativeError):
            c2.trail_strips(frames, good)
        pend.result()
        assert_all("after the flight", c2.trail_strips(frames, good, **kw), want)
    # and the session's context still works after every refusal
    assert_all("after the refusals", gpu_ctx.trail_strips(frames, good, **kw), want)
    assert want[0]["status"][0] == SR.OK


def test_a_found_trail_straightened(gpu_ctx):
    """inject a peak-0.02 trail -> search_lines finds the line -> masks.segments_from_radon_lines ->
    strips.segments_from_mask_segments -> trail_strips: the device's records equal the restatement's, the trail lies within 2 px
    of the strip's middle and its summed rate is positive"""
    import torch
    import test_radon_model as TM
    from lfd_amd import _native, masks, strips
    tr0, table, step = TM.trail_plan()
    frames = torch.from_numpy(TM.noise_frames()[:1].copy()).cuda()
    gpu_ctx.inject_trails(frames, tr0[:1], table, step)
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=1, bin=2) as r:
        lines, nl = r.search_lines(frames, sigma=TM.SET_SIGMA, max_lines=1, peel_halfwidth=8, min_seg=64)
    assert int(nl[0]) == 1
    msegs, where = masks.segments_from_radon_lines(lines, nl)
    segs = strips.segments_from_mask_segments(msegs)
    assert len(segs) == 1 and segs[0]["half"] == msegs[0]["half"] + 6.0 == 16.0
    kw = dict(sigma=TM.SET_SIGMA, sec_len=32.0, k_mom=3.0, max_sections=32)
    rec, sec, maps = strips.trail_strips(gpu_ctx, frames, segs, **kw)
    want = SR.trail_strips(frames.cpu().numpy(), segs, **kw)
    assert_same("sections", sec, want[1])
    assert_same("records", rec, want[0])
    assert rec[0]["status"] == SR.OK and rec[0]["n_ok"] >= 6 and rec[0]["n_mom"] >= 3
    assert abs(float(rec[0]["mean_centre"])) <= 2.0, rec[0]
    okj = sec[0]["status"][:int(rec[0]["n_sec"])] == SR.SEC_OK
    assert float(sec[0]["rate"][:int(rec[0]["n_sec"])][okj].sum()) > 0.0
    assert maps[0]["mean"].shape == (int(rec[0]["n_sec"]), 33)
