"""The frame seeing on the device against its restatement (tests/psf_ref.py), byte for byte: every packed record, status count
and frame record, on 4 frames of 96 x 160 -- native and big-endian, from host, page-locked and device memory, with the finder's
records on the host and on the device, at win = 1 and win = 16, and split into one frame per chunk -- and the argument checks
that sit behind the context."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as R  # noqa: E402
import stars_ref as S  # noqa: E402
from test_psf_abi import REFUSED, TAKEN  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (96, 160)
MAX_OBJ = 96
MAIN = {"max_used": 4, "min_stars": 3}                   # frame 0 has more OK stars than max_used
SETTINGS = {"main": MAIN, "defaults": {},
            "win1": {"win": 1, "gap": 0, "ring": 1, "iso": 3, "sat": 20.0, "min_stars": 2},
            "win16": {"win": 16, "gap": 8, "ring": 8, "iso": 1, "rad_max": 32, "min_stars": 1, "e_max": 1.0}}


def assert_same(got, want, what=""):
    (out, fr), (wout, wfr) = got, want
    assert out.dtype == R.STAR_DTYPE and fr.dtype == R.FRAME_DTYPE and out.shape == wout.shape and fr.shape == wfr.shape, what
    for i in range(len(wfr)):
        assert fr[i].tobytes() == wfr[i].tobytes(), (what, i, fr[i], wfr[i])
        for j in range(out.shape[1]):
            assert out[i, j].tobytes() == wout[i, j].tobytes(), (what, i, j, out[i, j], wout[i, j])


@functools.lru_cache(maxsize=None)
def case():
    """Frame 0: a star whose square just fits (x = 12) and one that leaves the frame by one pixel (x = 11), a pair at iso and a
    pair at iso + 1, three more: over max_used = 4 OK stars.  Frame 1: a streak and stars.  Frame 2: stars with a NaN, an inf,
    a +0, a -0 and a value beyond sat in their rings, and three clean ones.  Frame 3: faint noise, no record at all."""
    from lfd_amd import synth
    rng = np.random.default_rng(20240914)
    frames = rng.normal(0, 0.025, (4, *SHAPE)).astype(np.float32)
    frames[3] *= np.float32(0.25)

    def add(i, pts):
        xs, ys = np.array([p[0] for p in pts], float), np.array([p[1] for p in pts], float)
        synth._add_stars(frames[i], ys, xs, np.exp(rng.uniform(np.log(30.0), np.log(2000.0), len(pts))), 1.5)

    add(0, [(12, 40), (11, 70), (40, 30), (52, 30), (40, 60), (53, 60), (80, 20), (100, 50), (120, 75), (140, 30)])
    add(1, [(30, 70), (130, 20), (140, 70), (25, 25)])
    synth._add_streak(frames[1], 40.0, 80.0, 30.0, 1.0, 2.0)
    add(2, [(20, 20), (60, 20), (100, 20), (140, 20), (20, 60), (60, 60), (100, 60), (140, 60)])
    frames[2, 20, 31] = np.nan                                  # ring of (20, 20): dx = 11
    frames[2, 8, 60] = np.inf                                   # ring of (60, 20): dy = -12
    frames[2, 30, 90] = 0.0                                     # ring of (100, 20): the corner (-10, +10)
    frames[2, 32, 152] = -0.0                                   # ring of (140, 20): the corner (+12, +12)
    frames[2, 60, 30] = -5000.0                                 # ring of (20, 60): dx = 10
    rec, frec = S.find_stars_batch(frames, max_obj=MAX_OBJ)
    frames.setflags(write=False)
    return frames, rec, frec


@functools.lru_cache(maxsize=None)
def want(name):
    frames, rec, frec = case()
    out = R.measure_batch(frames, rec, frec, **SETTINGS[name])
    for a in out:
        a.setflags(write=False)
    return out


def statuses(name, i):
    frames, rec, frec = case()
    return R.measure_frame(frames[i], rec[i], frec[i]["n_out"], **SETTINGS[name])[2]


def test_the_case_holds_what_it_is_meant_to():
    frames, rec, frec = case()
    assert frec["n_out"][3] == 0 and frec["n_out"][:3].min() >= 8 and frec["n_found"].max() < MAX_OBJ
    wout, wfr = want("main")
    at = {(int(r["x"]), int(r["y"])): st for r, st in zip(rec[0], statuses("main", 0))}
    assert at[(12, 40)] == R.OK and at[(11, 70)] == R.CLIPPED
    assert at[(40, 30)] == at[(52, 30)] == R.CROWDED and at[(40, 60)] == at[(53, 60)] == R.OK
    assert wfr["n_ok"][0] > 4 and wfr["n_packed"][0] == 4 and wfr["status"][0] == R.SEEING_OK and wfr["n_used"][0] >= 3
    assert np.count_nonzero(rec[1]["flags"] & S.EXTENDED) >= 3 and wfr["n_not_candidate"][1] >= 3
    at = {(int(r["x"]), int(r["y"])): st for r, st in zip(rec[2], statuses("main", 2))}
    assert [at[(x, y)] for x, y in ((20, 20), (60, 20), (100, 20), (140, 20), (20, 60))] == [R.BAD_PIXEL] * 5
    assert [at[(x, y)] for x, y in ((60, 60), (100, 60), (140, 60))] == [R.OK] * 3
    assert wfr["n_bad_pixel"][2] == 5 and wfr["n_cand"][3] == 0 and wfr["status"][3] == R.SEEING_FEW and np.isnan(wfr["fwhm_px"][3])
    # the width of the frame's sigma 1.5 px stars, loosely: this is the model test's subject, here it guards the case
    assert 3.0 < wfr["fwhm_px"][0] < 4.2
    assert want("win1")[1]["n_bad_pixel"].sum() > 5 and want("win1")[1]["n_ok"].sum() >= 3      # sat = 20.0 refuses bright cores
    assert want("win16")[1]["n_ok"].sum() >= 3 and want("win16")[1]["n_clipped"].sum() >= 3
    assert want("defaults")[1]["n_packed"][0] == wfr["n_ok"][0]


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_host_frames_and_host_records(gpu_ctx, name):
    frames, rec, frec = case()
    assert_same(gpu_ctx.measure_seeing(frames, rec, frec, **SETTINGS[name]), want(name), name)


def test_one_frame_alone_and_sigmas(gpu_ctx):
    frames, rec, frec = case()
    wout, wfr = want("main")
    assert_same(gpu_ctx.measure_seeing(frames[0], rec[0], frec[:1], **MAIN), (wout[:1], wfr[:1]), "one frame")
    assert_same(gpu_ctx.measure_seeing(frames, rec, frec, sigma=0.025, **MAIN), (wout, wfr), "one sigma")
    sig = np.array([0.4, 0.5, 0.0125, 0.4], np.float32)           # floors of 60 and 75: among the peaks
    w2 = R.measure_batch(frames, rec, frec, sig, **MAIN)
    assert not np.array_equal(w2[1]["n_cand"], wfr["n_cand"])
    assert_same(gpu_ctx.measure_seeing(frames, rec, frec, sigma=sig, **MAIN), w2, "sigmas")
    out, fr = gpu_ctx.measure_seeing(frames[:0], rec[:0], frec[:0])
    assert out.shape[0] == 0 and len(fr) == 0


def _device_frames(ctx, be):
    """big-endian bytes in device memory as the ``DeviceFrames`` the bzip2 decoder hands out"""
    import torch
    from lfd_amd import _native
    t = torch.from_numpy(np.array(be).view(np.uint8).reshape(-1)).cuda()
    d = _native.DeviceFrames(t.data_ptr(), be.shape)
    d._keep = t
    return d


def test_big_endian_every_loc_and_device_records(gpu_ctx):
    import torch
    from lfd_amd import psf
    frames, rec, frec = case()
    w = want("main")
    be = frames.astype(">f4")
    assert_same(gpu_ctx.measure_seeing(be, rec, frec, **MAIN), w, "big-endian host")
    assert np.array_equal(be.view(np.uint32), frames.astype(">f4").view(np.uint32))            # only read
    pin = gpu_ctx.pinned_buffer(frames.nbytes)
    pv = pin.array.view("<f4").reshape(frames.shape)
    pv[:] = frames
    assert_same(gpu_ctx.measure_seeing(pv, rec, frec, pinned=True, **MAIN), w, "pinned")
    pb = pin.array.view(">f4").reshape(frames.shape)
    pb[:] = frames
    assert_same(gpu_ctx.measure_seeing(pb, rec, frec, pinned=True, **MAIN), w, "pinned big-endian")
    pin.close()
    dev = torch.from_numpy(np.array(frames)).cuda()
    assert_same(gpu_ctx.measure_seeing(dev, rec, frec, **MAIN), w, "device frames, host records")
    drec, dfrec = gpu_ctx.find_stars(dev, max_obj=MAX_OBJ, device_out=True)
    assert dfrec.tobytes() == frec.tobytes()
    assert_same(gpu_ctx.measure_seeing(dev, drec, dfrec, **MAIN), w, "device frames, device records")
    assert_same(gpu_ctx.measure_seeing(frames, drec, dfrec, **MAIN), w, "host frames, device records")
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), frames.view(np.uint32))
    assert drec.cpu().numpy().tobytes() == rec.tobytes()                                       # only read
    dbe = _device_frames(gpu_ctx, be)
    assert_same(gpu_ctx.measure_seeing(dbe, drec, dfrec, **MAIN), w, "device big-endian")
    # the one-call helper: the finder with its records left on the device, then the measurement
    out, fr, sfr = psf.measure_seeing(gpu_ctx, dev, stars_params={"max_obj": MAX_OBJ}, **MAIN)
    assert_same((out, fr), w, "helper")
    assert sfr.tobytes() == frec.tobytes()
    # the host step of the package on the packed records: the library's frame records
    host = psf.frame_seeing(out, fr["n_packed"], min_stars=3)
    for k in host.dtype.names:
        assert host[k].tobytes() == np.ascontiguousarray(fr[k]).tobytes(), k


def test_one_frame_per_chunk_gives_the_same_bytes():
    import torch
    from lfd_amd import _native
    frames, rec, frec = case()
    w = want("main")
    with _native.Context(0, SHAPE[0], SHAPE[1], 2) as ctx:
        assert_same(ctx.measure_seeing(frames, rec, frec, **MAIN), w, "unsplit")
        ctx.debug_unit_limits()
        assert_same(ctx.measure_seeing(frames, rec, frec, **MAIN), w, "recorded")
        assert ctx.debug_unit_split() == dict(chunks=1, batches=0, grid=0, launches=0)
        ctx.debug_unit_limits(stage_bytes=1)
        assert_same(ctx.measure_seeing(frames, rec, frec, **MAIN), w, "one host frame per chunk")
        assert ctx.debug_unit_split()["chunks"] == 4
        dev = torch.from_numpy(np.array(frames)).cuda()
        drec, dfrec = ctx.find_stars(dev, max_obj=MAX_OBJ, device_out=True)
        assert_same(ctx.measure_seeing(dev, drec, dfrec, **MAIN), w, "device frames are not staged")
        assert ctx.debug_unit_split()["chunks"] == 1
        ctx.debug_unit_limits(stars_rec_bytes=MAX_OBJ * 64)
        assert_same(ctx.measure_seeing(dev, drec, dfrec, **MAIN), w, "one frame of records per chunk")
        assert ctx.debug_unit_split()["chunks"] == 4
        ctx.debug_unit_limits(stars_rec_bytes=2 * MAX_OBJ * 64)
        assert_same(ctx.measure_seeing(frames, rec, frec, **MAIN), w, "two frames per chunk")
        assert ctx.debug_unit_split()["chunks"] == 2
        with pytest.raises(_native.NativeError):
            ctx.measure_seeing(frames, rec, frec, win=0)
        assert ctx.debug_unit_split() == dict(chunks=0, batches=0, grid=0, launches=0)        # nothing ran


def test_the_library_refuses_what_validate_refuses(gpu_ctx):
    from lfd_amd import _native
    frames, rec, frec = case()
    for bad in REFUSED:
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.measure_seeing(frames[:1], rec[:1], frec[:1], **bad)
        assert e.value.code == _native.ERR_ARG, bad
    for good in TAKEN:
        gpu_ctx.measure_seeing(frames[:1], rec[:1], frec[:1], **good)
    for sigma in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.measure_seeing(frames[:1], rec[:1], frec[:1], sigma=sigma)
        assert e.value.code == _native.ERR_ARG
    for n_out in (-1, MAX_OBJ + 1):
        bad = frec[:1].copy()
        bad["n_out"] = n_out
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.measure_seeing(frames[:1], rec[:1], bad)
        assert e.value.code == _native.ERR_ARG
    with pytest.raises(TypeError):
        gpu_ctx.measure_seeing(frames.astype(np.float64), rec, frec)
    with pytest.raises(ValueError):
        gpu_ctx.measure_seeing(frames, rec[:2], frec[:2])
    # records that point outside the frame are clipped, not read
    wild = rec[:1].copy()
    wild["x"][0, 0], wild["y"][0, 1] = 2 ** 31 - 1, -2 ** 31
    got = gpu_ctx.measure_seeing(frames[:1], wild, frec[:1], **MAIN)
    assert_same(got, R.measure_batch(frames[:1], wild, frec[:1], **MAIN), "wild records")
