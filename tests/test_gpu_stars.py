"""The source finder on the device against its restatement (tests/stars_ref.py), bit for bit: records, frame records and the
catalogue arrays of step 8, on 4 frames of 96 x 160 with injected stars and one streak -- native and big-endian, from host,
page-locked and device memory -- and the argument checks that sit behind the context."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402
from test_stars_abi import REFUSED, TAKEN  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (96, 160)
MAX_OBJ = 96


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_records(got, want, what=""):
    (rec, frec), (wrec, wfrec) = got, want
    assert same_bits(frec, wfrec), (what, frec, wfrec)
    for i in range(len(wfrec)):
        for j in range(rec.shape[1]):
            assert rec[i, j].tobytes() == wrec[i, j].tobytes(), (what, i, j, rec[i, j], wrec[i, j])


@functools.lru_cache(maxsize=None)
def case():
    """4 frames: stars of many fluxes (two on the frame's edge), a streak on frame 1, a NaN and an inf on frame 2"""
    from lfd_amd import synth
    rng = np.random.default_rng(20240607)
    frames = rng.normal(0, 0.025, (4, *SHAPE)).astype(np.float32)
    for i in range(4):
        n = 12
        ys, xs = rng.uniform(0, SHAPE[0], n), rng.uniform(0, SHAPE[1], n)
        ys[0], xs[1] = 0.3, SHAPE[1] - 0.6
        synth._add_stars(frames[i], ys, xs, np.exp(rng.uniform(np.log(2.0), np.log(2000.0), n)), 1.5)
    synth._add_streak(frames[1], 40.0, 80.0, 30.0, 1.0, 2.0)
    frames[2, 50, 70], frames[2, 10, 10] = np.nan, np.inf
    want = R.find_stars_batch(frames, max_obj=MAX_OBJ)
    frames.setflags(write=False)
    return frames, want


def test_records_and_catalogue(gpu_ctx):
    from lfd_amd import stars
    frames, want = case()
    wrec, wfrec = want
    assert wfrec["n_found"].min() >= 8 and wfrec["n_found"].max() < MAX_OBJ
    assert np.count_nonzero(wrec["flags"] & R.EXTENDED) >= 5 and np.count_nonzero(wrec["flags"] & R.EDGE) >= 2
    got = stars.find_stars(gpu_ctx, frames, max_obj=MAX_OBJ)
    assert got[0].dtype == R.STAR_DTYPE and got[0].shape == (4, MAX_OBJ)
    assert_records(got, want)
    wcat = R.to_catalog(wrec, wfrec, 0.396)
    for cat in (gpu_ctx.stars_catalog(got[0], got[1], 0.396), stars.to_catalog(got[0], got[1], 0.396)):
        assert set(cat) == set(wcat)
        for k in wcat:
            assert same_bits(cat[k], wcat[k]), k
    # one frame alone, as a 2-d array
    one = gpu_ctx.find_stars(frames[3], max_obj=MAX_OBJ)
    assert_records(one, (wrec[3:], wfrec[3:]), "one frame")


def test_big_endian_and_every_loc(gpu_ctx):
    import torch
    frames, want = case()
    be = frames.astype(">f4")
    assert_records(gpu_ctx.find_stars(be, max_obj=MAX_OBJ), want, "big-endian host")
    assert same_bits(be.view(np.uint32), frames.astype(">f4").view(np.uint32))        # only read
    pin = gpu_ctx.pinned_buffer(frames.nbytes)
    pv = pin.array.view("<f4").reshape(frames.shape)
    pv[:] = frames
    assert_records(gpu_ctx.find_stars(pv, pinned=True, max_obj=MAX_OBJ), want, "pinned")
    pb = pin.array.view(">f4").reshape(frames.shape)
    pb[:] = frames
    assert_records(gpu_ctx.find_stars(pb, pinned=True, max_obj=MAX_OBJ), want, "pinned big-endian")
    pin.close()
    dev = torch.from_numpy(np.array(frames)).cuda()
    assert_records(gpu_ctx.find_stars(dev, max_obj=MAX_OBJ), want, "device")
    assert same_bits(dev.cpu().numpy(), frames)
    # records kept on the device, and the catalogue built there from them
    drec, frec = gpu_ctx.find_stars(dev, max_obj=MAX_OBJ, device_out=True)
    back = drec.cpu().numpy().view(R.STAR_DTYPE).reshape(4, MAX_OBJ)
    assert_records((back, frec), want, "device records")
    dcat = gpu_ctx.stars_catalog(drec, frec, 0.396, device=True)
    wcat = R.to_catalog(*want, 0.396)
    for k in wcat:
        assert same_bits(dcat[k].cpu().numpy(), wcat[k]), k
    dbe = _device_frames(gpu_ctx, be)
    assert_records(gpu_ctx.find_stars(dbe, max_obj=MAX_OBJ), want, "device big-endian")


def _device_frames(ctx, be):
    """big-endian bytes in device memory as the ``DeviceFrames`` the bzip2 decoder hands out"""
    import torch
    from lfd_amd import _native
    t = torch.from_numpy(np.array(be).view(np.uint8).reshape(-1)).cuda()
    d = _native.DeviceFrames(t.data_ptr(), be.shape)
    d._keep = t
    return d


def test_sigma_per_frame_and_defaults(gpu_ctx):
    frames, want = case()
    sig = np.array([0.025, 0.05, 0.0125, 0.1], np.float32)
    w2 = R.find_stars_batch(frames, sig, max_obj=MAX_OBJ)
    assert not same_bits(w2[1], want[1])
    assert_records(gpu_ctx.find_stars(frames, sigma=sig, max_obj=MAX_OBJ), w2, "sigmas")
    assert_records(gpu_ctx.find_stars(frames, sigma=0.025, max_obj=MAX_OBJ), want, "one sigma")
    rec, frec = gpu_ctx.find_stars(frames[:1])                                     # the default max_obj
    assert rec.shape == (1, 4096) and same_bits(rec[:, :MAX_OBJ], want[0][:1]) and not rec[:, MAX_OBJ:].view(np.uint8).any()


def test_the_library_refuses_what_validate_refuses(gpu_ctx):
    from lfd_amd import _native
    frames, _ = case()
    for bad in REFUSED:
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.find_stars(frames[:1], **bad)
        assert e.value.code == _native.ERR_ARG, bad
    for good in TAKEN:
        if good.get("max_obj", 0) <= 4096:
            gpu_ctx.find_stars(frames[:1], **good)
    for sigma in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_native.NativeError) as e:
            gpu_ctx.find_stars(frames[:1], sigma=sigma)
        assert e.value.code == _native.ERR_ARG
    with pytest.raises(TypeError):
        gpu_ctx.find_stars(frames.astype(np.float64))
    rec, frec = gpu_ctx.find_stars(frames[:0])
    assert rec.shape[0] == 0 and len(frec) == 0
