"""The frame seeing on the device on hand-made records (tests/psf_cases.py), byte for byte against its restatement
(tests/psf_ref.py): lists of more than 64 and more than 256 records, very different n_out in one launch and in uneven chunks,
the four sides of the clip test and the last pixel of the last frame, the bit patterns where psf_fix rounds, pixels at and one ulp
above sat, the largest sums the parameters allow, and records the finder cannot write.  tests/test_psf_cases_model.py checks on
the CPU that each case holds what it is named for.  No tolerance: every comparison is on bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_cases as P  # noqa: E402
from test_gpu_psf import _device_frames, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu


def snapshot(*arrays):
    return [np.array(a).tobytes() for a in arrays]


def on_device(c):
    """the case's frames and records as device tensors, uploaded from the hand-made arrays"""
    import torch
    n, m = c.records.shape
    dev = torch.from_numpy(np.array(c.frames)).cuda()
    drec = torch.from_numpy(np.array(c.records).view(np.uint8).reshape(n, m, c.records.dtype.itemsize)).cuda()
    return dev, drec


@pytest.mark.parametrize("name", P.NAMES)
def test_host_frames_and_host_records(gpu_ctx, name):
    c = P.get(name)
    before = snapshot(c.frames, c.records, c.frame_records)
    got = gpu_ctx.measure_seeing(c.frames, c.records, c.frame_records, sigma=c.sigma, **c.params)
    assert_same(got, P.want(name), name)
    assert snapshot(c.frames, c.records, c.frame_records) == before


@pytest.mark.parametrize("name", P.DEVICE_ROUTE)
def test_device_frames_and_device_records(gpu_ctx, name):
    c = P.get(name)
    dev, drec = on_device(c)
    before = snapshot(c.frame_records)
    assert_same(gpu_ctx.measure_seeing(dev, drec, c.frame_records, sigma=c.sigma, **c.params), P.want(name), name)
    assert_same(gpu_ctx.measure_seeing(c.frames, drec, c.frame_records, sigma=c.sigma, **c.params), P.want(name), name + ": host frames")
    assert dev.cpu().numpy().tobytes() == c.frames.tobytes() and drec.cpu().numpy().tobytes() == c.records.tobytes()       # only read
    assert snapshot(c.frame_records) == before


@pytest.mark.parametrize("name", P.BIG_ENDIAN)
def test_big_endian(gpu_ctx, name):
    c = P.get(name)
    be = c.big_endian()
    assert be.dtype == np.dtype(">f4") and be.tobytes() == c.frames.byteswap().tobytes()
    before = snapshot(be, c.records)
    assert_same(gpu_ctx.measure_seeing(be, c.records, c.frame_records, sigma=c.sigma, **c.params), P.want(name), name + ": host")
    dbe = _device_frames(gpu_ctx, be)
    assert_same(gpu_ctx.measure_seeing(dbe, c.records, c.frame_records, sigma=c.sigma, **c.params), P.want(name), name + ": device")
    assert dbe._keep.cpu().numpy().tobytes() == be.tobytes() and snapshot(be, c.records) == before


def test_uneven_chunks_give_the_same_bytes():
    """n_out = 1101, 257, 0, 65, 600 split into chunks of one frame (the empty frame alone: no measure launch at all) and of two
    (1101 with 257: a launch shaped by the longer list, the shorter one's slots past its n_out)"""
    from lfd_amd import _native
    c = P.get("long_lists")
    cut = P.get("long_lists_cut300")
    assert c.n_out == [1101, 257, 0, 65, 600]
    one = c.max_obj * 64
    h, w = c.frames.shape[1:]
    dev, drec = on_device(c)
    before = snapshot(c.frames, c.records, c.frame_records)
    with _native.Context(0, h, w, 2) as ctx:
        def run(case, frames, rec, what):
            assert_same(ctx.measure_seeing(frames, rec, case.frame_records, **case.params), P.want(case.name), what)
            return ctx.debug_unit_split()["chunks"]

        ctx.debug_unit_limits()
        assert run(c, c.frames, c.records, "unsplit") == 1
        ctx.debug_unit_limits(stars_rec_bytes=one)
        assert run(c, c.frames, c.records, "one frame per chunk") == 5
        assert run(cut, dev, drec, "one frame per chunk, on the device, cut at 300") == 5
        ctx.debug_unit_limits(stars_rec_bytes=2 * one)
        assert run(c, c.frames, c.records, "two frames per chunk") == 3
        assert run(cut, c.frames, drec, "two frames per chunk, device records, cut at 300") == 3
        assert run(c, dev, drec, "two frames per chunk, on the device") == 3
        ctx.debug_unit_limits(stars_rec_bytes=2 * one + 63)
        assert run(c, c.frames, c.records, "a limit that is no whole number of frames") == 3
        ctx.debug_unit_limits(stage_bytes=1)
        assert run(c, c.frames, c.records, "one host frame per chunk") == 5
        assert run(c, dev, drec, "device frames are not staged") == 1
        ctx.debug_unit_limits(stage_bytes=3 * h * w * 4, stars_rec_bytes=4 * one)
        assert run(c, c.frames, c.records, "three frames per chunk by the stage") == 2
    assert snapshot(c.frames, c.records, c.frame_records) == before
    assert dev.cpu().numpy().tobytes() == c.frames.tobytes() and drec.cpu().numpy().tobytes() == c.records.tobytes()
