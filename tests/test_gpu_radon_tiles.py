"""The faint-trail search on the device at the sizes where its kernels re-tile (tests/radon_tile_cases.py; DESIGN.md lists the
constants): working arrays of 1024, 1025, 1032 and 2056 columns, wide and tall, against the numpy restatement of steps 1 - 9
(tests/radon_lines_ref.py).  Every integer field, the float32 bits of sum, snr, seg_sum and seg_snr and n_lines exactly, the
doubles to 1e-12, the input untouched.  That each case lands on the path it is there for is checked without a GPU in
tests/test_radon_tiles_model.py; the restatement's records are computed once per case and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_tile_cases as TC  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_gpu_radon_lines as TGL  # noqa: E402

pytestmark = pytest.mark.gpu


def open_handle(ctx, name, max_frames=None):
    from lfd_amd import _native
    n = len(TC.frames(name))
    return _native.Radon(ctx, TC.shape(name), max_frames=n if max_frames is None else max_frames, **TC.CASES[name]["params"])


def differences(name, dev, dev_n):
    """how the device's (records, n_lines) of a case differ from the restatement's"""
    bad = []
    for i, (recs, n_lines) in enumerate(TC.records(name)):
        if int(dev_n[i]) != n_lines:
            bad.append((i, f"n_lines: device {int(dev_n[i])} != restatement {n_lines}"))
        for k, ref in enumerate(recs):
            msg = TGL.same_line(dev[i, k], ref)
            if msg:
                bad.append((i, k, msg))
    return bad


def search_lines(r, name, frames=None):
    c = TC.CASES[name]
    return r.search_lines(TC.frames(name).copy() if frames is None else frames, sigma=c["sigma"], **c["lines"])


@pytest.mark.parametrize("name", list(TC.CASES))
def test_lines_equal_the_restatement_across_the_tiles(gpu_ctx, name):
    from lfd_amd import _native
    frames = TC.frames(name).copy()
    with open_handle(gpu_ctx, name) as r:
        assert (r.p01, r.p23) == tuple(p["P"] for p in TC.launch_facts(name)["pairs"])
        dev, dev_n = search_lines(r, name, frames)
        assert dev.shape == (len(frames), 3) and dev.dtype == _native.RADON_LINE_DTYPE and dev_n.dtype == np.int32
        assert np.array_equal(frames.view(np.uint32), TC.frames(name).view(np.uint32))          # only read
        bad = differences(name, dev, dev_n)
        assert not bad, bad[:5]
        plain = r.search(frames, sigma=TC.CASES[name]["sigma"])
    for i, ref in enumerate(TC.plain(name)):
        assert TG.same_record(plain[i], ref) is None, (i, TG.same_record(plain[i], ref))


def test_w1024_plain_search_repeats_and_byte_orders(gpu_ctx):
    """record 0 is the plain search, a second call returns the same bytes, and the big-endian copy gives them too"""
    from lfd_amd import _native
    name = "W1024"
    frames = TC.frames(name).copy()
    names = list(_native.RADON_DTYPE.names)
    with open_handle(gpu_ctx, name) as r:
        plain = r.search(frames, sigma=TC.CASES[name]["sigma"])
        dev, dev_n = search_lines(r, name)
        assert not differences(name, dev, dev_n)
        assert np.array_equal(plain, dev[:, 0][names])
        assert np.array_equal(r.search(frames, sigma=TC.CASES[name]["sigma"]), plain)     # the alternate buffers do not leak into it
        again, again_n = search_lines(r, name)
        assert again.tobytes() == dev.tobytes() and again_n.tobytes() == dev_n.tobytes()
        be = frames.astype(">f4")
        keep = be.copy()
        got, got_n = search_lines(r, name, be)
        assert got.tobytes() == dev.tobytes() and got_n.tobytes() == dev_n.tobytes()
        assert np.array_equal(be.view(np.uint32), keep.view(np.uint32))


def test_w1032_in_two_chunks_of_one_frame(gpu_ctx):
    """max_frames = 1: the two frames go through the same slot one after the other and give what they give side by side"""
    name = "W1032"
    with open_handle(gpu_ctx, name, max_frames=1) as r:
        dev, dev_n = search_lines(r, name)
    bad = differences(name, dev, dev_n)
    assert not bad, bad[:5]
