"""The frame previews on the device against their restatement (tests/preview_ref.py): every byte of the images, every int64
cell and every field of every record, at every bin and in both modes, on frames whose rows start off a 16 B boundary (37 x 53,
25 x 25) and on one whose rows do not (64 x 256).  No tolerance: every comparison is on bytes."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((37, 53), (25, 25), (64, 256))
TEST_LUT = ((np.arange(R.LUT) // 16 + np.arange(R.LUT) * 3 + 3) % 256).astype(np.uint8)


def assert_same(got, want, what=""):
    (out, cells, rec), (wout, wcells, wrec) = got, want
    assert out.dtype == np.uint8 and cells.dtype == np.int64 and rec.dtype == R.FRAME_DTYPE, what
    assert out.shape == wout.shape and cells.shape == wcells.shape and rec.shape == wrec.shape, (what, out.shape, wout.shape)
    for i in range(len(wrec)):
        assert rec[i].tobytes() == wrec[i].tobytes(), (what, i, rec[i], wrec[i])
        assert cells[i].tobytes() == wcells[i].tobytes(), (what, i, np.argwhere(cells[i] != wcells[i])[:4])
        assert out[i].tobytes() == wout[i].tobytes(), (what, i, np.argwhere(out[i] != wout[i])[:4])


@functools.lru_cache(maxsize=None)
def frames(shape):
    """three frames: noise with a gradient and a few pixels that are not finite, huge, tiny, +0 and -0; a frame of many ties
    (values of a coarse grid); noise with a block of NaN larger than a cell of 16"""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    f = rng.normal(0.0, 0.025, (3, h, w)).astype(np.float32)
    f[0] += np.linspace(-0.05, 0.05, w, dtype=np.float32)[None, :]
    flat = f[0].reshape(-1)
    spots = rng.choice(flat.size, 12, replace=False)
    flat[spots] = np.array([np.nan, np.inf, -np.inf, 3e7, -3e7, 1e-12, -1e-12, 0.0, -0.0, 16777216.0, 1e30, 2.0 ** -31], np.float32)
    f[1] = np.round(f[1] * 80.0) / 80.0
    f[2, 1:min(h, 20), 2:min(w, 23)] = np.nan
    return f


@functools.lru_cache(maxsize=None)
def want(shape, bin, mode):
    kw = {"limits": np.array([[-0.05, 0.25], [0.0, 0.0125], [0.03, -0.03]])} if mode == R.GIVEN else {"lo_ppm": 20000, "hi_ppm": 990000}
    return R.frame_previews(frames(shape), TEST_LUT, bin=bin, mode=mode, **kw), kw


@pytest.mark.parametrize("mode", (R.RANK, R.GIVEN))
@pytest.mark.parametrize("bin", R.BINS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_byte(gpu_ctx, shape, bin, mode):
    w, kw = want(shape, bin, mode)
    f = frames(shape)
    before = f.tobytes()
    got = gpu_ctx.frame_previews(f, lut=TEST_LUT, bin=bin, mode=("rank", "given")[mode], want_cells=True, **kw)
    assert_same(got, w, (shape, bin, mode))
    assert f.tobytes() == before


def test_defaults_and_no_cells(gpu_ctx):
    from lfd_amd import previews
    f = frames((64, 256))
    out, rec = previews.frame_previews(gpu_ctx, f)
    wout, _, wrec = R.frame_previews(f, previews.lut("asinh"))
    assert out.tobytes() == wout.tobytes() and rec.tobytes() == wrec.tobytes() and out.shape == (3, 16, 64)
    one, rec1 = gpu_ctx.frame_previews(f[1])                     # a single 2-d frame
    assert one.shape == (1, 16, 64) and one[0].tobytes() == wout[1].tobytes() and rec1[0].tobytes() == wrec[1].tobytes()
