"""The frame previews on the device at their edges, byte for byte: the hand-worked cases of tests/preview_cases.py (which carry
their own answers), ties, a frame without a finite pixel between two ordinary ones, widths and heights at the binning kernel's
tile (a wavefront owns 256 columns and bin rows; four wavefronts share a workgroup) and one off it on either side, one SDSS-size
frame at bin 4 and at bin 1, and n == 0."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_cases as P  # noqa: E402
import preview_ref as R  # noqa: E402
from test_gpu_previews import TEST_LUT, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu


def mode_name(kw):
    kw = dict(kw)
    kw["mode"] = ("rank", "given")[kw.get("mode", R.RANK)]
    return kw


@pytest.mark.parametrize("name", P.NAMES)
def test_hand_worked(gpu_ctx, name):
    c = P.CASES[name]
    out, cells, rec = gpu_ctx.frame_previews(c.frames, lut=P.TEST_LUT, want_cells=True, **mode_name(c.kwargs()))
    P.check(name, out, cells, rec)
    assert_same((out, cells, rec), R.frame_previews(c.frames, P.TEST_LUT, **c.kwargs()), name)


def test_hand_worked_on_the_device_route(gpu_ctx):
    import torch
    for name in ("partial_last_row_and_column", "flat_empty_ordinary", "clamp_and_infinities"):
        c = P.CASES[name]
        dev = torch.from_numpy(np.array(c.frames)).cuda()
        out, cells, rec = gpu_ctx.frame_previews(dev, lut=P.TEST_LUT, want_cells=True, **mode_name(c.kwargs()))
        P.check(name, out, cells, rec)


def test_a_constant_frame_and_a_two_valued_frame(gpu_ctx):
    f = np.zeros((3, 40, 300), np.float32)
    f[0] = 0.125                                             # constant: FLAT
    f[1, :, :150] = 0.25                                     # two values, half and half: the default ranks fall on either side
    f[2, :, :3] = 0.25                                       # 1 % of the columns: rank 10000 ppm stays on the lower value
    for b in (1, 4):
        got = gpu_ctx.frame_previews(f, lut=TEST_LUT, bin=b, want_cells=True)
        w = R.frame_previews(f, TEST_LUT, bin=b)
        assert_same(got, w, b)
        assert got[2]["status"].tolist()[:2] == [R.FLAT, R.OK]


def test_an_empty_frame_between_two_ordinary_ones(gpu_ctx):
    rng = np.random.default_rng(3)
    f = rng.normal(0, 0.025, (3, 33, 70)).astype(np.float32)
    f[1] = np.nan
    for kw in ({}, {"mode": R.GIVEN, "limits": np.array([-0.05, 0.1])}):
        got = gpu_ctx.frame_previews(f, lut=TEST_LUT, want_cells=True, **mode_name(kw))
        assert_same(got, R.frame_previews(f, TEST_LUT, **kw), kw)
        assert got[2]["status"].tolist() == [R.OK, R.EMPTY, R.OK] and not got[0][1].any()


@functools.lru_cache(maxsize=None)
def noise(n, h, w):
    rng = np.random.default_rng(h * 4099 + w)
    f = rng.normal(0.0, 0.025, (n, h, w)).astype(np.float32)
    f[0, h // 2, w // 3] = np.nan
    return f


# widths at one and two wavefronts' columns, heights at one and four preview rows (a workgroup's four wavefronts), +-1 of each
@pytest.mark.parametrize("bin,h,w", [(4, 3, 255), (4, 4, 256), (4, 5, 257), (4, 15, 511), (4, 16, 512), (4, 17, 513),
                                     (16, 15, 255), (16, 16, 256), (16, 17, 257), (16, 63, 512), (16, 64, 513), (16, 65, 511),
                                     (1, 3, 255), (1, 4, 256), (1, 5, 257), (2, 7, 512), (8, 33, 257), (8, 31, 256)])
def test_at_the_tile_sizes(gpu_ctx, bin, h, w):
    f = noise(2, h, w)
    assert_same(gpu_ctx.frame_previews(f, lut=TEST_LUT, bin=bin, want_cells=True), R.frame_previews(f, TEST_LUT, bin=bin), (bin, h, w))


@pytest.mark.parametrize("bin", (4, 1))
def test_one_sdss_frame(gpu_ctx, bin):
    f = noise(1, 1489, 2048)
    got = gpu_ctx.frame_previews(f, lut=TEST_LUT, bin=bin, want_cells=True)
    assert_same(got, R.frame_previews(f, TEST_LUT, bin=bin), bin)
    assert got[0].shape == (1, -(-1489 // bin), 2048 // bin) and got[2]["n_empty"][0] == (1 if bin == 1 else 0)


def test_no_frame_is_a_valid_call(gpu_ctx):
    out, cells, rec = gpu_ctx.frame_previews(np.zeros((0, 37, 53), np.float32), lut=TEST_LUT, want_cells=True)
    assert out.shape == (0, 10, 14) and cells.shape == (0, 10, 14) and rec.shape == (0,)
    out, rec = gpu_ctx.frame_previews(np.zeros((0, 8, 8), np.float32), mode="given", limits=np.zeros((0, 2)))
    assert out.shape == (0, 2, 2) and len(rec) == 0
