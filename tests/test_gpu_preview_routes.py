"""The frame previews by every route, byte for byte against the restatement: native and big-endian frames on the device, host
frames, pinned frames of both byte orders; images and cells on the host and left on the device; the caller's frames untouched;
a device buffer that starts off a 16 B boundary; and the same call with its chunk limits lowered so that 5 frames split unevenly."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402
from test_gpu_previews import TEST_LUT, assert_same  # noqa: E402
from test_gpu_psf import _device_frames  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N = 45, 260, 5
KW = {"bin": 4, "lo_ppm": 30000, "hi_ppm": 980000}


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(77)
    f = rng.normal(0.0, 0.025, (N, H, W)).astype(np.float32)
    f += np.arange(N, dtype=np.float32)[:, None, None] * np.float32(0.01)      # every frame has limits of its own
    f[1, 3, 5], f[3, 40, 259] = np.nan, np.inf
    f[2] = np.nan                                                            # an EMPTY frame inside a chunk
    return f


@functools.lru_cache(maxsize=None)
def want():
    return R.frame_previews(frames(), TEST_LUT, **KW)


def pinned_copy(ctx, a):
    buf = ctx.pinned_buffer(a.nbytes)
    view = buf.array.view(a.dtype).reshape(a.shape)
    view[...] = a
    return buf, view


@pytest.mark.parametrize("out_device", (False, True))
def test_every_route(gpu_ctx, out_device):
    import torch
    f = frames()
    be = f.astype(">f4")

    def run(x, what, **kw):
        out, cells, rec = gpu_ctx.frame_previews(x, lut=TEST_LUT, want_cells=True, out_device=out_device, **KW, **kw)
        if out_device:
            assert out.is_cuda and cells.is_cuda and out.dtype == torch.uint8 and cells.dtype == torch.int64
            out, cells = out.cpu().numpy(), cells.cpu().numpy()
        assert_same((out, cells, rec), want(), what)

    dev = torch.from_numpy(f.copy()).cuda()
    run(dev, "F32 device")
    assert dev.cpu().numpy().tobytes() == f.tobytes()
    dbe = _device_frames(gpu_ctx, be)
    run(dbe, "F32_BE device")
    assert dbe._keep.cpu().numpy().tobytes() == be.tobytes()
    before = f.tobytes()
    run(f, "F32 host")
    run(be, "F32_BE host")
    assert f.tobytes() == before and be.tobytes() == f.byteswap().tobytes()
    for a, what in ((f, "F32 pinned"), (be, "F32_BE pinned")):
        buf, view = pinned_copy(gpu_ctx, a)
        run(view, what, pinned=True)
        assert view.tobytes() == a.tobytes()
        buf.close()


def test_a_device_buffer_off_the_16_byte_boundary(gpu_ctx):
    """W = 260 is a multiple of 4, so aligned frames take the 16 B loads; the same frames one float further on may not"""
    import torch
    f = frames()
    flat = torch.zeros(f.size + 4, dtype=torch.float32, device="cuda")
    for off in (1, 2, 3):
        flat[off:off + f.size] = torch.from_numpy(f.reshape(-1)).cuda()
        dev = flat[off:off + f.size].view(N, H, W)
        assert dev.data_ptr() % 16 == 4 * off
        got = gpu_ctx.frame_previews(dev, lut=TEST_LUT, want_cells=True, **KW)
        assert_same(got, want(), off)


def test_uneven_chunks_give_the_same_bytes():
    import torch
    from lfd_amd import _native
    f = frames()
    dev = torch.from_numpy(f.copy()).cuda()
    cell_plane = -(-H // 4) * -(-W // 4) * 8
    with _native.Context(0, H, W, 2) as ctx:
        def run(x, what, **kw):
            got = ctx.frame_previews(x, lut=TEST_LUT, want_cells=True, **KW, **kw)
            if kw.get("out_device"):
                got = (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2])
            assert_same(got, want(), what)
            return ctx.debug_unit_split()["chunks"]

        ctx.debug_unit_limits()
        assert run(f, "unsplit") == 1
        ctx.debug_unit_limits(cell_bytes=2 * cell_plane)
        assert run(f, "two frames per chunk by the cells") == 3
        assert run(dev, "two frames per chunk by the cells, on the device") == 3
        assert run(dev, "two frames per chunk, everything on the device", out_device=True) == 3
        ctx.debug_unit_limits(cell_bytes=2 * cell_plane + 7)
        assert run(f, "a limit that is no whole number of frames") == 3
        ctx.debug_unit_limits(cell_bytes=1)
        assert run(f, "one frame alone always fits") == 5
        ctx.debug_unit_limits(stage_bytes=3 * H * W * 4)
        assert run(f, "three frames per chunk by the stage") == 2
        assert run(dev, "device frames are not staged") == 1
        ctx.debug_unit_limits(stage_bytes=4 * H * W * 4, cell_bytes=3 * cell_plane)
        assert run(f.astype(">f4"), "the smaller of the two limits") == 2
        lim = np.tile(np.array([[-0.02, 0.08]]), (N, 1)) + np.arange(N)[:, None] * 0.01
        got = ctx.frame_previews(f, lut=TEST_LUT, want_cells=True, bin=4, mode="given", limits=lim)
        assert ctx.debug_unit_split()["chunks"] == 2                          # (each chunk takes its own frames' limits)
        assert_same(got, R.frame_previews(f, TEST_LUT, bin=4, mode=R.GIVEN, limits=lim), "given limits across chunks")
    assert dev.cpu().numpy().tobytes() == f.tobytes()
