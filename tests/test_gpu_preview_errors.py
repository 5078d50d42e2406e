"""Every refusal of lfdmi_frame_previews: LFDMI_ERR_ARG, nothing written to the images, the cells or the records, and the
context serves the next call.  The entry point is called as C sees it, so that NULL pointers and bad codes reach it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402
from test_gpu_previews import TEST_LUT  # noqa: E402

from lfd_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 12, 20


def raw_call(ctx, frames=True, dtype=_native.F32, n=2, h=H, w=W, loc=_native.HOST, params=None, limits=None, lut=True, out=True,
             out_loc=_native.HOST, records=True):
    """lfdmi_frame_previews with these arguments -> (return code, the out / cells / records arrays as they were left);
    True: a good array, None: NULL"""
    f = np.full((max(n, 1), 16, 32), 0.5, np.float32)
    o = np.full((max(n, 1), 16, 32), 0xAB, np.uint8)
    cells = np.full((max(n, 1), 16, 32), 0x5A5A, np.int64)
    rec = np.full(max(n, 1), 0x77, np.uint8).repeat(R.FRAME_DTYPE.itemsize).view(R.FRAME_DTYPE)
    p = None
    if params is not None:
        p = _native.PreviewParamsStruct(*params)
    lim = None if limits is None else np.ascontiguousarray(limits, np.float64)
    ptr = _native._ptr
    rc = ctx._lib.lfdmi_frame_previews(ctx._h, ptr(f) if frames else None, dtype, n, h, w, loc, C.byref(p) if p is not None else None,
                                       ptr(lim), ptr(TEST_LUT) if lut else None, ptr(o) if out else None, out_loc, ptr(cells),
                                       ptr(rec) if records else None)
    untouched = (o == 0xAB).all() and (cells == 0x5A5A).all() and (rec.view(np.uint8) == 0x77).all()
    return rc, untouched


REFUSED = {
    "bin 3": dict(params=(3, 0, 10000, 995000)),
    "bin 0": dict(params=(0, 0, 10000, 995000)),
    "bin 32": dict(params=(32, 0, 10000, 995000)),
    "a negative bin": dict(params=(-4, 0, 10000, 995000)),
    "a negative ppm": dict(params=(4, 0, -1, 995000)),
    "a ppm above 1000000": dict(params=(4, 0, 10000, 1000001)),
    "lo_ppm above hi_ppm": dict(params=(4, 0, 600000, 500000)),
    "ppm checked in GIVEN mode too": dict(params=(4, 1, 600000, 500000), limits=[[0.0, 1.0]] * 2),
    "a bad mode": dict(params=(4, 2, 10000, 995000)),
    "a NaN limit": dict(params=(4, 1, 10000, 995000), limits=[[0.0, 1.0], [float("nan"), 1.0]]),
    "an infinite limit": dict(params=(4, 1, 10000, 995000), limits=[[0.0, float("inf")], [0.0, 1.0]]),
    "GIVEN without limits": dict(params=(4, 1, 10000, 995000)),
    "a NULL lut": dict(lut=None),
    "a NULL lut with no frame": dict(lut=None, n=0),
    "h * w above 1e9": dict(h=40000, w=40000),
    "h of 0": dict(h=0),
    "w above 65536": dict(w=65537),
    "a negative n": dict(n=-1),
    "NULL frames": dict(frames=None),
    "NULL out": dict(out=None),
    "NULL records": dict(records=None),
    "a uint8 dtype": dict(dtype=_native.U8),
    "a float64 dtype": dict(dtype=_native.F64),
    "a bad loc": dict(loc=7),
    "a bad out_loc": dict(out_loc=7),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused(gpu_ctx, what):
    rc, untouched = raw_call(gpu_ctx, **REFUSED[what])
    assert rc == _native.ERR_ARG and untouched, what
    assert gpu_ctx._lib.lfdmi_last_error(gpu_ctx._h)            # a message is left
    # the context is usable: the good call runs and writes everything
    rc, untouched = raw_call(gpu_ctx)
    assert rc == 0 and not untouched
    f = np.full((2, H, W), 0.5, np.float32)
    f[1, 0, 0] = 1.0
    out, rec = gpu_ctx.frame_previews(f, lut=TEST_LUT)
    wout, _, wrec = R.frame_previews(f, TEST_LUT)
    assert out.tobytes() == wout.tobytes() and rec.tobytes() == wrec.tobytes()


def test_refused_while_calls_are_in_flight():
    from lfd_amd.detecttrails.detecttrails import default_params
    bright, dim, _ = default_params()
    with _native.Context(0, 64, 64, 2) as ctx:
        import torch
        pending = ctx.detect_batch_begin(torch.zeros((2, 64, 64), dtype=torch.float32, device="cuda"), bright, dim)
        assert ctx.calls_in_flight() == 1
        rc, untouched = raw_call(ctx)
        assert rc == _native.ERR_ARG and untouched
        pending.result()
        assert ctx.calls_in_flight() == 0
        rc, untouched = raw_call(ctx)
        assert rc == 0 and not untouched


def test_python_refuses_what_it_can_see(gpu_ctx):
    f = np.zeros((1, H, W), np.float32)
    with pytest.raises(ValueError):
        gpu_ctx.frame_previews(f, lut=TEST_LUT[:100])
    with pytest.raises(ValueError):
        gpu_ctx.frame_previews(f, mode="given")
    with pytest.raises(TypeError):
        gpu_ctx.frame_previews(f.astype(np.float64))
    with pytest.raises(_native.NativeError) as e:
        gpu_ctx.frame_previews(f, bin=3)
    assert e.value.code == _native.ERR_ARG
