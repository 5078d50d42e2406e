"""What lfdmi_detect_rounds refuses (include/lfdmi.h: detection rounds, step 5): the code, the message, and that a refused call
writes no output and leaves nothing behind -- the valid call after it equals the same call on a fresh context.  Argument
refusals only, through ``lib()`` directly (the Python wrapper would refuse first)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_gpu as RG  # noqa: E402

from lfd_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, K = 64, 96, 3
FILL = 0xAB
FN = "lfdmi_detect_rounds"


def make_frames():
    rng = np.random.default_rng(5)
    f = rng.normal(0.0, 0.025, (2, H, W)).astype(np.float32)
    f[0, 30:33, :] += np.float32(2.0)
    return f


def call(ctx, frames, dtype=N.F32, loc=N.HOST, n=2, h=H, w=W, params="default", null=None, bright=True, **fields):
    pb, pd, rs, _ = RG.params()
    b, k1 = N.make_params(pb)
    d, k2 = N.make_params(pd, dim=True)
    p = N.make_rounds_params(max_trails=K)
    for k, v in fields.items():
        setattr(p, k, v)
    outs = [np.empty((2, 8), N.RESULT_DTYPE), np.empty(2, np.int32), np.empty((2, 8), np.int32)]
    for o in outs:
        o.view(np.uint8).reshape(-1)[:] = FILL
    before = [o.tobytes() for o in outs]
    ptrs = [None if null == i else N._ptr(o) for i, o in enumerate(outs)]
    rc = N.lib().lfdmi_detect_rounds(ctx._h, N._ptr(frames), dtype, n, h, w, None, None, C.byref(b) if bright else None, C.byref(d),
                                     C.byref(p) if params == "default" else None, *ptrs, loc)
    return rc, (N.lib().lfdmi_last_error(ctx._h) or b"").decode(), [o.tobytes() for o in outs], before


@pytest.fixture(scope="module")
def world():
    frames = make_frames()
    other = N.Context(0, H, W, 2)
    rc, msg, want, before = call(other, frames.copy())
    assert rc == 0 and all(a != b for a, b in zip(want, before)), (rc, msg)
    ctx = N.Context(0, H, W, 2)
    yield frames, ctx, want
    ctx.close()
    other.close()


def refused(world, code, message, **bad):
    frames, ctx, want = world
    rc, msg, outs, before = call(ctx, bad.pop("frames", frames.copy()), **bad)
    assert (rc, msg) == (code, message)
    assert outs == before
    rc, msg, outs, before = call(ctx, frames.copy())
    assert rc == 0 and outs == want, (rc, msg)


@pytest.mark.parametrize("v", [0, -1, 9])
def test_max_trails_out_of_range(world, v):
    refused(world, N.ERR_ARG, FN + ": max_trails must be 1 .. LFDMI_ROUNDS_MAX_TRAILS", max_trails=v)


@pytest.mark.parametrize("v", [-1.0, float("nan"), float("inf")])
def test_half_and_dup_dist(world, v):
    refused(world, N.ERR_ARG, FN + ": half must be finite and >= 0", half=v)
    refused(world, N.ERR_ARG, FN + ": dup_dist must be finite and >= 0", dup_dist=v)
    refused(world, N.ERR_ARG, FN + ": half must be finite and >= 0", half=v, dup_dist=v)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_null_outputs(world, which):
    refused(world, N.ERR_ARG, FN + ": NULL records, n_found or dup_of", null=which)


def test_what_the_plain_call_refuses(world):
    refused(world, N.ERR_ARG, FN + " takes LFDMI_F32 / LFDMI_F32_BE frames", dtype=N.U8)
    refused(world, N.ERR_ARG, FN + ": bad loc", loc=7)
    refused(world, N.ERR_ARG, FN + ": NULL argument", frames=None)
    refused(world, N.ERR_ARG, FN + ": bad shape", h=0)
    refused(world, N.ERR_CAPACITY, FN + ": frame larger than the context was created for (height and width must both fit)", h=H + 1)


def test_calls_in_flight(world):
    import torch
    frames, ctx, want = world
    pb, pd, rs, _ = RG.params()
    t = torch.from_numpy(frames.copy()).cuda()
    pend = ctx.detect_batch_begin(t, pb, pd)
    try:
        rc, msg, outs, before = call(ctx, frames.copy())
        assert (rc, msg) == (N.ERR_ARG, FN + ": calls in flight on this context: lfdmi_end_oldest them first") and outs == before
    finally:
        pend.result()
    rc, msg, outs, before = call(ctx, frames.copy())
    assert rc == 0 and outs == want


def test_defaults_with_null_params(world):
    frames, ctx, want = world
    rc, msg, outs, before = call(ctx, frames.copy(), params=None)
    assert rc == 0, msg
    rec = np.frombuffer(outs[0], N.RESULT_DTYPE)
    assert rec[:8].tobytes() != before[0][:8 * 48]             # [2][4] records written: the defaults' max_trails
