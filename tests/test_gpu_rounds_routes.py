"""lfdmi_detect_rounds by every route the frames can take: F32 device, F32_BE device, F32 host, F32 pinned, F32_BE pinned with a
catalogue (the caller's bytes stay untouched; the blot of rounds >= 1 comes from the compacted catalogue); catalogue on the host
and on the device.  The records are identical across all routes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_cases as RC  # noqa: E402
import rounds_gpu as RG  # noqa: E402

from lfd_amd import _native, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    import torch
    frames, cats = RC.frames()
    ctx = _native.Context(0, *RC.SHAPE, 8)
    pb, pd, rs, _ = RG.params()
    cat = synth.pack_catalogs(cats)
    want = ctx.detect_rounds(frames.copy(), pb, pd, cat, rs, max_trails=4, half=RC.HALF)
    blotted = frames.copy()
    ctx.detect_batch(blotted, pb, pd, cat, rs)
    dcat = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cat.items()}
    yield frames, cat, dcat, ctx, want, blotted
    ctx.close()


@pytest.mark.parametrize("cat_on", ["host", "device"])
@pytest.mark.parametrize("route", ["f32_device", "be_device", "f32_host", "f32_pinned", "be_pinned"])
def test_route(world, route, cat_on):
    import torch
    frames, cat, dcat, ctx, want, blotted = world
    pb, pd, rs, _ = RG.params()
    c = cat if cat_on == "host" else dcat
    kw = dict(max_trails=4, half=RC.HALF)
    n, h, w = frames.shape
    if route == "f32_device":
        t = torch.from_numpy(frames.copy()).cuda()
        got = ctx.detect_rounds(t, pb, pd, c, rs, **kw)
        after = t.cpu().numpy()
    elif route == "be_device":
        t = torch.from_numpy(frames.astype(">f4").view(np.uint8).reshape(-1).copy()).cuda()
        got = ctx.detect_rounds(_native.DeviceFrames(t.data_ptr(), (n, h, w)), pb, pd, c, rs, **kw)
        torch.cuda.synchronize()
        after = t.cpu().numpy().view("<f4").reshape(n, h, w)               # swapped in place, then blotted
    elif route == "f32_host":
        after = frames.copy()
        got = ctx.detect_rounds(after, pb, pd, c, rs, **kw)
    else:
        buf = ctx.pinned_buffer(frames.nbytes)
        be = route == "be_pinned"
        view = buf.array.view(">f4" if be else "<f4").reshape(n, h, w)
        view[...] = frames
        before = buf.array.tobytes()
        got = ctx.detect_rounds(view, pb, pd, c, rs, pinned=True, **kw)
        if be:
            assert buf.array.tobytes() == before                            # a file's bytes stay as they are
            after = None
        else:
            after = np.array(view)
        del view
        buf.close()
    assert RG.same(got, want)
    if after is not None:
        assert after.tobytes() == blotted.tobytes()                         # as the plain call leaves them; no band in them
