"""The argument contract the measurement units share (csrc/unit.h): which code and which message lfdmi_sky_normalize,
lfdmi_radon_search, lfdmi_radon_search_lines, lfdmi_stack_profiles, lfdmi_inject_trails and lfdmi_measure_trails give for a
dtype they do not take, a bad loc, NULL frames, a sigma that is not positive and a handle of another context, which of two bad
arguments is named, and that n = 0 does nothing.  Every case goes through ``lib()`` directly (the Python wrappers would refuse
first) and is refused on the host before any launch; a refused call writes nothing and leaves nothing behind: the valid call
after it equals, byte for byte, the same call on a context nothing was refused on."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 32, 48                                  # (w is no multiple of 64)
FNS = ("lfdmi_sky_normalize", "lfdmi_radon_search", "lfdmi_radon_search_lines", "lfdmi_stack_profiles", "lfdmi_inject_trails",
       "lfdmi_measure_trails")
WITH_SIGMA = FNS[1:4]
WITH_HANDLE = FNS[:3]
FILL = 0xAB                                    # what every output holds before a call


def make_frames():
    rng = np.random.default_rng(7)
    f = rng.normal(0.0, 0.025, (2, H, W)).astype(np.float32)
    for i, row in enumerate((12, 20)):         # a streak each, three rows wide
        f[i, row - 1:row + 2, 4:44] += np.float32(0.2)
    return f


class Env:
    """a context of two slots with its Sky and Radon handle"""

    def __init__(self):
        from lfd_amd import _native
        self.ctx = _native.Context(0, H, W, 2)
        self.sky = _native.Sky(self.ctx, (H, W), max_frames=2)
        self.radon = _native.Radon(self.ctx, (H, W), max_frames=2, bin=1, min_len=8)

    def close(self):
        self.ctx.close()


def call(env, fn, frames, dtype=None, loc=None, n=2, sigma=None, handle=None):
    """one call of ``fn`` on env's context -> (code, message, the bytes of every output, what they were before the call)"""
    from lfd_amd import _native as N
    lib, ctx, ptr = N.lib(), env.ctx._h, N._ptr
    dtype = N.F32 if dtype is None else dtype
    loc = N.HOST if loc is None else loc
    m = 2 if n else 0                          # segments / trails: none for a call without frames

    def blank(shape, dt):
        a = np.empty(shape, dt)
        a.view(np.uint8).reshape(-1)[:] = FILL
        return a

    if fn == "lfdmi_sky_normalize":
        outs = [blank(2, N.SKY_DTYPE), blank((2, H, W), np.float32)]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_sky_normalize(ctx, handle or env.sky._s, ptr(frames), dtype, n, loc, ptr(outs[1]), N.HOST, ptr(outs[0]), None, None)
    elif fn == "lfdmi_radon_search":
        outs = [blank(2, N.RADON_DTYPE)]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_radon_search(ctx, handle or env.radon._r, ptr(frames), dtype, n, loc, ptr(sigma), ptr(outs[0]))
    elif fn == "lfdmi_radon_search_lines":
        lp = N.make_radon_lines_params(max_lines=2, peel_halfwidth=2, min_seg=4)
        outs = [blank((2, 2), N.RADON_LINE_DTYPE), blank(2, np.int32)]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_radon_search_lines(ctx, handle or env.radon._r, ptr(frames), dtype, n, loc, ptr(sigma), C.byref(lp), ptr(outs[0]),
                                          ptr(outs[1]))
    elif fn == "lfdmi_stack_profiles":
        p = N.make_stack_params(prof_half=6.0, step=0.5, wing=2, min_cols=16, max_shift=2.0)
        seg = np.zeros(2, N.STACK_SEGMENT_DTYPE)
        seg["frame"], seg["x1"], seg["y1"], seg["x2"], seg["y2"] = [0, 1], 5.0, [19.0, 11.0], 42.0, [19.5, 11.0]
        outs = [blank(2, N.STACK_DTYPE), blank((2, N.stack_bins(p)), np.float32)]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_stack_profiles(ctx, ptr(frames), dtype, n, H, W, loc, ptr(seg), m, ptr(sigma), C.byref(p), ptr(outs[0]), ptr(outs[1]),
                                      None, None)
    elif fn == "lfdmi_inject_trails":
        tr = np.zeros(2, N.INJECT_DTYPE)       # one trail per frame
        tr["frame"], tr["rho"], tr["theta"], tr["t0"], tr["t1"], tr["amplitude"] = [0, 1], [10.0, 20.0], [1.2, 0.4], -np.inf, np.inf, 0.5
        tab = np.exp(-0.5 * (np.arange(-8, 9) * 0.25 / 1.5) ** 2).astype(np.float32)
        outs = [blank((2, H, W), np.float32) if frames is None else frames.copy()]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_inject_trails(ctx, None if frames is None else ptr(outs[0]), dtype, n, H, W, loc, ptr(tr), m, ptr(tab), 1, len(tab),
                                     C.c_double(0.25), 2)
    else:
        p = N.make_trail_params(half_width=8, seg_len=8, wing=4, prof_half=6.0)
        rec = np.zeros(2, N.RESULT_DTYPE)
        rec["found"], rec["rho"], rec["theta"] = 1, [19.0, 11.0], np.float32(np.pi / 2)
        outs = [blank(2, N.TRAIL_DTYPE), blank((2, N.trail_bins(p)), np.float32)]
        before = [o.tobytes() for o in outs]
        rc = lib.lfdmi_measure_trails(ctx, ptr(frames), dtype, n, H, W, loc, ptr(rec), None, None, C.byref(p), ptr(outs[0]), ptr(outs[1]))
    return rc, (lib.lfdmi_last_error(ctx) or b"").decode(), [o.tobytes() for o in outs], before


@pytest.fixture(scope="module")
def world():
    """(frames, the context under test, the other context, the valid call's outputs on that other, still fresh, context)"""
    frames = make_frames()
    other = Env()
    want = {}
    for fn in FNS:
        rc, msg, want[fn], before = call(other, fn, frames)
        assert rc == 0, (fn, rc, msg)
        assert all(a != b for a, b in zip(want[fn], before)), fn                   # (the valid call writes every output)
    env = Env()
    yield frames, env, other, want
    env.close()
    other.close()


def refused(world, fn, code, message, **bad):
    frames, env, other, want = world
    rc, msg, outs, before = call(env, fn, bad.pop("frames", frames), **bad)
    assert (rc, msg) == (code, message)
    assert outs == before                                                          # (a refused call writes nothing)
    rc, msg, outs, before = call(env, fn, frames)
    assert rc == 0, (fn, rc, msg)
    assert outs == want[fn]


def takes(fn):
    from lfd_amd import _native as N
    if fn == "lfdmi_inject_trails":
        return N.ERR_ARG, fn + " takes LFDMI_F32 frames"
    return (N.ERR_DTYPE if fn == "lfdmi_measure_trails" else N.ERR_ARG), fn + " takes LFDMI_F32 / LFDMI_F32_BE frames"


@pytest.mark.parametrize("fn", FNS)
def test_a_dtype_it_does_not_take(world, fn):
    from lfd_amd import _native as N
    refused(world, fn, *takes(fn), dtype=N.U8)


@pytest.mark.parametrize("fn", FNS)
def test_bad_loc(world, fn):
    from lfd_amd import _native as N
    refused(world, fn, N.ERR_ARG, "bad loc", loc=7)


@pytest.mark.parametrize("fn", FNS)
def test_null_frames(world, fn):
    from lfd_amd import _native as N
    refused(world, fn, N.ERR_ARG, "NULL argument", n=1, frames=None)


@pytest.mark.parametrize("first", [0.0, float("nan")], ids=["zero", "nan"])
@pytest.mark.parametrize("fn", WITH_SIGMA)
def test_sigma_must_be_positive(world, fn, first):
    from lfd_amd import _native as N
    refused(world, fn, N.ERR_ARG, fn + ": sigma must be positive", sigma=np.array([0.025, first], np.float32))
    refused(world, fn, N.ERR_ARG, fn + ": sigma must be positive", sigma=np.array([first, 0.025], np.float32))


@pytest.mark.parametrize("fn", WITH_HANDLE)
def test_a_handle_of_another_context(world, fn):
    from lfd_amd import _native as N
    other = world[2]
    refused(world, fn, N.ERR_ARG, fn + ": the handle belongs to another context",
            handle=other.sky._s if fn == "lfdmi_sky_normalize" else other.radon._r)


@pytest.mark.parametrize("fn", FNS)
def test_the_dtype_is_checked_before_loc(world, fn):
    from lfd_amd import _native as N
    refused(world, fn, *takes(fn), dtype=N.U8, loc=7)


@pytest.mark.parametrize("fn", FNS)
def test_no_frames_is_no_work(world, fn):
    frames, env, other, want = world
    rc, msg, outs, before = call(env, fn, frames, n=0)
    assert rc == 0, (fn, rc, msg)
    assert outs == before
    rc, msg, outs, before = call(env, fn, frames)
    assert rc == 0 and outs == want[fn], (fn, rc, msg)
