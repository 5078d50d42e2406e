"""lfdmi_radon_null_scheme on the device against the numpy restatement of the null schemes and the peel rounds
(tests/radon_null_schemes_ref.py): every record bit for bit, through ``test_gpu_radon_null.check`` -- the sign-flip, row-shift and
column-shift schemes over shapes, bins, byte orders and locations, a shape where k_radon_first re-tiles, frames of planted invalid
patterns, the scramble through the new entry point against the old one, peel records of the three kinds with frames of one chunk
that have different numbers of lines, the searches sharing the handle, and every refusal of step 22."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_ref as NR  # noqa: E402
import radon_null_schemes_ref as NS  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_tile_cases as TC  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_gpu_radon_null as TN  # noqa: E402

pytestmark = pytest.mark.gpu

NEW = ("signflip", "rowshift", "colshift")
SIGMA3 = TN.SIGMA3


@functools.lru_cache(maxsize=None)
def shape_want(shape, b, scheme):
    frames, min_len, _ = TN.shape_case(shape, b)
    return NS.null_records(frames, 3, "lines", SIGMA3, scheme=scheme, bin=b, min_len=min_len)


@pytest.mark.parametrize("scheme", NEW)
@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("shape", TN.SHAPES, ids=["%dx%d" % s for s in TN.SHAPES])
def test_schemes_over_shapes_bins_byte_orders_and_locations(gpu_ctx, shape, b, scheme):
    """nine realisations through four slots (three chunks, frames split between them) from host, big-endian, pinned and device
    frames: all the restatement's records, and the frames are only read"""
    import torch
    from lfd_amd import _native
    frames, min_len, _ = TN.shape_case(shape, b)
    want = shape_want(shape, b, scheme)
    with _native.Radon(gpu_ctx, shape, max_frames=4, bin=b, min_len=min_len) as r:
        host = r.null(frames, K=3, sigma=SIGMA3, scheme=scheme)
        assert host.dtype == _native.RADON_DTYPE
        TN.check(host, want)
        be = frames.astype(">f4")
        keep = be.copy()
        assert np.array_equal(r.null(be, K=3, sigma=SIGMA3, scheme=scheme), host)        # LFDMI_F32_BE
        assert np.array_equal(be.view(np.uint32), keep.view(np.uint32))
        TN.check(host, NS.null_records(be, 3, "lines", SIGMA3, scheme=scheme, bin=b, min_len=min_len))
        pin = gpu_ctx.pinned_buffer(frames.nbytes)
        for order in ("<f4", ">f4"):
            pv = pin.array.view(order).reshape(frames.shape)
            pv[:] = frames
            assert np.array_equal(r.null(pv, K=3, sigma=SIGMA3, pinned=True, scheme=scheme), host), order
        pin.close()
        dev_frames = torch.from_numpy(np.array(frames)).cuda()
        assert np.array_equal(r.null(dev_frames, K=3, sigma=SIGMA3, scheme=scheme), host)
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))


@pytest.mark.parametrize("scheme", NEW)
def test_a_shape_where_the_first_kernel_retiles(gpu_ctx, scheme):
    """W1025 of tests/radon_tile_cases.py: 12 x 1025, rows that start on no 16-byte boundary, so the row shift wraps inside a
    16-byte group, and the column shift runs over H = 12"""
    from lfd_amd import _native
    c = TC.CASES["W1025"]
    frames = TC.frames("W1025")
    want = NS.null_records(frames, 2, "lines", c["sigma"], seeds=[9], scheme=scheme, **c["params"])
    with _native.Radon(gpu_ctx, TC.shape("W1025"), max_frames=2, **c["params"]) as r:
        TN.check(r.null(frames, K=2, sigma=c["sigma"], seeds=[9], scheme=scheme), want)


@pytest.mark.parametrize("scheme", NEW)
@pytest.mark.parametrize("b", [1, 2, 4])
def test_planted_patterns_under_each_scheme(gpu_ctx, b, scheme):
    """NaNs with payloads, +-inf, +-0 and values on either side of the clip in half the pixels, min_len = 1: what is invalid is
    neither summed nor counted wherever the scheme puts it; under the sign flip every line's count is the frame's own"""
    from lfd_amd import _native
    shape = (66, 130)
    frames = np.stack([TN.planted(shape, 1), TN.planted(shape, 2, 1.0 / 64), TN.planted(shape, 3, -1.0 / 64), TN.planted(shape, 4)])
    sigma = np.array([0.025, 1.0 / 64, 1.0 / 64, 0.03], np.float32)
    want = NS.null_records(frames, 4, "lines", sigma, scheme=scheme, bin=b, min_len=1)
    with _native.Radon(gpu_ctx, shape, max_frames=16, bin=b, min_len=1) as r:
        dev = r.null(frames, K=4, sigma=sigma, scheme=scheme)
    TN.check(dev, want)
    assert dev["n_pix"].tolist() == [[rec["n_pix"] for rec in row] for row in want]
    if scheme == "signflip":
        for k in range(4):
            assert np.array_equal(R.prepare(NS.null_frame(frames[0], 0, k, scheme), b, 0.125)[1], R.prepare(frames[0], b, 0.125)[1])


def test_the_scramble_through_the_new_call_is_the_old_call(gpu_ctx):
    from lfd_amd import _native
    shape = (66, 130)
    frames = np.stack([TG.dirty_noise(shape, 80), TG.dirty_noise(shape, 81)])
    kp = {"lines": {}, "short": {"min_seg": 8, "short_threshold": 3.0}, "wide": {"min_seg": 8, "max_width": 4, "wide_threshold": 3.0}}
    dt = {"lines": _native.RADON_DTYPE, "short": _native.RADON_SHORT_DTYPE, "wide": _native.RADON_WIDE_DTYPE}
    make = {"lines": lambda **kw: None, "short": _native.make_radon_short_params, "wide": _native.make_radon_wide_params}
    lib = _native.lib()
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=1, min_len=16) as r:
        for kind in NR.KINDS:
            old = r.null(frames, K=4, kind=kind, sigma=SIGMA3[:2], **kp[kind])
            new = np.zeros((2, 4), dt[kind])
            p = make[kind](**kp[kind])
            rc = lib.lfdmi_radon_null_scheme(gpu_ctx._h, r._r, _native._ptr(frames), _native.F32, 2, _native.HOST, _native._ptr(SIGMA3[:2].copy()),
                                             None, 4, _native.RADON_NULL_KINDS[kind], None if p is None else C.byref(p),
                                             _native.RADON_NULL_SCRAMBLE, None, 0, _native._ptr(new))
            assert rc == 0 and np.array_equal(new, old), kind
            # an empty peel array goes the same way
            assert np.array_equal(r.null(frames, K=4, kind=kind, sigma=SIGMA3[:2], peel=np.zeros((2, 0), _native.RADON_PEEL_DTYPE),
                                         **kp[kind]), old)


PEEL_KW = {"peel_halfwidth": 2, "min_seg": 8}


@functools.lru_cache(maxsize=None)
def peel_frames():
    """three 66 x 130 frames: dirty noise, TG.batch's streak, and a frame with two planted streaks"""
    shape = (66, 130)
    b = TG.batch(shape, seed=31)
    two = TG.dirty_noise(shape, 40)
    for x in range(shape[1]):
        two[10 + x // 5, x] += 0.07
        two[60 - x // 3, x] += 0.06
    f = np.stack([b[0], b[3], two])
    f.setflags(write=False)
    return f


def as_dicts(peel):
    return [[{k: int(rec[k]) for k in ("q", "y0", "s", "width")} for rec in row] for row in peel]


def test_peel_rounds(gpu_ctx):
    """K = 3, three frames, four slots: n_peel = 0, 1, 2 from the frames' own search_lines lines, frames of one chunk with
    different numbers of lines (width = 0 entries), the short kind, and the wide kind with a width = 4 record"""
    from lfd_amd import _native, radon
    frames = peel_frames()
    shape = frames.shape[1:]
    hp = {"bin": 1, "min_len": 16, "threshold": 5.0}
    with _native.Radon(gpu_ctx, shape, max_frames=4, **hp) as r:
        lines, nl = r.search_lines(frames, sigma=SIGMA3, max_lines=3, **PEEL_KW)
        assert nl.max() >= 2 and len(set(nl.tolist())) > 1, nl
        base = r.null(frames, K=3, sigma=SIGMA3, scheme="signflip", **PEEL_KW)
        TN.check(base, NS.null_records(frames, 3, "lines", SIGMA3, scheme="signflip", **hp))
        for upto in (0, 1, 2):
            peel = radon.peel_from_lines(lines, nl, upto)
            assert peel.shape == (3, upto) and peel.dtype == _native.RADON_PEEL_DTYPE
            assert (peel["width"] == (np.arange(upto)[None, :] < nl[:, None])).all()
            assert as_dicts(peel) == NS.peel_of(lines, nl, upto)
            dev = r.null(frames, K=3, sigma=SIGMA3, scheme="signflip", peel=peel, **PEEL_KW)
            TN.check(dev, NS.null_records(frames, 3, "lines", SIGMA3, scheme="signflip", peel=as_dicts(peel), **hp, **PEEL_KW))
            if upto == 0:
                assert np.array_equal(dev, base)                                        # n_peel = 0: the call without peel
        assert (peel["width"] == 0).any() and (peel["width"] == 1).all(axis=1).any()
        assert not np.array_equal(dev, base)
        # a hole in a frame's list: the place is skipped, the later record still peeled
        holed = peel.copy()
        holed["width"][:, 0] = 0
        TN.check(r.null(frames, K=3, sigma=SIGMA3, scheme="signflip", peel=holed, **PEEL_KW),
                 NS.null_records(frames, 3, "lines", SIGMA3, scheme="signflip", peel=as_dicts(holed), **hp, **PEEL_KW))
        # the short kind, and the wide kind with a band of four lines
        peel1 = radon.peel_from_lines(lines, nl, 1)
        skw = {"short_threshold": 3.0, "min_strip": 64, **PEEL_KW}
        TN.check(r.null(frames, K=3, kind="short", sigma=SIGMA3, scheme="signflip", peel=peel1, **skw),
                 NS.null_records(frames, 3, "short", SIGMA3, scheme="signflip", peel=as_dicts(peel1), **hp, **skw))
        wide = peel.copy()
        wide["width"][1:, 0] = 4
        wkw = {"wide_threshold": 3.0, "max_width": 4, **PEEL_KW}
        dev = r.null(frames, K=3, kind="wide", sigma=SIGMA3, scheme="signflip", peel=wide, **wkw)
        TN.check(dev, NS.null_records(frames, 3, "wide", SIGMA3, scheme="signflip", peel=as_dicts(wide), **hp, **wkw))
        assert dev["found"].any()                                                       # found records carry their segments
        # round k of null_rounds is the call with lines 0 .. k-1
        rounds = radon.null_rounds(gpu_ctx, frames, lines, nl, K=3, sigma=SIGMA3, **hp, **PEEL_KW)
        assert rounds.shape == (3, 3, 3) and np.array_equal(rounds[:, 0], base["snr"])
        assert np.array_equal(np.isnan(rounds[:, :, 0]), np.arange(3)[None, :] > nl[:, None])
        assert np.array_equal(rounds, NS.null_rounds(frames, lines, nl, 3, "lines", SIGMA3, **hp, **PEEL_KW), equal_nan=True)


def test_the_searches_of_the_handle_are_what_they_were(gpu_ctx):
    """the new calls use the handle's V, M, second set, planes and record buffers: every search returns the same before and after"""
    from lfd_amd import _native, radon
    shape = (66, 130)
    frames = TG.batch(shape, seed=31)
    kw = {"max_lines": 2, "peel_halfwidth": 2, "min_seg": 8}
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=1, min_len=16, threshold=5.0) as r:
        def everything():
            return (r.search(frames), *r.search_lines(frames, **kw), *r.search_short(frames, plain=True, short_threshold=5.0, **kw),
                    *r.search_wide(frames, plain=True, wide_threshold=5.0, max_width=4, **kw), r.null(frames, K=2))
        before = everything()
        peel = radon.peel_from_lines(before[1], before[2], 2)
        kp = {"lines": PEEL_KW, "short": {"min_seg": 8}, "wide": {"min_seg": 8, "max_width": 4}}
        nulls = [r.null(frames, K=2, kind=k, scheme=s, **kp[k]) for k in NR.KINDS for s in NEW]
        nulls += [r.null(frames, K=2, kind=k, scheme="signflip", peel=peel, **kp[k]) for k in NR.KINDS]
        after = everything()
        assert len(before) == len(after) == 10 and all(np.array_equal(a, b) for a, b in zip(before, after))
        again = [r.null(frames, K=2, kind=k, scheme=s, **kp[k]) for k in NR.KINDS for s in NEW]
        assert all(np.array_equal(a, b) for a, b in zip(again, nulls))


def test_refusals_leave_the_handle_usable(gpu_ctx):
    """every refusal of step 22, each followed by a good call that returns what it returned before; ``records`` is untouched"""
    from lfd_amd import _native, radon
    shape = (40, 70)                                                                     # bin 1: P = 128, R = 40 (q = 0, 1); P = 64, R = 70 (q = 2, 3)
    frames = np.array(TN.small_frames()[:2])
    lib = _native.lib()
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=1, min_len=20) as r:
        good_peel = np.zeros((2, 2), _native.RADON_PEEL_DTYPE)
        good_peel[0, 0] = (1, -127, 127, 1)
        good_peel[1, 1] = (3, 69, 63, 16)
        first = r.null(frames, K=3, scheme="signflip", peel=good_peel)
        plain = r.null(frames, K=3, scheme="rowshift")
        res = np.full((2, 3 * _native.RADON_WIDE_DTYPE.itemsize), 7, np.uint8)         # room for the largest kind's records

        def refused(scheme, peel, n_peel, K=3, kind=_native.RADON_NULL_LINES, params=None):
            rc = lib.lfdmi_radon_null_scheme(gpu_ctx._h, r._r, _native._ptr(frames), _native.F32, 2, _native.HOST, None, None, K, kind,
                                             params, scheme, None if peel is None else _native._ptr(peel), n_peel, _native._ptr(res))
            assert rc == _native.ERR_ARG, (scheme, n_peel, peel)
            assert (res == 7).all()
            assert np.array_equal(r.null(frames, K=3, scheme="signflip", peel=good_peel), first)
        for scheme in (-1, 4):
            refused(scheme, None, 0)
        for n_peel in (-1, 9):
            refused(_native.RADON_NULL_SIGNFLIP, np.zeros((2, 9), _native.RADON_PEEL_DTYPE), n_peel)
        refused(_native.RADON_NULL_SIGNFLIP, None, 2)                                     # n_peel > 0 without records
        for scheme in (_native.RADON_NULL_SCRAMBLE, _native.RADON_NULL_ROWSHIFT, _native.RADON_NULL_COLSHIFT):
            refused(scheme, good_peel, 2)                                                # peel records with a scheme that moves pixels
        for bad in ((-1, 0, 0, 1), (4, 0, 0, 1), (0, 0, 0, 3), (0, 0, 0, 32), (0, 0, 0, -1), (0, 0, -1, 1), (0, 0, 128, 1), (2, 0, 64, 1),
                    (0, -128, 0, 1), (0, 40, 0, 1), (2, -64, 0, 1), (3, 70, 0, 2)):
            peel = good_peel.copy()
            peel[1, 0] = bad
            refused(_native.RADON_NULL_SIGNFLIP, peel, 2)
        # what lfdmi_radon_null refuses
        for K in (0, 65):
            refused(_native.RADON_NULL_SIGNFLIP, None, 0, K=K)
        for kind in (-1, 3):
            refused(_native.RADON_NULL_SIGNFLIP, None, 0, kind=kind)
        lp = _native.make_radon_lines_params(min_seg=21)                                 # above the handle's min_len
        refused(_native.RADON_NULL_SIGNFLIP, None, 0, params=C.byref(lp))
        wp = _native.make_radon_wide_params(max_width=3)
        refused(_native.RADON_NULL_SIGNFLIP, None, 0, kind=_native.RADON_NULL_WIDE, params=C.byref(wp))
        rc = lib.lfdmi_radon_null_scheme(gpu_ctx._h, r._r, _native._ptr(frames), _native.F32, 2, _native.HOST, None, None, 3, 0, None, 1, None, 0, None)
        assert rc == _native.ERR_ARG                                                     # no records
        with pytest.raises(_native.NativeError) as e:
            r.null(frames, K=3, scheme="signflip", sigma=-1.0)
        assert e.value.code == _native.ERR_ARG
        with pytest.raises(_native.NativeError) as e:
            r.null(frames, K=3, scheme="colshift", peel=good_peel)
        assert e.value.code == _native.ERR_ARG
        # the Python side's own checks
        with pytest.raises(ValueError):
            r.null(frames, scheme="flip")
        with pytest.raises(ValueError):
            r.null(frames, scheme="signflip", peel=good_peel[:1])
        with pytest.raises(TypeError):
            r.null(frames, scheme="signflip", max_width=4)
        with pytest.raises(ValueError):
            radon.null_peaks(gpu_ctx, frames, K=3, scheme="rowshift", peel=good_peel, bin=1, min_len=20)
        # a record of width 0 is not looked at
        loose = good_peel.copy()
        loose[0, 1] = (9, 999, -5, 0)
        assert np.array_equal(r.null(frames, K=3, scheme="signflip", peel=loose), first)
        assert np.array_equal(r.null(frames, K=3, scheme="rowshift"), plain)
        TN.check(first, NS.null_records(frames, 3, "lines", None, scheme="signflip", peel=as_dicts(good_peel), bin=1, min_len=20))
    peaks = radon.null_peaks(gpu_ctx, frames, K=3, scheme="signflip", peel=good_peel, bin=1, min_len=20)
    assert peaks.dtype == np.float32 and np.array_equal(peaks, first["snr"])
    assert radon.shift_scheme_for(0) == radon.shift_scheme_for(1) == "colshift" and radon.shift_scheme_for(3) == "rowshift"
