"""lfdmi_radon_null on the device against the numpy restatement of the null peaks (tests/radon_null_ref.py): every record bit
for bit -- every integer field, the float32 bits of sum, snr, seg_sum and seg_snr and every bit of the doubles -- over shapes
astride 64, a shape where k_radon_first re-tiles, bins, byte orders and locations, frames of planted invalid patterns,
realisations, chunks and seeds, the short and wide kinds, the searches sharing the handle, and every refusal."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_ref as NR  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_tile_cases as TC  # noqa: E402
import test_gpu_radon as TG  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA3 = np.array([0.025, 0.03, 1.0 / 64], np.float32)


def same(dev, ref):
    """every field of a device record against the restatement's dict (a field it does not have, a pad, is 0)"""
    for k in dev.dtype.names:
        kind = dev.dtype.fields[k][0].kind
        if kind == "i":
            if int(dev[k]) != int(ref.get(k, 0)):
                return f"{k}: device {int(dev[k])} != restatement {int(ref.get(k, 0))}"
        elif dev.dtype.fields[k][0].itemsize == 4:
            if TG.f32_bits(dev[k]) != TG.f32_bits(ref[k]):
                return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
        elif int(np.asarray(dev[k], np.float64).view(np.uint64)) != int(np.asarray(ref[k], np.float64).view(np.uint64)):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    return None


def check(dev, want):
    """device records [n, K] against the restatement's [n][K]"""
    assert dev.shape == (len(want), len(want[0])), dev.shape
    bad = [(f, r, msg) for f, row in enumerate(want) for r, ref in enumerate(row) for msg in [same(dev[f, r], ref)] if msg]
    assert not bad, bad[:5]


@functools.lru_cache(maxsize=None)
def shape_case(shape, b):
    """three frames of ``shape`` (dirty noise, a tie frame, a streak), K = 3, and the restatement's records: computed once"""
    frames = TG.batch(shape, seed=shape[0] + b)[1:]
    frames.setflags(write=False)
    min_len = max(1, min(shape) // (2 * b))
    return frames, min_len, NR.null_records(frames, 3, "lines", SIGMA3, bin=b, min_len=min_len)


SHAPES = [(40, 70), (66, 130)]


@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_bins_byte_orders_and_locations(gpu_ctx, shape, b):
    """nine realisations through four slots (three chunks, frames split between them) from host, big-endian, pinned and device
    frames: all the restatement's records, and the frames are only read"""
    import torch
    from lfd_amd import _native
    frames, min_len, want = shape_case(shape, b)
    with _native.Radon(gpu_ctx, shape, max_frames=4, bin=b, min_len=min_len) as r:
        host = r.null(frames, K=3, sigma=SIGMA3)
        assert host.dtype == _native.RADON_DTYPE
        check(host, want)
        assert all(rec["status"] == R.OK for row in want for rec in row)
        be = frames.astype(">f4")
        keep = be.copy()
        assert np.array_equal(r.null(be, K=3, sigma=SIGMA3), host)                       # LFDMI_F32_BE
        assert np.array_equal(be.view(np.uint32), keep.view(np.uint32))
        pin = gpu_ctx.pinned_buffer(frames.nbytes)
        for order in ("<f4", ">f4"):
            pv = pin.array.view(order).reshape(frames.shape)
            pv[:] = frames
            assert np.array_equal(r.null(pv, K=3, sigma=SIGMA3, pinned=True), host), order
        pin.close()
        dev_frames = torch.from_numpy(np.array(frames)).cuda()
        assert np.array_equal(r.null(dev_frames, K=3, sigma=SIGMA3), host)
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))


def test_a_shape_where_the_first_kernel_retiles(gpu_ctx):
    """W1025 of tests/radon_tile_cases.py: 12 x 1025, P = 2048 in orientations 0 and 1, so k_radon_first's strips of 32 columns
    number 64 and the last one holds a single column of the frame; 4-byte rows that start on no 16-byte boundary"""
    from lfd_amd import _native
    c = TC.CASES["W1025"]
    frames = TC.frames("W1025")
    want = NR.null_records(frames, 2, "lines", c["sigma"], seeds=[9], **c["params"])
    with _native.Radon(gpu_ctx, TC.shape("W1025"), max_frames=2, **c["params"]) as r:
        check(r.null(frames, K=2, sigma=c["sigma"], seeds=[9]), want)


def planted(shape, seed, value=None):
    """a frame in which about half the pixels carry a planted pattern: NaNs (one with a payload), +-inf, +-0, and values above
    the clip on either side of it; ``value``: every other pixel has it (then a line's score grows with its count alone)"""
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 0.025, shape).astype(np.float32) if value is None else np.full(shape, value, np.float32)
    pats = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7F812345,
                     np.float32(0.12500001).view(np.uint32), np.float32(-0.5).view(np.uint32), np.float32(3e38).view(np.uint32)], np.uint32)
    where = rng.random(shape) < 0.5
    f.view(np.uint32)[where] = pats[rng.integers(0, len(pats), int(where.sum()))]
    if value is None:
        f[0, 0], f[-1, -1] = np.float32(0.125), np.float32(-0.125)      # |x| = clip is valid
    return f


@pytest.mark.parametrize("b", [1, 2, 4])
def test_planted_patterns_reach_v_and_m_as_the_restatement_says(gpu_ctx, b):
    """what is invalid is neither summed nor counted wherever the scramble puts it.  The records see V and M only through a
    line, so two of the frames hold one value in every valid pixel: a line's score there is value * sqrt(N) / sigma, the best
    line is the one of largest count over the whole of M, and n_pix is that maximum.  The noise frames compare sums."""
    from lfd_amd import _native
    shape = (66, 130)
    frames = np.stack([planted(shape, 1), planted(shape, 2, 1.0 / 64), planted(shape, 3, -1.0 / 64), planted(shape, 4)])
    sigma = np.array([0.025, 1.0 / 64, 1.0 / 64, 0.03], np.float32)
    want = NR.null_records(frames, 4, "lines", sigma, bin=b, min_len=1)
    with _native.Radon(gpu_ctx, shape, max_frames=16, bin=b, min_len=1) as r:
        dev = r.null(frames, K=4, sigma=sigma)
    check(dev, want)
    assert dev["n_pix"].tolist() == [[rec["n_pix"] for rec in row] for row in want]
    # the count frames: the best line is a longest one, and a realisation's count is its own
    V, M = zip(*(R.prepare(NR.scramble(frames[1], 1, k), b, 0.125) for k in range(4)))
    assert [int(dev[1, k]["n_pix"]) for k in range(4)] == [max(int(R.transform(R.orient(M[k], q)).max()) for q in range(4)) for k in range(4)]
    assert len({int(m.sum()) for m in M}) > 1 and all(0 < int(m.sum()) < frames[1].size for m in M)


@functools.lru_cache(maxsize=None)
def small_frames():
    f = np.stack([TG.dirty_noise((40, 70), 50 + k) for k in range(3)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def small_records():
    """the restatement's 64 realisations of the small frames, computed once: realisation r does not depend on K"""
    return NR.null_records(small_frames(), NR.NULL_MAX, "lines", SIGMA3, bin=1, min_len=20)


@pytest.mark.parametrize("n,K", [(1, 1), (1, 5), (2, 4), (3, 5), (1, 64)], ids=lambda v: str(v))
def test_realisations_and_chunks(gpu_ctx, n, K):
    """eight slots: n K below (1, 5), equal to (8) and above them -- 15 realisations of three frames, so a frame's realisations
    split over two chunks, and 64 of one frame in eight chunks"""
    from lfd_amd import _native
    frames = small_frames()[:n]
    with _native.Radon(gpu_ctx, (40, 70), max_frames=8, bin=1, min_len=20) as r:
        dev = r.null(frames, K=K, sigma=SIGMA3[:n])
        one = _native.Radon(gpu_ctx, (40, 70), max_frames=1, bin=1, min_len=20)      # one slot: a chunk per realisation
        with one:
            assert np.array_equal(one.null(frames, K=min(K, 5), sigma=SIGMA3[:n]), dev[:, :min(K, 5)])
    check(dev, [row[:K] for row in small_records()[:n]])


def test_seeds(gpu_ctx):
    from lfd_amd import _native
    f = small_frames()[0]
    frames = np.stack([f, f, f])
    with _native.Radon(gpu_ctx, (40, 70), max_frames=8, bin=1, min_len=20) as r:
        dev = r.null(frames, K=5, seeds=[7, 7, 1 << 63])
        check(dev, NR.null_records(frames, 5, "lines", None, seeds=[7, 7, 1 << 63], bin=1, min_len=20))
        assert np.array_equal(dev[0], dev[1])                                          # equal frames, equal seeds
        assert not np.array_equal(dev[0], dev[2]) and len({r_["snr"].tobytes() for r_ in dev[2]}) == 5
        none = r.null(frames, K=5)
        assert np.array_equal(none, r.null(frames, K=5, seeds=np.arange(3)))           # seeds = NULL: frame f has seed f
        assert not np.array_equal(none[0], none[1])                                    # equal frames, other seeds
        check(none, NR.null_records(frames, 5, "lines", None, bin=1, min_len=20))
        with pytest.raises(ValueError):
            r.null(frames, K=5, seeds=[1, 2])


def test_short_kind(gpu_ctx):
    """24 x 130 at bin 1: P = 256 in orientations 0 and 1, so levels 64 and 128 are scored (orientations 2, 3 have none).  At
    the default threshold no null record is found; at 3.0 some are, and they carry their segments (step 12)"""
    from lfd_amd import _native
    shape = (24, 130)
    frames = np.stack([TG.dirty_noise(shape, 70), TG.dirty_noise(shape, 71)])
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=1, min_len=16) as r:
        dev = r.null(frames, K=4, kind="short", sigma=SIGMA3[:2])
        assert dev.dtype == _native.RADON_SHORT_DTYPE
        want = NR.null_records(frames, 4, "short", SIGMA3[:2], bin=1, min_len=16)
        check(dev, want)
        assert not dev["found"].any() and not dev["seg_n_pix"].any() and {rec["level"] for row in want for rec in row} <= {64, 128}
        kw = {"short_threshold": 3.0, "min_seg": 8, "min_strip": 64}
        low = r.null(frames, K=4, kind="short", sigma=SIGMA3[:2], **kw)
        check(low, NR.null_records(frames, 4, "short", SIGMA3[:2], bin=1, min_len=16, **kw))
        assert low["found"].any() and not low["found"].all()                             # some slots have a line, some do not
        assert (low["seg_n_pix"][low["found"] == 1] >= 8).all() and not low["seg_n_pix"][low["found"] == 0].any()
        check(r.null(frames, K=2, kind="short", min_strip=128), NR.null_records(frames, 2, "short", None, bin=1, min_len=16, min_strip=128))


def test_wide_kind(gpu_ctx):
    """66 x 130 at bin 2 with max_width = 4; found records (threshold 3.0) carry the band's segment (step 16)"""
    from lfd_amd import _native
    shape = (66, 130)
    frames = np.stack([TG.dirty_noise(shape, 80), TG.dirty_noise(shape, 81)])
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=2, min_len=16) as r:
        dev = r.null(frames, K=4, kind="wide", sigma=SIGMA3[:2], max_width=4, min_seg=16)
        assert dev.dtype == _native.RADON_WIDE_DTYPE
        check(dev, NR.null_records(frames, 4, "wide", SIGMA3[:2], bin=2, min_len=16, max_width=4, min_seg=16))
        assert not dev["found"].any() and set(dev["width"].reshape(-1).tolist()) <= {1, 2, 4}
        kw = {"wide_threshold": 3.0, "min_seg": 8, "max_width": 4}
        low = r.null(frames, K=4, kind="wide", sigma=SIGMA3[:2], **kw)
        check(low, NR.null_records(frames, 4, "wide", SIGMA3[:2], bin=2, min_len=16, **kw))
        assert low["found"].any() and not low["found"].all() and len(set(low["width"][low["found"] == 1].tolist())) > 1
        assert (low["seg_n_pix"][low["found"] == 1] >= 8).all() and not low["seg_n_pix"][low["found"] == 0].any()


def test_the_searches_of_the_handle_are_what_they_were(gpu_ctx):
    """the null uses the handle's V, M, planes and record buffers: every search returns the same before and after it"""
    from lfd_amd import _native
    shape = (66, 130)
    frames = TG.batch(shape, seed=31)
    kw = {"max_lines": 2, "peel_halfwidth": 2, "min_seg": 8}
    with _native.Radon(gpu_ctx, shape, max_frames=3, bin=1, min_len=16, threshold=5.0) as r:
        def everything():
            return (r.search(frames), *r.search_lines(frames, **kw), *r.search_short(frames, plain=True, short_threshold=5.0, **kw),
                    *r.search_wide(frames, plain=True, wide_threshold=5.0, max_width=4, **kw))
        before = everything()
        TG.check(frames, before[0], bin=1, min_len=16, threshold=5.0)
        kp = {"lines": {}, "short": {"min_seg": 8}, "wide": {"min_seg": 8, "max_width": 4}}
        nulls = [r.null(frames, K=2, kind=k, **kp[k]) for k in NR.KINDS]
        after = everything()
        assert len(before) == len(after) == 9 and all(np.array_equal(a, b) for a, b in zip(before, after))
        assert all(np.array_equal(r.null(frames, K=2, kind=k, **kp[k]), x) for k, x in zip(NR.KINDS, nulls))


def test_refusals_leave_the_handle_usable():
    import torch
    from lfd_amd import _native, radon
    from lfd_amd.detecttrails import default_params
    shape = (40, 70)
    frames = np.array(small_frames()[:2])
    with _native.Context(0, shape[0], shape[1], 2) as ctx:
        with _native.Radon(ctx, shape, max_frames=2, bin=1, min_len=20) as r:
            first = r.null(frames, K=3)

            def refused(call):
                with pytest.raises(_native.NativeError) as e:
                    call()
                assert e.value.code == _native.ERR_ARG
                assert np.array_equal(r.null(frames, K=3), first)
            for K in (0, -1, 65):
                refused(lambda: r.null(frames, K=K))
            res = np.zeros((2, 3), _native.RADON_WIDE_DTYPE)
            args = (ctx._h, r._r, _native._ptr(frames), _native.F32, 2, _native.HOST, None, None, 3)
            lib = _native.lib()
            for kind in (-1, 3):
                assert lib.lfdmi_radon_null(*args, kind, None, _native._ptr(res)) == _native.ERR_ARG
            p = _native.make_radon_wide_params()
            import ctypes as C
            assert lib.lfdmi_radon_null(*args, _native.RADON_NULL_LINES, C.byref(p), _native._ptr(res)) == _native.ERR_ARG   # LINES takes none
            assert lib.lfdmi_radon_null(*args, _native.RADON_NULL_WIDE, None, None) == _native.ERR_ARG                      # no records
            assert not res.view(np.uint8).any()
            refused(lambda: r.null(frames, K=3, sigma=np.array([0.02, 0.0], np.float32)))
            refused(lambda: r.null(frames, K=3, sigma=-1.0))
            for bad in ({"max_width": 3}, {"min_seg": 21}, {"wide_threshold": 0.0}, {"max_lines": 9}):
                refused(lambda: r.null(frames, K=3, kind="wide", **dict({"min_seg": 8}, **bad)))
            assert r.null(frames, K=3, kind="wide", min_seg=8).shape == (2, 3)
            for bad in ({"min_strip": 32}, {"min_seg": 33}, {"short_threshold": float("nan")}, {"peel_halfwidth": -1}):
                refused(lambda: r.null(frames, K=3, kind="short", **bad))
            with pytest.raises(_native.NativeError):
                r.null(np.zeros((1, 41, 70), np.float32))
            with pytest.raises(ValueError):
                r.null(frames, kind="band")
            with pytest.raises(TypeError):
                r.null(frames, kind="lines", max_width=4)
            pb, pd, _ = default_params()
            pend = ctx.detect_batch_begin(torch.zeros((2, *shape), dtype=torch.float32, device="cuda"), pb, pd)
            with pytest.raises(_native.NativeError) as e:                                  # while a call is in flight
                r.null(frames, K=3)
            assert e.value.code == _native.ERR_ARG
            pend.result()
            assert np.array_equal(r.null(frames, K=3), first)
        peaks = radon.null_peaks(ctx, frames, K=3, bin=1, min_len=20)
        assert peaks.dtype == np.float32 and np.array_equal(peaks, first["snr"])
        assert radon.false_alarm(float(peaks[0].max()) + 1, peaks[0]) == 1 / 4
        assert np.array_equal(radon.null_peaks(ctx, frames[0], K=2, kind="wide", bin=1, min_len=20, max_width=2, min_seg=8)[0],
                              radon.null_peaks(ctx, frames[:1], K=3, kind="wide", bin=1, min_len=20, max_width=2, min_seg=8)[0, :2])
