"""lfdmi_radon_search on the device against the numpy restatement of its definition (tests/radon_ref.py): every integer field
and the float32 bits of sum and snr exactly, the doubles to 1e-12; dtypes, locations, chunking, the untouched input, the CPU
test's noise and trail frames, and DetectTrails(radon=True) end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_ref as R  # noqa: E402
import test_radon_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "found", "q", "y0", "s", "n_pix")
F32_FIELDS = ("sum", "snr")
F64_FIELDS = ("x1", "y1", "x2", "y2", "rho", "theta")


def f32_bits(v):
    return int(np.asarray(v, np.float32).view(np.uint32))


def same_record(dev, ref):
    for k in INT_FIELDS:
        if int(dev[k]) != int(ref[k]):
            return f"{k}: device {int(dev[k])} != restatement {int(ref[k])}"
    for k in F32_FIELDS:
        if f32_bits(dev[k]) != f32_bits(ref[k]):
            return f"{k}: device {float(dev[k])!r} != restatement {float(ref[k])!r}"
    for k in F64_FIELDS:
        a, b = float(dev[k]), float(ref[k])
        if abs(a - b) > 1e-12 * abs(b):
            return f"{k}: device {a!r} != restatement {b!r}"
    return None


def check(frames, dev, sigma=None, **params):
    bad = []
    for i, f in enumerate(frames):
        sg = R.DEFAULT_SIGMA if sigma is None else np.asarray(sigma, np.float32).reshape(-1)[i % np.size(sigma)]
        msg = same_record(dev[i], R.search(f, sg, **params))
        if msg:
            bad.append((i, msg))
    assert not bad, bad[:5]


def dirty_noise(shape, seed):
    """noise with NaN, +-inf, zeroed squares (what remove_stars leaves) and pixels above the clip scattered in"""
    h, w = shape
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 0.025, shape).astype(np.float32)
    n = max(3, h * w // 40)
    ys, xs = rng.integers(0, h, n), rng.integers(0, w, n)
    kinds = (np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, -0.7, 0.125, 0.12500001)
    for k in range(n):
        f[ys[k], xs[k]] = kinds[k % len(kinds)]
    for k in range(3):
        y, x, e = rng.integers(0, h), rng.integers(0, w), int(rng.integers(1, 9))
        f[y:y + e, x:x + e] = 0.0
    return f


def tie_frame(shape):
    """small integers: many lines share the best score, so the tie rule decides the record"""
    h, w = shape
    f = np.full(shape, 1.0 / 64, np.float32)
    f[::3, ::2] = 2.0 / 64
    return f


def batch(shape, seed):
    f = [dirty_noise(shape, seed), dirty_noise(shape, seed + 1), tie_frame(shape)]
    line = dirty_noise(shape, seed + 2)
    h, w = shape
    for x in range(w):                                                   # a streak the search has to prefer to the noise
        y = (x * (h - 1)) // max(1, 2 * (w - 1)) + h // 4
        line[min(h - 1, y), x] += 0.06
    f.append(line)
    return np.stack(f)


SHAPES = [((5, 3), 1), ((64, 64), 1), ((37, 50), 1), ((37, 50), 2), ((97, 161), 2), ((97, 161), 4), ((70, 300), 1), ((300, 70), 1)]


@pytest.mark.parametrize("shape,b", SHAPES, ids=["%dx%d-bin%d" % (*s, b) for s, b in SHAPES])
def test_records_equal_the_restatement(gpu_ctx, shape, b):
    from lfd_amd import _native
    frames = batch(shape, seed=shape[0] + b)
    keep = frames.copy()
    min_len = max(1, min(shape) // (2 * b))
    sigma = np.array([0.025, 0.03, 1.0 / 64, 0.02], np.float32)
    with _native.Radon(gpu_ctx, shape, max_frames=4, bin=b, min_len=min_len) as r:
        dev = r.search(frames, sigma=sigma)
        assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))          # only read
        check(frames, dev, sigma, bin=b, min_len=min_len)
        assert dev["status"].tolist() == [0, 0, 0, 0]
        # a frame with no candidate: min_len above every N
        with _native.Radon(gpu_ctx, shape, max_frames=1, bin=b, min_len=4 * max(shape)) as none:
            rec = none.search(frames[:1])[0]
        assert rec["status"] == _native.RADON_NO_LINE and rec["snr"] == 0 and rec["found"] == 0
        assert same_record(rec, R.search(frames[0], bin=b, min_len=4 * max(shape))) is None
        hb, wb = -(-shape[0] // b), -(-shape[1] // b)
        assert (r.p01, r.p23) == (R.pow2_at_least(wb), R.pow2_at_least(hb)) and r.bytes > 0


def test_tie_rule_on_equal_scores(gpu_ctx):
    from lfd_amd import radon
    f = np.full((40, 40), 1.0 / 32, np.float32)                          # every full-length line of every orientation scores alike
    dev = radon.search_frames(gpu_ctx, f, bin=1, min_len=40)
    ref = R.search(f, bin=1, min_len=40)
    assert same_record(dev[0], ref) is None
    assert (ref["q"], ref["s"]) == (0, 0)


def test_chunks_dtypes_and_locations_agree(gpu_ctx):
    import torch
    from lfd_amd import _native
    shape = (37, 50)
    frames = np.stack([dirty_noise(shape, 70 + k) for k in range(5)])
    sigma = np.linspace(0.02, 0.03, 5).astype(np.float32)
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=1, min_len=16) as r:     # n = 5 through two slots: three chunks
        host = r.search(frames, sigma=sigma)
        check(frames, host, sigma, bin=1, min_len=16)
        be = frames.astype(">f4")
        assert np.array_equal(r.search(be, sigma=sigma), host)
        dev_frames = torch.from_numpy(frames).cuda()
        assert np.array_equal(r.search(dev_frames, sigma=sigma), host)
        assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))
        dev_be = torch.from_numpy(be.view(np.uint8).reshape(5, -1).copy()).cuda()
        raw = _native.DeviceFrames(dev_be.data_ptr(), (5, *shape))                 # big-endian device frames
        assert np.array_equal(r.search(raw, sigma=sigma), host)
        assert np.array_equal(dev_be.cpu().numpy().reshape(-1), be.view(np.uint8).reshape(-1))
        with pytest.raises(_native.NativeError):
            r.search(frames, sigma=np.array([0.02, 0.0, 0.02, 0.02, 0.02], np.float32))
        with pytest.raises(_native.NativeError):
            r.search(np.zeros((1, 38, 50), np.float32))
    for bad in ({"bin": 3}, {"clip": 0.0}, {"min_len": 0}):
        with pytest.raises(_native.NativeError):
            _native.Radon(gpu_ctx, shape, **bad)
    with pytest.raises(_native.NativeError):
        _native.Radon(gpu_ctx, (3, 50), bin=2)
    # a line of orientation 0 crosses all 20000 binned columns, four pixels in each: 80000 does not fit the 16-bit counts
    with pytest.raises(_native.NativeError) as e:
        _native.Radon(gpu_ctx, (64, 40000), max_frames=1, bin=2)
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(_native.NativeError) as e:
        _native.Radon(gpu_ctx, (40000, 64), max_frames=1, bin=2)
    assert e.value.code == _native.ERR_ARG


def test_pinned_frames_and_calls_in_flight():
    """LFDMI_HOST_PINNED frames of both byte orders give the host records; a pending detection call refuses the search"""
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (97, 161)
    frames = np.stack([dirty_noise(shape, 90 + k) for k in range(3)])
    with _native.Context(0, shape[0], shape[1], 2) as ctx:
        with _native.Radon(ctx, shape, max_frames=2, bin=2, min_len=16) as r:
            host = r.search(frames)
            check(frames, host, bin=2, min_len=16)
            pin = ctx.pinned_buffer(frames.nbytes)
            pv = pin.array.view("<f4").reshape(frames.shape)
            pv[:] = frames
            assert np.array_equal(r.search(pv, pinned=True), host)
            pb_ = pin.array.view(">f4").reshape(frames.shape)
            pb_[:] = frames
            assert np.array_equal(r.search(pb_, pinned=True), host)
            assert np.array_equal(pb_.view(np.uint32), frames.astype(">f4").view(np.uint32))    # only read
            pin.close()
            assert np.array_equal(r.search(torch.from_numpy(frames).cuda()), host)
            pb, pd, _ = default_params()
            dev = torch.zeros((2, *shape), dtype=torch.float32, device="cuda")
            pend = ctx.detect_batch_begin(dev, pb, pd)
            with pytest.raises(_native.NativeError) as e:
                r.search(frames)
            assert e.value.code == _native.ERR_ARG
            pend.result()
            assert np.array_equal(r.search(frames), host)                             # the context stays usable


@pytest.mark.parametrize("b", [1, 2])
def test_denormal_pixels_count_and_add(gpu_ctx, b):
    """a denormal pixel is valid (finite, not +-0): its value enters the sums unflushed and the line counts it"""
    from lfd_amd import _native
    shape = (37, 50)
    rng = np.random.default_rng(3)
    tiny = np.float32(2.0 ** -140)
    allden = (rng.integers(1, 8, shape).astype(np.float32) * tiny).astype(np.float32)   # every pixel denormal: exact sums
    allden[5:9, 7:30] = 0.0
    mixed = dirty_noise(shape, 17)
    mixed[rng.integers(0, shape[0], 60), rng.integers(0, shape[1], 60)] = tiny * np.float32(3)
    mixed[11, :] = -tiny
    frames = np.stack([allden, mixed])
    assert np.all(np.abs(allden[allden != 0]) < np.finfo(np.float32).tiny)
    with _native.Radon(gpu_ctx, shape, max_frames=2, bin=b, min_len=8) as r:
        dev = r.search(frames)
    check(frames, dev, bin=b, min_len=8)
    assert dev["sum"][0] > 0 and dev["n_pix"][0] >= 8


@pytest.mark.parametrize("b", [1, 2])
def test_noise_and_faint_trails_as_on_the_cpu(gpu_ctx, b):
    """the CPU test's frames; the trails are rendered by Context.inject_trails (bit for bit the restatement's injection)"""
    import torch
    from lfd_amd import _native
    tr, table, step = TM.trail_plan()
    noise = torch.from_numpy(TM.noise_frames().copy()).cuda()
    trails = noise.clone()
    gpu_ctx.inject_trails(trails, tr, table, step)
    assert np.array_equal(trails.cpu().numpy().view(np.uint32), TM.trail_frames().view(np.uint32))
    with _native.Radon(gpu_ctx, TM.SET_SHAPE, max_frames=16, bin=b) as r:
        for kind, frames in (("noise", noise), ("trail", trails)):
            dev = r.search(frames, sigma=TM.SET_SIGMA)
            ref = TM.set_records(kind, b)
            bad = [(i, m) for i, m in ((i, same_record(dev[i], ref[i])) for i in range(len(ref))) if m]
            assert not bad, (kind, bad[:5])
            assert dev["found"].tolist() == [int(kind == "trail")] * TM.SET_SIZE


def test_handle_outlives_and_precedes_its_context():
    from lfd_amd import _native
    ctx = _native.Context(0, 64, 64, 2)
    r = _native.Radon(ctx, (37, 50), max_frames=2, bin=1, min_len=8)
    f = dirty_noise((37, 50), 5)[None]
    a = r.search(f)
    ctx.close()                                                          # closes the handle first
    with pytest.raises(ValueError):
        r.search(f)
    with _native.Context(0, 64, 64, 2) as ctx2:
        with _native.Radon(ctx2, (37, 50), max_frames=2, bin=1, min_len=8) as r2:
            assert np.array_equal(r2.search(f), a)


# ---- drop-in: DetectTrails(radon=True), radon.txt -------------------------------------------------------------------------------
def lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


@pytest.mark.parametrize("batch", [1, 4])
def test_dropin_radon_finds_the_faint_trail_and_leaves_results_alone(tmp_path, batch):
    """three frames of sky noise: nothing, a trail of peak 0.02 (0.8 sky sigma per pixel), a trail of peak 5 the detector finds"""
    import math
    import inject_ref as IR
    from lfd_amd import inject as I, radon, synth
    from lfd_amd.detecttrails import DetectTrails
    shape = (512, 768)
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (3, *shape)).astype(np.float32)
    tr = np.zeros(2, IR.TRAIL_DTYPE)
    th = math.radians(115.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    tr[0] = (1, 0, rho, th, -np.inf, np.inf, 0.02)
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, shape)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r", bz2_fields=(101,) if batch > 1 else ())
    plain = tmp_path / "plain"
    plain.mkdir()
    dt0 = DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain))
    dt0.process(batch=batch)
    assert len(lines(dt0.results)) == 1 and lines(dt0.results)[0].split()[3] == "102"
    assert not os.path.exists(dt0.radon_file)                                             # radon=False: nothing new runs
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), radon=True)
    dt.process(batch=batch)
    assert lines(dt.results) == lines(dt0.results) and open(dt.errors).read() == open(dt0.errors).read()
    rows = radon.read_radon(dt.radon_file)
    assert [r["field"] for r in rows] == [101]
    r = rows[0]
    theta = math.atan2(-(r["x2"] - r["x1"]), r["y2"] - r["y1"]) % math.pi
    line = {"theta": theta, "rho": r["x1"] * math.cos(theta) + r["y1"] * math.sin(theta)}
    deg, px = TM.line_error(line, tr[0], shape)
    assert deg <= 0.5 and px <= 4.0 and r["snr"] >= 8.0 and r["n_pix"] >= 256
