"""lfdmi_sky_normalize on the device against the numpy restatement of its definition (tests/sky_ref.py): records, both meshes
and every output pixel bit for bit; then end to end through BatchDetector(sky=...) against the CPU oracle on the restatement's
output, and the handle's lifecycle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sky_ref as S  # noqa: E402
import trail_ref as T  # noqa: E402
from test_sky_model import disguise, noise  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_rec(dev, ref):
    for k in ("status", "ny", "nx", "n_empty", "sky", "sigma", "gain"):
        a, b = dev[k].item(), ref[k]
        if not (a == b or (isinstance(b, float) and np.isnan(a) and np.isnan(b))):
            return f"{k}: device {a!r} != restatement {b!r}"
    return None


def check(frames_native, dev_out, dev_rec, dev_mb, dev_ms, **params):
    bad = []
    for i, x in enumerate(frames_native):
        out, rec, mb, ms = S.normalize(x, **params)
        msg = same_rec(dev_rec[i], rec)
        if msg is None and not np.array_equal(bits(dev_mb[i]), bits(mb)):
            msg = "sky mesh differs"
        if msg is None and not np.array_equal(bits(dev_ms[i]), bits(ms)):
            msg = "sigma mesh differs"
        if msg is None and not np.array_equal(bits(dev_out[i]), bits(out)):
            msg = "%d output pixels differ" % (bits(dev_out[i]) != bits(out)).sum()
        if msg:
            bad.append((i, msg))
    assert not bad, bad[:5]


def mixed_batch(shape, seed=0):
    """good frames beside every special case: NaN / Inf blocks, an empty cell, NO_SKY, NO_NOISE, -0 pixels"""
    h, w = shape
    f = [disguise(noise(shape, 0.025, seed + k)) for k in range(3)]
    f[1][10:50, 20:90] = np.nan
    f[1][h // 2:h // 2 + 20, w // 2:w // 2 + 30] = np.inf
    f[1][h // 3, :] = -np.inf
    f[2][:min(h, 40), :min(w, 40)] = np.nan
    f.append(np.full(shape, np.nan, np.float32))
    f.append(np.full(shape, 7.0, np.float32))
    z = noise(shape, 1.0, seed + 9)
    z[::3, ::5] = -0.0
    z[1::3, ::5] = 0.0
    f.append(z)
    return np.stack(f)


@pytest.mark.parametrize("shape", [(512, 768), (333, 517)])
@pytest.mark.parametrize("cell", [16, 32, 64, 128, 256])
def test_parity_over_cells_and_shapes(gpu_ctx, shape, cell):
    from lfd_amd import _native
    frames = mixed_batch(shape, seed=cell)
    for n_clip, filt, mode in ((3, 3, S.NORMALISE), (0, 1, S.SUBTRACT), (3, 1, S.SUBTRACT), (0, 3, S.NORMALISE)):
        p = dict(cell=cell, n_clip=n_clip, filter=filt, mode=mode)
        with _native.Sky(gpu_ctx, shape, max_frames=4, **p) as sky:      # 6 frames through 4 slots: two chunks
            out = np.empty_like(frames)
            rec, mb, ms = sky.normalize(frames, out=out, meshes=True)
        assert list(rec["status"][3:5]) == [S.NO_SKY, S.NO_NOISE if mode == S.NORMALISE else S.OK]
        check(frames, out, rec, mb, ms, **p)


def test_parity_on_disguised_sdss_frames_every_route(gpu_ctx):
    """F32 and F32_BE; host, pinned and device input; caller's buffer, in place and the handle's buffer"""
    import torch
    from lfd_amd import _native, synth
    frames = np.stack([disguise(synth.make_frame(k)[0]) for k in range(3)])
    n, h, w = frames.shape
    ref = [S.normalize(x) for x in frames]
    want = np.stack([r[0] for r in ref])

    def ok(out, rec):
        assert all(same_rec(rec[i], ref[i][1]) is None for i in range(n)), [same_rec(rec[i], ref[i][1]) for i in range(n)]
        assert np.array_equal(bits(out), bits(want))
    with _native.Sky(gpu_ctx, (h, w), max_frames=2) as sky:
        out = np.empty_like(frames)
        rec, mb, ms = sky.normalize(frames, out=out, meshes=True)                       # host F32 -> host, chunked
        ok(out, rec)
        assert all(np.array_equal(bits(mb[i]), bits(ref[i][2])) and np.array_equal(bits(ms[i]), bits(ref[i][3])) for i in range(n))
        be = frames.astype(">f4")
        out[:] = 0
        ok(out, sky.normalize(be, out=out))                                             # host F32_BE -> host
        assert np.array_equal(be, frames.astype(">f4"))                                 # only read
        pin = gpu_ctx.pinned_buffer(frames.nbytes)
        pv = pin.array.view(">f4").reshape(frames.shape)
        pv[:] = frames
        dev_out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        rec = sky.normalize(pv, out=dev_out, pinned=True)                               # pinned F32_BE -> caller's device buffer
        ok(dev_out.cpu().numpy(), rec)
        pin.close()
        dev_in = torch.from_numpy(frames).cuda()
        dev_out.zero_()
        rec = sky.normalize(dev_in, out=dev_out)                                        # device -> device
        ok(dev_out.cpu().numpy(), rec)
        assert np.array_equal(dev_in.cpu().numpy(), frames)
        rec = sky.normalize(dev_in, out="inplace")                                      # in place
        ok(dev_in.cpu().numpy(), rec)
        dev_in = torch.from_numpy(frames[:2].copy()).cuda()
        rec2 = sky.normalize(dev_in)                                                    # the handle's buffer
        assert same_rec(rec2[1], ref[1][1]) is None
        with _native.Sky(gpu_ctx, (h, w), max_frames=2, mode="subtract") as again:      # read it back through a second handle
            out2 = np.empty((2, h, w), np.float32)
            again.normalize(sky.frames(2), out=out2)
        assert all(np.array_equal(bits(out2[i]), bits(S.normalize(want[i], mode=S.SUBTRACT)[0])) for i in range(2))
        with pytest.raises(_native.NativeError):
            sky.normalize(torch.from_numpy(frames).cuda())                              # 3 frames, a buffer of 2


def test_end_to_end_detect_and_measure(oracle):
    """plain detection on the disguised frames finds nothing like the original records; BatchDetector(sky={}) gives the
    oracle's records on the restatement's output, and measure_trails the restatement's trails on it"""
    from lfd_amd import _native, synth
    from lfd_amd.batch import BatchDetector
    from lfd_amd.detecttrails import default_params
    pb, pd, prs = default_params()
    shape = (512, 768)
    ks = [2, 3, 4, 5, 10, 12]
    made = [synth.make_frame(k, shape) for k in ks]
    orig = np.stack([m[0] for m in made])
    cats = [m[1] for m in made]
    packed = synth.pack_catalogs(cats)
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    rs_o = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    dis = np.stack([disguise(x) for x in orig])
    bd = BatchDetector(0, shape, inflight=8)
    try:
        base = bd.detect(orig.copy(), pb, pd, packed, rs)
        plain = bd.detect(dis.copy(), pb, pd, packed, rs)
    finally:
        bd.close()
    assert (base["found"] != 0).sum() >= 4
    assert not np.array_equal(plain, base)
    bd = BatchDetector(0, shape, inflight=8, sky={})
    try:
        got = bd.detect(dis.copy(), pb, pd, packed, rs)
        sky_rec = bd.last_sky
        src = dis.copy()
        got2 = bd.detect(src, pb, pd, packed, rs)
        tr, prof = bd.measure_trails(src, got2, packed, rs)
        sub = bd.submit(dis.copy(), pb, pd, packed, rs).result()
    finally:
        bd.close()
    assert np.array_equal(got, got2) and np.array_equal(got, sub)
    for i in range(len(ks)):
        out, rec, _, _ = S.normalize(dis[i])
        assert same_rec(sky_rec[i], rec) is None
        want = oracle.detect_frame(out.copy(), pb, pd, cats[i], rs_o)
        for k, v in want.items():
            assert got[k][i].item() == v, (ks[i], k, got[k][i].item(), v)
    assert (got["found"] != 0).sum() >= 4
    ones = np.ones((len(ks), *shape), np.float32)
    with _native.Context(0, *shape, 8) as ctx:
        ctx.remove_stars(ones, packed, rs)
    for i in range(len(ks)):
        out = S.normalize(dis[i])[0]
        r, p = T.measure(out, got[i]["rho"], got[i]["theta"], found=got[i]["found"], star_mask=ones[i] == 0)
        for k in T.FIELDS:
            a, b = tr[i][k].item(), r[k]
            assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (ks[i], k, a, b)
        assert np.array_equal(prof[i], p, equal_nan=True)


def test_lifecycle_and_refusals():
    import torch
    from lfd_amd import _native, synth
    from lfd_amd.batch import BatchDetector
    from lfd_amd.detecttrails import default_params
    pb, pd, prs = default_params()
    shape = (256, 384)
    x = np.stack([disguise(noise(shape, 0.025, k)) for k in range(2)])
    ctx = _native.Context(0, *shape, 4)
    a = _native.Sky(ctx, shape, max_frames=2)
    b = _native.Sky(ctx, shape, max_frames=2, cell=32, mode="subtract")              # two handles on one context
    ra, rb = a.normalize(x), b.normalize(x)
    assert ra["nx"][0] == 6 and rb["nx"][0] == 12 and (rb["gain"] == 1).all() and (ra["gain"] != 1).all()
    for bad in (dict(n_clip=9), dict(cell=8), dict(cell=300), dict(filter=2), dict(k_clip=0.0), dict(target_sigma=-1.0)):
        with pytest.raises(_native.NativeError) as e:
            _native.Sky(ctx, shape, **bad)
        assert e.value.code == _native.ERR_ARG
    with pytest.raises(_native.NativeError) as e:
        a.normalize(np.zeros((1, 128, 384), np.float32))                                # wrong shape
    assert e.value.code == _native.ERR_ARG
    with pytest.raises(TypeError):
        a.normalize(np.zeros((1, *shape), np.float64))                                  # wrong dtype
    rc = ctx._lib.lfdmi_sky_normalize(ctx._h, a._s, _native._ptr(x), _native.F64, 2, _native.HOST, None, 0,
                                      _native._ptr(np.zeros(2, _native.SKY_DTYPE)), None, None)
    assert rc == _native.ERR_ARG
    assert same_rec(a.normalize(x)[0], S.normalize(x[0])[1]) is None                    # the context stays usable
    dev = torch.from_numpy(np.zeros((2, *shape), np.float32)).cuda()
    pend = ctx.detect_batch_begin(dev, pb, pd)
    with pytest.raises(_native.NativeError) as e:                                       # a call is pending: refused
        a.normalize(x)
    assert e.value.code == _native.ERR_ARG
    pend.result()
    assert same_rec(a.normalize(x)[1], S.normalize(x[1])[1]) is None
    sa, a._s = a._s, None                                                               # destroy after the context's destroy
    ctx.close()
    assert not b._s                                                                     # (closed with its context)
    ctx._lib.lfdmi_sky_destroy(sa)
    # the default sky=None leaves BatchDetector as it was: the golden records
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_golden.json")) as f:
        cases = json.load(f)["cases"][:4]
    bd = BatchDetector(0, tuple(cases[0]["shape"]), inflight=4)
    try:
        assert bd.sky is None and bd.last_sky is None
        made = [synth.make_portable_frame(c["k"], tuple(c["shape"])) for c in cases]
        rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
        recs = bd.detect(np.stack([m[0] for m in made]), pb, pd, synth.pack_catalogs([m[1] for m in made]), rs)
    finally:
        bd.close()
    for c, r in zip(cases, recs):
        assert all(np.float32(r[k]) == np.float32(v) if k in ("rho", "theta") else r[k].item() == v for k, v in c["record"].items()), (c["k"], r)


# ---- drop-in: DetectTrails(normalize=True), sky.txt, Jobs, resume --------------------------------------------------------------
def disguised_tree(root, n=6, bz2_fields=(101, 104)):
    """a small $BOSS tree of disguised portable frames, plain and .fits.bz2 -> (frames, catalogues, header values)"""
    from lfd_amd import synth
    made = [synth.make_portable_frame(k, (512, 768)) for k in range(n)]
    frames = [disguise(m[0]) for m in made]
    cats = [m[1] for m in made]
    hdr = synth.write_boss_tree(root, frames, cats, field0=100, filter="r", bz2_fields=bz2_fields)
    return frames, cats, hdr


def by_hand(frames, cats, hdr):
    """the two-step call: normalise with a Sky handle, detect on its buffer -> (results rows, sky rows)"""
    from lfd_amd import _native, results, sky, synth
    from lfd_amd.detecttrails import default_params
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    x = np.stack(frames)
    with _native.Context(0, 512, 768, 8) as ctx, _native.Sky(ctx, (512, 768), max_frames=len(x)) as h:
        srec = h.normalize(x)
        recs = ctx.detect_batch(h.frames(len(x)), pb, pd, synth.pack_catalogs(cats), rs)
    rows = [results.format_result_row(94, 1, "r", 100 + i, hdr, {k: r[k].item() for k in r.dtype.names})
            for i, r in enumerate(recs) if r["found"]]
    return rows, [sky.format_row((94, 1, "r", 100 + i), srec[i]) for i in range(len(x))]


def lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


@pytest.mark.parametrize("batch", [1, 4])
def test_dropin_normalize_equals_the_two_step_call(tmp_path, batch):
    from lfd_amd import sky
    from lfd_amd.detecttrails import DetectTrails
    frames, cats, hdr = disguised_tree(tmp_path)
    want_rows, want_sky = by_hand(frames, cats, hdr)
    assert len(want_rows) >= 2
    plain = tmp_path / "plain"
    plain.mkdir()
    dt0 = DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain))
    dt0.process(batch=4)
    assert lines(dt0.results) != want_rows and not os.path.exists(dt0.sky_file)          # without the pass: nothing like it
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), normalize=True)
    dt.process(batch=batch)
    assert lines(dt.results) == want_rows and open(dt.errors).read() == ""
    assert lines(dt.sky_file) == want_sky                                                # one row per frame, in order
    rows = sky.read_sky(dt.sky_file)
    assert [r["field"] for r in rows] == list(range(100, 106)) and all(r["status"] == sky.OK and r["gain"] < 0.01 for r in rows)
    dt.process(batch=batch, resume=True)                                                 # nothing left: nothing appended
    assert dt.last_stats["skipped_by_resume"] == 6 and lines(dt.results) == want_rows and lines(dt.sky_file) == want_sky


def test_dropin_resume_after_a_cut_off_chunk(tmp_path):
    """The state a run leaves when it dies inside its second chunk (rows and marks of the first chunk only: rows are flushed
    before marks): resume=True completes the files, no row twice."""
    from lfd_amd.detecttrails import DetectTrails
    frames, cats, hdr = disguised_tree(tmp_path)
    want_rows, want_sky = by_hand(frames, cats, hdr)
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path), normalize=True)
    dt.process(batch=3)
    assert lines(dt.sky_file) == want_sky
    marks = lines(dt.results + ".progress")
    assert len(marks) == 7
    first = {int(m.split()[3]) for m in marks[1:4]}
    with open(dt.results + ".progress", "w") as f:
        f.write("\n".join(marks[:4]) + "\n")
    for path, rows in ((dt.results, want_rows), (dt.sky_file, want_sky)):
        with open(path, "w") as f:
            f.write("".join(r + "\n" for r in rows if int(r.split()[3]) in first))
    dt.process(batch=3, resume=True)
    assert dt.last_stats["skipped_by_resume"] == 3
    assert lines(dt.results) == want_rows and lines(dt.sky_file) == want_sky


def test_dropin_jobs_join_sky_rows_in_selection_order(tmp_path):
    from lfd_amd.jobs import Jobs
    frames, cats, hdr = disguised_tree(tmp_path)
    want_rows, want_sky = by_hand(frames, cats, hdr)
    out = tmp_path / "two"
    out.mkdir()
    results, errors = Jobs(2, devices=[0, 0], run=94, camcol=1, filter="r", savepath=str(out), normalize=True,
                           sky_params={"cell": 64}).launch(batch=2, timeout=600)
    assert lines(results) == want_rows and open(errors).read() == ""
    assert lines(out / "sky.txt") == want_sky
    assert not os.path.exists(str(out / "sky.txt") + ".rank0") and not os.path.exists(str(out / "sky.txt") + ".rank1")
