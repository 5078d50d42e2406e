"""The found catalogue in the places a photoObj catalogue goes: ``remove_stars_found`` blots what ``Context.remove_stars`` blots
with the restatement's catalogue (tests/stars_ref.py), and ``BatchDetector(stars={})`` without catalogues returns the records of
``detect`` with that catalogue passed explicitly; ``DetectTrails(find_stars=True)`` over a tree without photoObj files writes
the results.txt of the per-frame path over the same frames with the restatement's catalogue as their photoObj files, and a
stars.txt row per frame."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (372, 512)
MAX_OBJ = 256


@functools.lru_cache(maxsize=None)
def case():
    """8 frames of synth.make_frame, the restatement's catalogue of them and the default parameters"""
    from lfd_amd import _native, synth
    from lfd_amd.detecttrails import default_params
    frames = np.stack([synth.make_frame(k, shape=SHAPE)[0] for k in range(8)])
    rec, frec = R.find_stars_batch(frames, max_obj=MAX_OBJ)
    assert frec["status"].max() == R.OK and frec["n_found"].min() >= 20
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    frames.setflags(write=False)
    return frames, rec, frec, R.to_catalog(rec, frec, prs["pixscale"]), (pb, pd, prs, rs)


def test_remove_stars_found(gpu_ctx):
    import torch
    from lfd_amd.detecttrails.removestars import remove_stars_found
    frames, rec, frec, cat, (pb, pd, prs, rs) = case()
    want = np.array(frames[:3])
    gpu_ctx.remove_stars(want, {k: v[:3] for k, v in cat.items()}, rs)
    assert (want == 0).sum() > 3 * 5000 and not np.array_equal(want, frames[:3])
    kw = {k: v for k, v in prs.items() if k != "debug"}
    for i in range(3):
        img = np.array(frames[i])
        assert remove_stars_found(img, "r", stars_params={"max_obj": MAX_OBJ}, **kw) is img
        assert np.array_equal(img.view(np.uint32), want[i].view(np.uint32)), i
    dev = torch.from_numpy(np.array(frames[1])).cuda()
    remove_stars_found(dev, "r", **kw)                        # the default max_obj: the same sources
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    with pytest.raises(ValueError):
        remove_stars_found(np.zeros((2, 8, 8), np.float32), "r")
    with pytest.raises(ValueError):
        remove_stars_found(np.zeros((8, 8), np.float64), "r")


def test_batch_detector_finds_its_catalogue():
    import torch
    from lfd_amd import _native
    from lfd_amd.batch import BatchDetector
    frames, rec, frec, cat, (pb, pd, prs, rs) = case()
    with pytest.raises(ValueError):
        BatchDetector(0, SHAPE, inflight=8, stars={"sep": 9})
    with pytest.raises(ValueError):
        BatchDetector(0, SHAPE, inflight=8, stars={}, lanes=2)
    bd = BatchDetector(0, SHAPE, inflight=8, stars={"max_obj": MAX_OBJ})
    plain = BatchDetector(0, SHAPE, inflight=8)
    try:
        want = plain.detect(torch.from_numpy(np.array(frames)).cuda(), pb, pd, cat, rs)
        assert np.count_nonzero(want["found"]) >= 1
        dev = torch.from_numpy(np.array(frames)).cuda()
        got = bd.detect(dev, pb, pd, None, rs)
        assert got.tobytes() == want.tobytes()
        assert bd.last_stars.tobytes() == frec.tobytes()
        blot = np.array(frames)
        plain.ctx.remove_stars(blot, cat, rs)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), blot.view(np.uint32))      # the frames were blotted with it
        # host frames, and the call in flight
        assert bd.detect(np.array(frames), pb, pd, None, rs).tobytes() == want.tobytes()
        dev2 = torch.from_numpy(np.array(frames)).cuda()
        assert bd.submit(dev2, pb, pd, None, rs).result().tobytes() == want.tobytes()
        # an explicit catalogue wins: an empty one leaves the stars in place
        empty = {k: np.zeros_like(v) for k, v in cat.items()}
        bd.last_stars = None
        no_blot = bd.detect(torch.from_numpy(np.array(frames)).cuda(), pb, pd, empty, rs)
        assert bd.last_stars is None and no_blot.tobytes() == plain.detect(torch.from_numpy(np.array(frames)).cuda(), pb, pd, empty, rs).tobytes()
        with pytest.raises(ValueError):
            bd.detect(dev, pb, pd, None, None)
        # after sky=, the normalised buffer is searched with target_sigma
        sk = BatchDetector(0, SHAPE, inflight=8, sky={}, stars={"max_obj": MAX_OBJ})
        try:
            raw = np.array(frames) * np.float32(2.0) + np.float32(10.0)
            got = sk.detect(raw, pb, pd, None, rs)
            norm = np.empty_like(raw)
            sk.sky.normalize(raw, out=norm)
            r2, f2 = R.find_stars_batch(norm, 0.025, max_obj=MAX_OBJ)
            assert sk.last_stars.tobytes() == f2.tobytes() and len(sk.last_sky) == 8
            want2 = plain.detect(norm, pb, pd, R.to_catalog(r2, f2, prs["pixscale"]), rs)
            assert got.tobytes() == want2.tobytes()
        finally:
            sk.close()
    finally:
        bd.close()
        plain.close()


def _lines(path):
    return open(path).read().splitlines() if os.path.exists(path) else []


@pytest.mark.parametrize("mode", ["plain", "bz2", "normalize"])
def test_detecttrails_finds_its_catalogues(tmp_path, mode):
    """6 fields (frames 4 .. 9 of the recipe: bright, dim and no streak).  Tree ``ref`` carries the restatement's catalogue as
    photoObj files and goes through the per-frame path (batch=1) without find_stars; tree ``raw`` has its photoObj files
    deleted.  ``bz2``: the frames decompressed on the device; ``normalize``: frames that carry a sky, catalogue of the normalised
    frame."""
    from lfd_amd import _native, stars, synth
    from lfd_amd.detecttrails import DetectTrails, default_params, sdssfiles
    from lfd_amd.sky import normalize_frames
    prs = default_params()[2]
    frames = np.stack([synth.make_frame(k, shape=SHAPE)[0] for k in range(4, 10)])
    kw = {}
    seen = frames
    if mode == "normalize":
        frames = frames * np.float32(2.0) + np.float32(10.0)
        kw = {"normalize": True}
        with _native.Context(0, *SHAPE, 8) as ctx:
            seen = normalize_frames(ctx, frames)[0]
    rec, frec = R.find_stars_batch(seen, 0.025)
    cat = R.to_catalog(rec, frec, prs["pixscale"])
    ref, raw = tmp_path / "ref", tmp_path / "raw"
    for d in (ref, raw, tmp_path / "out_ref", tmp_path / "out_1", tmp_path / "out_4", tmp_path / "out_none"):
        d.mkdir()
    synth.write_boss_tree(ref, list(frames), [R.frame_catalog(cat, i) for i in range(6)], field0=100, filter="r")
    want = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path / "out_ref"), **kw)
    want.process(batch=1)
    assert len(_lines(want.results)) >= 2 and not _lines(want.errors) and not os.path.exists(want.stars_file)
    synth.write_boss_tree(raw, list(frames), [R.frame_catalog(cat, i) for i in range(6)], field0=100, filter="r",
                          bz2_all=mode == "bz2")
    for f in range(100, 106):
        os.remove(sdssfiles.filename("photoObj", run=94, camcol=1, field=f))
    rows = [stars.format_row((94, 1, "r", 100 + i), frec[i], stars.n_extended(rec, frec)[i]) for i in range(6)]
    for batch in (1, 4):
        dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path / ("out_%d" % batch)), find_stars=True, **kw)
        dt.process(batch=batch)
        assert _lines(dt.results) == _lines(want.results), batch
        assert not _lines(dt.errors) and _lines(dt.stars_file) == rows, batch
        assert [r["n_found"] for r in stars.read_stars(dt.stars_file)] == frec["n_found"].tolist()
        if mode == "normalize":
            assert len(_lines(dt.sky_file)) == 6
    # without find_stars the same tree fails as before: every frame's photoObj file is missing
    none = DetectTrails(run=94, camcol=1, filter="r", savepath=str(tmp_path / "out_none"), **kw)
    none.process(batch=4)
    assert not _lines(none.results) and not os.path.exists(none.stars_file)
    err = open(none.errors).read()
    assert err.count("photoObj") >= 6 and all(("94 1 r %d" % f) in err for f in range(100, 106))
