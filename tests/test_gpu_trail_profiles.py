"""lfdmi_measure_trails on the device against the CPU restatement of its definition (tests/trail_ref.py): records and
profiles equal in value (-0.0 == 0.0, NaN where NaN), over synthetic SDSS and 4096 x 4096 frames, every input type and
location, the batch paths, and with star squares, NaN and inf pixels on the trail."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trail_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu


def params():
    from lfd_amd.detecttrails import default_params
    return default_params()


def rs_struct(prs, flt="r"):
    from lfd_amd import _native
    return _native.make_rs_params(flt, **{k: v for k, v in prs.items() if k != "debug"})


def star_masks(ctx, n, shape, packed, rs):
    """remove_stars' squares per frame, from the library's own remove_stars on planes of ones (buffer orientation)"""
    ones = np.ones((n, *shape), np.float32)
    ctx.remove_stars(ones, packed, rs)
    return ones == 0


def same(dev_rec, dev_prof, ref_rec, ref_prof):
    for k in T.FIELDS:
        a, b = dev_rec[k].item(), ref_rec[k]
        if not (a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))):
            return f"{k}: device {a!r} != restatement {b!r}"
    if not np.array_equal(dev_prof, ref_prof, equal_nan=True):
        return f"profile differs at {np.flatnonzero(~((dev_prof == ref_prof) | (np.isnan(dev_prof) & np.isnan(ref_prof))))[:8]}"
    return None


def check_against_ref(frames, recs, out, prof, masks=None):
    bad = []
    for i in range(len(frames)):
        r, p = T.measure(frames[i], recs[i]["rho"], recs[i]["theta"], found=recs[i]["found"],
                         star_mask=None if masks is None else masks[i])
        msg = same(out[i], prof[i], r, p)
        if msg:
            bad.append((i, msg))
    assert not bad, bad[:5]


_CACHE = {}


def sdss_batch(n=64, k0=0):
    """n synthetic SDSS frames (75 % with a bright or dim trail) as detect_batch left them (blotted), the originals, the
    packed catalogue, remove_stars params and the records"""
    key = (n, k0)
    if key in _CACHE:
        return _CACHE[key]
    from lfd_amd import _native, synth
    pb, pd, prs = params()
    frames, cats = zip(*[synth.make_frame(k0 + k)[:2] for k in range(n)])
    orig = np.stack(frames)
    packed = synth.pack_catalogs(list(cats))
    rs = rs_struct(prs)
    blotted = orig.copy()
    with _native.Context(0, *synth.SDSS_SHAPE, 16) as ctx:
        recs = ctx.detect_batch(blotted, pb, pd, packed, rs)
        masks = star_masks(ctx, n, synth.SDSS_SHAPE, packed, rs)
    _CACHE[key] = (blotted, orig, packed, rs, recs, masks)
    return _CACHE[key]


def test_trail_struct_layout():
    from lfd_amd import _native
    assert _native.TRAIL_DTYPE.itemsize == 112
    assert [_native.TRAIL_DTYPE.fields[k][1] for k in ("status", "n_pos", "n_seg", "min_valid", "rho", "depth")] == [0, 4, 8, 12, 16, 104]
    assert C.sizeof(_native.TrailParams) == 48 and _native.TrailParams.k_sig.offset == 16
    with _native.Context(0, 256, 256, 2) as ctx:       # a record the device filled: every field where the layout says
        img = np.zeros((256, 256), np.float32)
        img[:, 120:125] = 1.0
        rec = np.zeros(1, _native.RESULT_DTYPE)
        rec["found"], rec["rho"], rec["theta"] = 1, 122.0, 0.0
        out, prof = ctx.measure_trails(img, rec)
    r, p = T.measure(img, np.float32(122.0), np.float32(0.0))
    assert r["status"] == T.OK and same(out[0], prof[0], r, p) is None


def test_sdss_batch_equals_the_restatement():
    from lfd_amd import _native
    blotted, orig, packed, rs, recs, masks = sdss_batch()
    assert (recs["found"] != 0).sum() >= 32 and ((recs["found"] == 1).any() and (recs["found"] == 2).any())
    with _native.Context(0, 1489, 2048, 16) as ctx:
        b0 = ctx.workspace_bytes()
        out, prof = ctx.measure_trails(blotted, recs, packed, rs)
        assert ctx.workspace_bytes() > b0
    assert (out["status"][recs["found"] != 0] == T.OK).sum() >= 0.8 * (recs["found"] != 0).sum()
    assert (out["status"][recs["found"] == 0] == T.NOT_FOUND).all()
    check_against_ref(blotted, recs, out, prof, masks)


def test_unblotted_big_endian_frames_measure_like_blotted_ones():
    from lfd_amd import _native
    blotted, orig, packed, rs, recs, masks = sdss_batch()
    with _native.Context(0, 1489, 2048, 16) as ctx:
        a, pa = ctx.measure_trails(blotted, recs, packed, rs)
        be = orig.astype(">f4")
        b, pb = ctx.measure_trails(be, recs, packed, rs)
        assert np.array_equal(be, orig.astype(">f4"))          # only read
    assert a.tobytes() == b.tobytes() and np.array_equal(pa, pb, equal_nan=True)
    # and the squares did cross trails
    crossed = [i for i in range(len(recs)) if recs[i]["found"] and a[i]["status"] == T.OK and a[i]["min_valid"] < a[i]["n_pos"]]
    assert crossed


def test_context_without_a_measurement_keeps_its_workspace():
    from lfd_amd import _native
    with _native.Context(0, 1489, 2048, 16) as ctx:
        b0 = ctx.workspace_bytes()
        recs = np.zeros(2, _native.RESULT_DTYPE)
        out, prof = ctx.measure_trails(np.zeros((2, 1489, 2048), np.float32), recs)   # nothing found: no work, no tables
        assert ctx.workspace_bytes() == b0
        assert (out["status"] == T.NOT_FOUND).all() and np.isnan(prof).all()


def test_locations_and_batch_paths_agree():
    import torch
    from lfd_amd import _native
    from lfd_amd.batch import BatchDetector
    blotted, orig, packed, rs, recs, masks = sdss_batch()
    pb, pd, prs = params()
    with _native.Context(0, 1489, 2048, 16) as ctx:
        ref, pref = ctx.measure_trails(blotted, recs, packed, rs)
        buf = ctx.pinned_buffer(blotted.nbytes)
        pin = buf.array.view(np.float32).reshape(blotted.shape)
        pin[:] = blotted
        a, pa = ctx.measure_trails(pin, recs, packed, rs, pinned=True)
        dev = torch.from_numpy(blotted).to("cuda:0")
        dcat = {k: torch.from_numpy(v).to("cuda:0") for k, v in packed.items()}
        b, pbp = ctx.measure_trails(dev, recs, dcat, rs)
        del pin
        buf.close()
    for o, p in ((a, pa), (b, pbp)):
        assert o.tobytes() == ref.tobytes() and np.array_equal(p, pref, equal_nan=True)
    frames = orig.copy()
    bd = BatchDetector(0, inflight=16, calls_in_flight=2)
    try:
        f1 = bd.detect_async(frames[:32], pb, pd, {k: v[:32] for k, v in packed.items()}, rs)
        f2 = bd.detect_async(frames[32:], pb, pd, {k: v[32:] for k, v in packed.items()}, rs)
        r2 = np.concatenate([f1.result(), f2.result()])
        assert r2.tobytes() == recs.tobytes()
        c, pc = bd.measure_trails(frames, r2, packed, rs)
    finally:
        bd.close()
    assert c.tobytes() == ref.tobytes() and np.array_equal(pc, pref, equal_nan=True)
    bd = BatchDetector(0, inflight=16, lanes=2)
    try:
        d, pdd = bd.measure_trails(blotted, recs, packed, rs)
    finally:
        bd.close()
    assert d.tobytes() == ref.tobytes() and np.array_equal(pdd, pref, equal_nan=True)


def test_batch_of_256_equals_single_calls():
    from lfd_amd import _native
    blotted, orig, packed, rs, recs, masks = sdss_batch()
    fr = np.concatenate([blotted] * 4)
    rc = np.concatenate([recs] * 4)
    pk = {k: np.concatenate([v] * 4) for k, v in packed.items()}
    with _native.Context(0, 1489, 2048, 64) as ctx:
        out, prof = ctx.measure_trails(fr, rc, pk, rs)
        for i in range(256):
            o1, p1 = ctx.measure_trails(fr[i], rc[i:i + 1], {k: v[i:i + 1] for k, v in pk.items()}, rs)
            assert o1.tobytes() == out[i:i + 1].tobytes() and np.array_equal(p1[0], prof[i], equal_nan=True), i


def test_edge_cases_and_bad_pixels_equal_the_restatement():
    from lfd_amd import _native
    blotted, orig, packed, rs, recs, masks = sdss_batch()
    i = int(np.flatnonzero(recs["found"])[0])
    img = blotted[i].copy()
    rows = []
    rec = recs[i].copy()
    rows.append(rec.copy())                                        # the detection itself
    corner = rec.copy(); corner["rho"], corner["theta"] = np.float32(60.0), np.float32(math.pi / 4)
    rows.append(corner)                                            # TOO_SHORT
    faint = rec.copy(); faint["rho"], faint["theta"] = np.float32(rec["rho"] + 300), rec["theta"]
    rows.append(faint)                                             # nothing there: TOO_FAINT (or a star run)
    none = rec.copy(); none["found"] = 0
    rows.append(none)                                              # NOT_FOUND
    rows.append(rec.copy())                                        # NaN / inf pixels on the trail
    frames = np.stack([img] * 5)
    th, rho = float(rec["theta"]), float(rec["rho"])
    c, s = math.cos(th), math.sin(th)
    for t in range(-600, 600, 37):                                 # points of the record's line, flipped -> buffer
        x, y = rho * c - t * s, rho * s + t * c
        if 1 <= x < 2046 and 1 <= y < 1487:
            frames[4, 1488 - int(y), int(x)] = np.nan if t % 2 else np.inf
    recs5 = np.array(rows, _native.RESULT_DTYPE)
    ms = np.stack([masks[i]] * 5)
    with _native.Context(0, 1489, 2048, 8) as ctx:
        out, prof = ctx.measure_trails(frames, recs5, {k: np.stack([v[i]] * 5) for k, v in packed.items()}, rs)
    assert out["status"][1] == T.TOO_SHORT and out["status"][3] == T.NOT_FOUND
    assert out["status"][0] == T.OK and out["status"][4] == T.OK
    check_against_ref(frames, recs5, out, prof, ms)


def test_lsst_size_frames_equal_the_restatement():
    from lfd_amd import _native, synth
    pb, pd, prs = params()
    frames, cats = zip(*[synth.make_frame(k, shape=synth.LSST_SHAPE)[:2] for k in (1, 2, 3, 5)])
    fr = np.stack(frames)
    packed = synth.pack_catalogs(list(cats))
    rs = rs_struct(prs)
    with _native.Context(0, *synth.LSST_SHAPE, 4) as ctx:
        recs = ctx.detect_batch(fr, pb, pd, packed, rs)
        masks = star_masks(ctx, len(fr), synth.LSST_SHAPE, packed, rs)
        out, prof = ctx.measure_trails(fr, recs, packed, rs)
    assert (out["status"] == T.OK).any()
    check_against_ref(fr, recs, out, prof, masks)


def test_single_frame_entry_point():
    from lfd_amd import synth
    from lfd_amd.detecttrails import measure_trail, process_frame_arrays
    pb, pd, prs = params()
    for k in range(8):
        img, cat, truth = synth.make_frame(k)
        det, res, rec = process_frame_arrays(img, cat, "r", pb, pd, prs)
        if not det:
            continue
        o, p = measure_trail(img, rec, cat, "r", prs)
        packed = synth.pack_catalogs([cat])
        from lfd_amd import _native
        with _native.Context(0, 1489, 2048, 2) as ctx:
            m = star_masks(ctx, 1, img.shape, packed, rs_struct(prs))[0]
        r, pr = T.measure(img, rec["rho"], rec["theta"], star_mask=m)
        assert same(o, p, r, pr) is None
        return
    pytest.fail("no detection among the first frames")


# ---- DetectTrails(trail_profiles=True): profiles.txt --------------------------------------------------------------------------
def boss_tree(root, n=6, bz2_all=False):
    from lfd_amd import synth
    frames, cats = zip(*[synth.make_frame(40 + k)[:2] for k in range(n)])
    synth.write_boss_tree(root, list(frames), list(cats), field0=100, bz2_all=bz2_all)
    return frames, cats


def parse_profiles(path):
    out = {}
    for line in open(path):
        f = line.split()
        if f:
            out[tuple(f[:4])] = np.array([float(x) for x in f[4:]])
    return out


def same_values(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def expected_profiles(frames, cats):
    """rows the restatement gives for the tree's frames: records from detect_batch, star squares from remove_stars"""
    from lfd_amd import _native, synth
    pb, pd, prs = params()
    rs = rs_struct(prs)
    out = {}
    with _native.Context(0, *synth.SDSS_SHAPE, 8) as ctx:
        for k, (img, cat) in enumerate(zip(frames, cats)):
            packed = synth.pack_catalogs([cat])
            rec = ctx.detect_batch(img.copy()[None], pb, pd, packed, rs)[0]
            if not rec["found"]:
                continue
            m = star_masks(ctx, 1, img.shape, packed, rs)[0]
            r, p = T.measure(img, rec["rho"], rec["theta"], star_mask=m)
            out[("94", "1", "r", str(100 + k))] = np.array([float(r[f]) for f in T.FIELDS] + [float(v) for v in p])
    return out


@pytest.mark.parametrize("batch", [1, 4])
def test_detecttrails_profiles_rows_equal_the_restatement(tmp_path, batch):
    from lfd_amd.detecttrails import DetectTrails
    frames, cats = boss_tree(tmp_path / "boss")
    want = expected_profiles(frames, cats)
    assert len(want) >= 2
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir()
    off.mkdir()
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(on), trail_profiles=True)
    dt.process(batch=batch)
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=batch)
    assert open(on / "results.txt", "rb").read() == open(off / "results.txt", "rb").read()
    assert not os.path.exists(off / "profiles.txt")
    got = parse_profiles(dt.profiles)
    assert list(got) == [tuple(l.split()[:4]) for l in open(on / "results.txt") if l.strip()]   # one row per results row, in order
    assert sorted(got) == sorted(want)
    for key in want:
        assert same_values(got[key], want[key]), key
    assert open(on / "errors.txt").read() == open(off / "errors.txt").read()


def test_bz2_tree_and_jobs_give_the_same_profiles(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    from lfd_amd.jobs import Jobs
    plain, packed = tmp_path / "plain", tmp_path / "bz2"
    boss_tree(plain / "boss")
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain), trail_profiles=True).process(batch=4)
    want = open(plain / "profiles.txt", "rb").read()
    assert want.count(b"\n") >= 2
    boss_tree(packed / "boss", bz2_all=True)                      # decompressed on the device, measured there
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(packed), trail_profiles=True).process(batch=4)
    assert open(packed / "profiles.txt", "rb").read() == want
    jobs = tmp_path / "jobs"
    jobs.mkdir()
    results, _ = Jobs(2, devices=[0, 0], run=94, camcol=1, filter="r", savepath=str(jobs), trail_profiles=True).launch(batch=4, timeout=600)
    assert open(jobs / "profiles.txt", "rb").read() == want
    assert not os.path.exists(str(jobs / "profiles.txt") + ".rank0")
    assert open(results, "rb").read() == open(packed / "results.txt", "rb").read()
