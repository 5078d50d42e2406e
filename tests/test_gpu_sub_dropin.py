"""DetectTrails(subtract_trails=True) end to end on synthetic trees: subtracted.txt holds, for every results.txt row and every
found faint line, exactly the row the restatement (tests/sub_ref.py) gives on the segments written to masks.txt, widened by the
wing; with ``clean_dir`` every changed frame is written, bit for bit the restatement's cleaned frame; every other output does not
change with the option; two ranks' files concatenate to the one-process files."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sub_ref as UR  # noqa: E402
from test_gpu_strips_dropin import FIELD0, N_FIELDS, SHAPE, detect_tree, lines, read  # noqa: E402

pytestmark = pytest.mark.gpu


def expected(frames, mask_rows, **params):
    """subtracted.txt's rows for the segments of masks.txt, and per field (the restatement's cleaned frame, its segments): a
    frame's segments go through one call, in their order"""
    from lfd_amd import subtract
    wing = params.get("wing", 6.0)
    rows, clean = [], {}
    for field in sorted({r["field"] for r in mask_rows}):
        mine = [r for r in mask_rows if r["field"] == field]
        segs = subtract.segments([(0, r["x1"], r["y1"], r["x2"], r["y2"], r["half"] + wing) for r in mine])
        cl, rec, _ = UR.subtract_trails(frames[field], segs, max_sections=1024, **params)
        for r, o in zip(mine, rec):
            rows += subtract.format_rows((r["run"], r["camcol"], r["filter"], r["field"]), r["source"], r["line"], o)
        clean[field] = (cl, segs)
    return rows, clean


def check_clean(clean_dir, key_of, clean):
    assert sorted(os.listdir(clean_dir)) == sorted("clean-%s-%s-%s-%s.npz" % key_of(f) for f in clean)
    for f, (cl, segs) in clean.items():
        z = np.load(os.path.join(clean_dir, "clean-%s-%s-%s-%s.npz" % key_of(f)))
        assert z["frame"].dtype == np.float32 and np.array_equal(z["frame"].view(np.uint32), cl.view(np.uint32)), f
        assert z["segments"].tolist() == [[float(s[k]) for k in ("x1", "y1", "x2", "y2", "half")] for s in segs]


# (the synthetic streaks peak at 0.2 and 5: far above the default clip of 0.125, which is the faint-trail searches' star cut)
@pytest.mark.parametrize("sub_params", [{}, {"clip": 16.0, "sec_len": 16.0, "wing": 4.0, "smooth": 1, "min_sec": 2}], ids=["defaults", "clip16"])
def test_rows_and_frames_equal_the_restatement_and_nothing_else_changes(tmp_path, sub_params):
    from lfd_amd import masks, subtract
    from lfd_amd.detecttrails import DetectTrails
    frames = detect_tree(tmp_path)
    plain, off, on = tmp_path / "plain", tmp_path / "off", tmp_path / "on"
    for d in (plain, off, on):
        d.mkdir()
    kw = dict(run=94, camcol=1, filter="r", trail_profiles=True, trail_masks=True, light_curves=True, trail_strips=True)
    DetectTrails(savepath=str(plain), **kw).process(batch=4)
    DetectTrails(savepath=str(off), subtract_trails=False, **kw).process(batch=4)
    dt = DetectTrails(savepath=str(on), subtract_trails=True, sub_params=sub_params, clean_dir=str(on / "clean"), **kw)
    assert dt.subtracted_file == str(on / "subtracted.txt")
    dt.process(batch=4)
    for name in ("results.txt", "profiles.txt", "errors.txt", "masks.txt", "lightcurves.txt", "lightcurve_summary.txt", "strips.txt"):
        assert read(on / name) == read(plain / name) == read(off / name), name
    assert not os.path.exists(plain / "subtracted.txt") and not os.path.exists(off / "subtracted.txt")
    assert sorted(os.listdir(off)) == sorted(os.listdir(plain))
    assert sorted(os.listdir(on)) == sorted(os.listdir(plain) + ["subtracted.txt", "clean"])
    mrows = masks.read_masks(dt.masks_file)
    assert len(mrows) >= 2 and all(r["source"] == "detect" for r in mrows)
    want_rows, clean = expected(frames, mrows, **sub_params)
    assert lines(dt.subtracted_file) == want_rows and len(want_rows) == len(mrows)
    check_clean(on / "clean", lambda f: (94, 1, "r", f), clean)
    got = subtract.read_subtracted(dt.subtracted_file)
    if "clip" in sub_params:                              # the bright streaks are modelled once the clip lets their pixels in
        assert any(r["status"] == UR.OK and r["n_pix"] > 1000 and r["removed"] > 0 for r in got)
        f = got[0]["field"]
        assert not np.array_equal(clean[f][0], frames[f])
    # the frame-at-a-time loop cleans the frame remove_stars has blotted, on the segments of its own masks.txt: the geometry is
    # the restatement's, and every other output is the batch path's
    single = tmp_path / "single"
    single.mkdir()
    DetectTrails(savepath=str(single), subtract_trails=True, sub_params=sub_params, clean_dir=str(single / "clean"), **kw).process(batch=1)
    want_single = [ln.split() for ln in expected(frames, masks.read_masks(str(single / "masks.txt")), **sub_params)[0]]
    got_single = [ln.split() for ln in lines(single / "subtracted.txt")]
    assert [g[:6] + [g[7]] for g in got_single] == [w[:6] + [w[7]] for w in want_single]       # the key and n_sec
    assert read(single / "results.txt") == read(on / "results.txt")
    assert sorted(os.listdir(single / "clean")) == sorted(os.listdir(on / "clean"))
    # a bad parameter is refused at construction
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(on), subtract_trails=True, sub_params={"sec_len": 3.0}, **kw)
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(on), subtract_trails=True, sub_params={"apply": 0}, **kw)
    with pytest.raises(TypeError):
        DetectTrails(savepath=str(on), subtract_trails=True, sub_params={"no_such": 1}, **kw)


def test_found_faint_lines_get_radon_rows_and_are_taken_out(tmp_path):
    """the three-frame tree of test_gpu_masks_dropin: field 101 carries two faint trails and no detection, field 102 a bright one"""
    import inject_ref as IR
    from lfd_amd import inject as I, masks, subtract, synth
    from lfd_amd.detecttrails import DetectTrails
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (3, *SHAPE)).astype(np.float32)
    tr = np.zeros(3, IR.TRAIL_DTYPE)
    th, th2 = math.radians(115.0), math.radians(30.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    tr[0] = (1, 0, rho, th, -np.inf, np.inf, 0.02)
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    tr[2] = (1, 0, 400 * math.cos(th2) + 240 * math.sin(th2), th2, -np.inf, np.inf, 0.018)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, SHAPE)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=FIELD0, filter="r")
    kw = dict(run=94, camcol=1, filter="r", radon=True, radon_lines=3, radon_profiles=True, trail_masks=True)
    plain, on = tmp_path / "plain", tmp_path / "on"
    plain.mkdir()
    on.mkdir()
    DetectTrails(savepath=str(plain), **kw).process(batch=4)
    dt = DetectTrails(savepath=str(on), subtract_trails=True, clean_dir=str(on / "clean"), **kw)
    dt.process(batch=4)
    for name in ("results.txt", "errors.txt", "radon.txt", "radon_segments.txt", "radon_profiles.txt", "masks.txt"):
        assert read(on / name) == read(plain / name), name
    mrows = masks.read_masks(dt.masks_file)
    assert [(r["field"], r["source"], r["line"]) for r in mrows] == [(101, "radon", 0), (101, "radon", 1), (102, "detect", 0)]
    want_rows, clean = expected({FIELD0 + k: frames[k] for k in range(3)}, mrows)
    assert lines(dt.subtracted_file) == want_rows
    check_clean(on / "clean", lambda f: (94, 1, "r", f), clean)
    got = [r for r in subtract.read_subtracted(dt.subtracted_file) if r["field"] == 101]
    assert len(got) == 2 and all(r["status"] == UR.OK and r["removed"] > 0.0 and r["n_pix"] > 3000 for r in got)


def test_two_ranks_equal_one_process(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    detect_tree(tmp_path)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    kw = dict(run=94, camcol=1, filter="r", subtract_trails=True, sub_params={"clip": 16.0})
    DetectTrails(savepath=str(one), **kw).process(batch=4)
    for r in (0, 1):
        DetectTrails(savepath=str(two), **kw).process(batch=2, rank=r, world_size=2)
    for name in ("subtracted.txt", "results.txt"):
        whole = read(one / name)
        assert whole and read(two / (name + ".rank0")) + read(two / (name + ".rank1")) == whole, name      # rows in selection order
    # a complete run resumed appends nothing
    before = read(one / "subtracted.txt")
    dt = DetectTrails(savepath=str(one), **kw)
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS and read(one / "subtracted.txt") == before
    # the option is off by default
    off = tmp_path / "off"
    off.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=4)
    assert not os.path.exists(off / "subtracted.txt") and read(off / "results.txt") == read(one / "results.txt")
