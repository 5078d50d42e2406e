"""DetectTrails(trail_strips=True) end to end on synthetic trees: strips.txt holds, for every results.txt row and every found faint
line, exactly the rows the restatement (tests/strip_ref.py) gives on the segments written to masks.txt, widened by the wing; each
segment has its .npz and .png; every other output does not change with the option; two ranks' files concatenate to the
one-process files."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strip_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (512, 768)
FIELD0 = 100
N_FIELDS = 5


def read(path):
    with open(path, "rb") as f:
        return f.read()


def lines(path):
    return [ln.rstrip("\n") for ln in open(path) if ln.strip()]


def detect_tree(root):
    """a handful of plain frame files with their catalogues -> the frames by field"""
    from lfd_amd import synth
    made = [synth.make_portable_frame(k, SHAPE) for k in range(N_FIELDS)]
    synth.write_boss_tree(root, [m[0] for m in made], [m[1] for m in made], field0=FIELD0, filter="r")
    return {FIELD0 + k: made[k][0] for k in range(N_FIELDS)}


def expected(frames, mask_rows, **params):
    """strips.txt's rows for the segments of masks.txt (frames in order, ``line`` counting within a frame and source), and per
    segment (file stem, restatement's record, cells)"""
    from lfd_amd import strips
    rows, per_seg = [], []
    wing = params.get("wing", 6.0)
    for r in mask_rows:
        seg = strips.segments([(0, r["x1"], r["y1"], r["x2"], r["y2"], r["half"] + wing)])
        rec, sec, cel = SR.trail_strips(frames[r["field"]], seg, sigma=0.025, max_sections=1024, **params)
        key = (r["run"], r["camcol"], r["filter"], r["field"])
        rows += strips.format_rows(key, r["source"], r["line"], rec[0], sec[0])
        per_seg.append(("strip-%s-%s-%s-%s-%s%d" % (*key, r["source"], r["line"]), rec[0], cel[0], seg[0]))
    return rows, per_seg


def check_maps(strips_dir, per_seg):
    assert sorted(os.listdir(strips_dir)) == sorted(stem + ext for stem, _, _, _ in per_seg for ext in (".npz", ".png"))
    for stem, rec, cel, seg in per_seg:
        ns, no = int(rec["n_sec"]), int(rec["n_off"])
        z = np.load(os.path.join(strips_dir, stem + ".npz"))
        assert z["mean"].shape == (ns, no) and z["mean"].dtype == np.float32
        assert np.array_equal(z["mean"].view(np.uint32), SR.mean_map(cel[:ns * no]).reshape(ns, no).view(np.uint32))
        assert np.array_equal(z["n"], cel[:ns * no]["n"].reshape(ns, no)) and np.array_equal(z["n_geom"], cel[:ns * no]["n_geom"].reshape(ns, no))
        assert z["segment"].tolist() == [float(seg[k]) for k in ("x1", "y1", "x2", "y2", "half")]
        assert read(os.path.join(strips_dir, stem + ".png"))[:8] == b"\x89PNG\r\n\x1a\n"


# (the synthetic streaks peak at 0.2 and 5: far above the default clip of 0.125, which is the faint-trail searches' star cut)
@pytest.mark.parametrize("strips_params", [{}, {"clip": 16.0, "sec_len": 32.0, "step": 0.5, "wing": 4.0}], ids=["defaults", "clip16"])
def test_rows_and_maps_equal_the_restatement_and_nothing_else_changes(tmp_path, strips_params):
    from lfd_amd import masks, strips
    from lfd_amd.detecttrails import DetectTrails
    frames = detect_tree(tmp_path)
    plain, off, on = tmp_path / "plain", tmp_path / "off", tmp_path / "on"
    for d in (plain, off, on):
        d.mkdir()
    kw = dict(run=94, camcol=1, filter="r", trail_profiles=True, trail_masks=True, light_curves=True)
    DetectTrails(savepath=str(plain), **kw).process(batch=4)
    DetectTrails(savepath=str(off), trail_strips=False, **kw).process(batch=4)
    dt = DetectTrails(savepath=str(on), trail_strips=True, strips_params=strips_params, strips_dir=str(on / "maps"), **kw)
    assert dt.strips_file == str(on / "strips.txt")
    dt.process(batch=4)
    for name in ("results.txt", "profiles.txt", "errors.txt", "masks.txt", "lightcurves.txt", "lightcurve_summary.txt"):
        assert read(on / name) == read(plain / name) == read(off / name), name
    assert not os.path.exists(plain / "strips.txt") and not os.path.exists(off / "strips.txt")
    assert sorted(os.listdir(off)) == sorted(os.listdir(plain))
    mrows = masks.read_masks(dt.masks_file)
    assert len(mrows) >= 2 and all(r["source"] == "detect" for r in mrows)
    want_rows, per_seg = expected(frames, mrows, **strips_params)
    assert lines(dt.strips_file) == want_rows and len(want_rows) > len(mrows)
    check_maps(on / "maps", per_seg)
    got = strips.read_strips(dt.strips_file)
    assert all(r["status"] in (SR.SEC_OK, SR.SEC_LOW) for r in got)
    if "clip" in strips_params:
        assert any(r["status"] == SR.SEC_OK and r["rate"] > 10 * r["rate_err"] and abs(r["centre"]) < 2.0 for r in got)
    # the frame-at-a-time loop measures the frame remove_stars has blotted, on the segments of its own masks.txt: the sections and
    # their extents are the restatement's (they depend on the geometry alone), the counts can only be smaller
    single = tmp_path / "single"
    single.mkdir()
    DetectTrails(savepath=str(single), trail_strips=True, strips_params=strips_params, **kw).process(batch=1)
    srows = masks.read_masks(str(single / "masks.txt"))
    want_single = [ln.split() for ln in expected(frames, srows, **strips_params)[0]]
    got_single = [ln.split() for ln in lines(single / "strips.txt")]
    assert len(srows) == len(mrows) and [g[:9] for g in got_single] == [w[:9] for w in want_single]
    assert all(int(g[9]) <= int(w[9]) and int(g[10]) <= int(w[10]) for g, w in zip(got_single, want_single))
    assert read(single / "results.txt") == read(on / "results.txt")
    # a bad parameter is refused at construction
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(on), trail_strips=True, strips_params={"sec_len": 3.0}, **kw)
    with pytest.raises(TypeError):
        DetectTrails(savepath=str(on), trail_strips=True, strips_params={"no_such": 1}, **kw)


def test_found_faint_lines_get_radon_rows(tmp_path):
    """the three-frame tree of test_gpu_masks_dropin: field 101 carries two faint trails and no detection, field 102 a bright one"""
    import inject_ref as IR
    from lfd_amd import inject as I, masks, strips, synth
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
    params = {"sec_len": 32.0}
    dt = DetectTrails(savepath=str(on), trail_strips=True, strips_params=params, strips_dir=str(on / "maps"), **kw)
    dt.process(batch=4)
    for name in ("results.txt", "errors.txt", "radon.txt", "radon_segments.txt", "radon_profiles.txt", "masks.txt"):
        assert read(on / name) == read(plain / name), name
    mrows = masks.read_masks(dt.masks_file)
    assert [(r["field"], r["source"], r["line"]) for r in mrows] == [(101, "radon", 0), (101, "radon", 1), (102, "detect", 0)]
    want_rows, per_seg = expected({FIELD0 + k: frames[k] for k in range(3)}, mrows, **params)
    assert lines(dt.strips_file) == want_rows
    check_maps(on / "maps", per_seg)
    got = [r for r in strips.read_strips(dt.strips_file) if (r["field"], r["line"]) == (101, 0) and r["status"] == SR.SEC_OK]
    assert len(got) >= 6 and sum(r["rate"] for r in got) > 0.0


def test_two_ranks_equal_one_process(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    detect_tree(tmp_path)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    kw = dict(run=94, camcol=1, filter="r", trail_strips=True)
    DetectTrails(savepath=str(one), **kw).process(batch=4)
    for r in (0, 1):
        DetectTrails(savepath=str(two), **kw).process(batch=2, rank=r, world_size=2)
    for name in ("strips.txt", "results.txt"):
        whole = read(one / name)
        assert whole and read(two / (name + ".rank0")) + read(two / (name + ".rank1")) == whole, name      # rows in selection order
    # a complete run resumed appends nothing
    before = read(one / "strips.txt")
    dt = DetectTrails(savepath=str(one), **kw)
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS and read(one / "strips.txt") == before
    # the option is off by default
    off = tmp_path / "off"
    off.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=4)
    assert not os.path.exists(off / "strips.txt") and read(off / "results.txt") == read(one / "results.txt")
