"""DetectTrails(light_curves=True) end to end on synthetic trees: lightcurves.txt and lightcurve_summary.txt hold, for every
results.txt row and every found faint line, exactly the rows the restatement (tests/lc_ref.py) gives on the segments written to
masks.txt; every other output does not change with the option; two ranks' files concatenate to the one-process files; a
resumed run continues where the marks stop."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (512, 768)
FIELD0 = 100
N_FIELDS = 7


def read(path):
    with open(path, "rb") as f:
        return f.read()


def lines(path):
    return [ln.rstrip("\n") for ln in open(path) if ln.strip()]


def detect_tree(root):
    """seven plain frame files with their catalogues -> the frames by field"""
    from lfd_amd import synth
    made = [synth.make_portable_frame(k, SHAPE) for k in range(N_FIELDS)]
    synth.write_boss_tree(root, [m[0] for m in made], [m[1] for m in made], field0=FIELD0, filter="r")
    return {FIELD0 + k: made[k][0] for k in range(N_FIELDS)}


def expected(frames, mask_rows, **params):
    """the two files' rows for the segments of masks.txt (frames in order, ``line`` counting within a frame and source)"""
    from lfd_amd import lightcurve
    rows, summary = [], []
    for r in mask_rows:
        seg = lightcurve.segments([(0, r["x1"], r["y1"], r["x2"], r["y2"], r["half"])])
        rec, sec = LR.light_curves(frames[r["field"]], seg, sigma=0.025, **params)
        key = (r["run"], r["camcol"], r["filter"], r["field"])
        rows += lightcurve.format_rows(key, r["source"], r["line"], rec[0], sec[0])
        summary.append(lightcurve.format_summary_row(key, r["source"], r["line"], rec[0]))
    return rows, summary


# (the synthetic streaks peak at 0.2 and 5: far above the default clip of 0.125, which is the faint-trail searches' star cut)
@pytest.mark.parametrize("lc_params", [{}, {"clip": 16.0}, {"sec_len": 48.0, "min_core": 8, "clip": 16.0}], ids=["defaults", "clip16", "sec48"])
def test_rows_equal_the_restatement_and_nothing_else_changes(tmp_path, lc_params):
    from lfd_amd import lightcurve, masks
    from lfd_amd.detecttrails import DetectTrails
    frames = detect_tree(tmp_path)
    plain, with_lc = tmp_path / "plain", tmp_path / "lc"
    plain.mkdir()
    with_lc.mkdir()
    kw = dict(run=94, camcol=1, filter="r", trail_profiles=True, trail_masks=True)
    DetectTrails(savepath=str(plain), **kw).process(batch=4)
    dt = DetectTrails(savepath=str(with_lc), light_curves=True, lc_params=lc_params, **kw)
    assert dt.lightcurves_file == str(with_lc / "lightcurves.txt") and dt.lightcurve_summary_file == str(with_lc / "lightcurve_summary.txt")
    dt.process(batch=4)
    for name in ("results.txt", "profiles.txt", "errors.txt", "masks.txt"):
        assert read(with_lc / name) == read(plain / name), name
    assert not os.path.exists(plain / "lightcurves.txt") and not os.path.exists(plain / "lightcurve_summary.txt")
    mrows = masks.read_masks(dt.masks_file)
    assert len(mrows) >= 2 and all(r["source"] == "detect" for r in mrows)
    want_rows, want_summary = expected(frames, mrows, **lc_params)
    assert lines(dt.lightcurve_summary_file) == want_summary
    assert lines(dt.lightcurves_file) == want_rows and len(want_rows) > len(want_summary)
    got = lightcurve.read_summary(dt.lightcurve_summary_file)
    assert [(r["field"], r["source"], r["line"]) for r in got] == [(r["field"], "detect", 0) for r in mrows]      # results.txt's order
    if "clip" in lc_params:
        assert any(r["status"] == LR.OK and r["n_ok"] >= 4 and r["mean_rate"] > 10 * r["mean_rate_err"] for r in got)
    sec = lightcurve.read_lightcurves(dt.lightcurves_file)
    assert all(r["status"] in (LR.SEC_OK, LR.SEC_LOW) and r["n_geom"] > 0 for r in sec)
    # a bad parameter is refused at construction
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(with_lc), light_curves=True, lc_params={"sec_len": 4.0}, **kw)
    with pytest.raises(TypeError):
        DetectTrails(savepath=str(with_lc), light_curves=True, lc_params={"no_such": 1}, **kw)


def test_found_faint_lines_get_radon_rows(tmp_path):
    """the three-frame tree of test_gpu_masks_dropin: field 101 carries two faint trails and no detection, field 102 a bright one"""
    import inject_ref as IR
    from lfd_amd import inject as I, lightcurve, masks, synth
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
    plain, with_lc = tmp_path / "plain", tmp_path / "lc"
    plain.mkdir()
    with_lc.mkdir()
    DetectTrails(savepath=str(plain), **kw).process(batch=4)
    dt = DetectTrails(savepath=str(with_lc), light_curves=True, **kw)
    dt.process(batch=4)
    for name in ("results.txt", "errors.txt", "radon.txt", "radon_segments.txt", "radon_profiles.txt", "masks.txt"):
        assert read(with_lc / name) == read(plain / name), name
    mrows = masks.read_masks(dt.masks_file)
    assert [(r["field"], r["source"], r["line"]) for r in mrows] == [(101, "radon", 0), (101, "radon", 1), (102, "detect", 0)]
    want_rows, want_summary = expected({FIELD0 + k: frames[k] for k in range(3)}, mrows)
    assert lines(dt.lightcurve_summary_file) == want_summary
    assert lines(dt.lightcurves_file) == want_rows
    got = lightcurve.read_summary(dt.lightcurve_summary_file)
    assert [r["status"] for r in got[:2]] == [LR.OK] * 2 and len(got) == 3
    assert abs(got[0]["mean_rate"] - 0.02 * 2.0 * math.sqrt(2.0 * math.pi)) < 5 * got[0]["mean_rate_err"]     # the peak-0.02 trail


def test_two_ranks_equal_one_process_and_a_resume_continues(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    detect_tree(tmp_path)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    kw = dict(run=94, camcol=1, filter="r", light_curves=True)
    DetectTrails(savepath=str(one), **kw).process(batch=4)
    for r in (0, 1):
        DetectTrails(savepath=str(two), **kw).process(batch=2, rank=r, world_size=2)
    for name in ("lightcurves.txt", "lightcurve_summary.txt", "results.txt"):
        whole = read(one / name)
        assert whole and read(two / (name + ".rank0")) + read(two / (name + ".rank1")) == whole, name
    # the option is off by default
    off = tmp_path / "off"
    off.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=4)
    assert not os.path.exists(off / "lightcurves.txt") and not os.path.exists(off / "lightcurve_summary.txt")
    assert read(off / "results.txt") == read(one / "results.txt") and read(off / "errors.txt") == read(one / "errors.txt")
    # a complete run resumed appends nothing; with the marks of the last three frames taken away it does those again, and only those
    before = {name: read(one / name) for name in ("lightcurves.txt", "lightcurve_summary.txt", "results.txt")}
    dt = DetectTrails(savepath=str(one), **kw)
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS
    assert all(read(one / name) == data for name, data in before.items())
    marks = lines(one / "results.txt.progress")
    assert len(marks) == 1 + N_FIELDS
    with open(one / "results.txt.progress", "w") as f:
        f.write("\n".join(marks[:-3]) + "\n")
    redo = {m.split()[3] for m in marks[-3:]}
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS - 3
    for name, data in before.items():
        again = [ln for ln in data.decode().splitlines() if ln.split()[3] in redo]
        assert read(one / name).decode().splitlines() == data.decode().splitlines() + again, name
    assert any(ln.split()[3] in redo for ln in before["lightcurve_summary.txt"].decode().splitlines())
