"""``DetectTrails(previews=...)`` over a small tree: the PNG files decode to the overlay of the restatement's preview of the
frames as loaded (tests/preview_ref.py), their names are the image checker's and parse back to the frames' ids, previews.txt
carries the restatement's records, every other file stays byte for byte what it is without the option, and a resumed run leaves
the first run's files alone."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (372, 512)
N_FIELDS = 4
KW = dict(run=94, camcol=1, filter="r")


def read(path):
    return open(path, "rb").read() if os.path.exists(path) else b""


def lines(path):
    return read(path).decode().splitlines()


@functools.lru_cache(maxsize=None)
def case():
    """4 fields of the recipe with their photoObj catalogues (bright streak, none, bright, dim) and the restatement's previews of
    them at the defaults and at bin 8 with given limits"""
    from lfd_amd import previews, synth
    made = [synth.make_frame(k, shape=SHAPE) for k in (4, 5, 8, 9)]
    frames = np.stack([m[0] for m in made])
    frames.setflags(write=False)
    return frames, [m[1] for m in made], R.frame_previews(frames, previews.lut("asinh")), \
        R.frame_previews(frames, previews.lut("sqrt"), bin=8, mode=R.GIVEN, limits=np.array([-0.05, 0.3]))


def tree(tmp_path):
    from lfd_amd import synth
    frames, cats = case()[:2]
    synth.write_boss_tree(tmp_path / "tree", list(frames), cats, field0=100, filter="r")


def run(tmp_path, name, batch=4, **kw):
    from lfd_amd.detecttrails import DetectTrails
    out = tmp_path / name
    out.mkdir(exist_ok=True)
    dt = DetectTrails(savepath=str(out), **KW, **kw)
    dt.process(batch=batch)
    return dt, out


def check_pictures(dt, out, want, bin, fields, segments_of, **draw):
    """previews.txt and the PNG files of `fields` against the restatement `want` = (images, cells, records)"""
    from lfd_amd import previews
    from lfd_amd.detecttrails import debugio
    rows = previews.read_previews(dt.previews_file)
    assert [r["field"] for r in rows] == fields
    assert sorted(os.listdir(dt.preview_dir)) == sorted(r["file"] for r in rows)
    for r in rows:
        i = r["field"] - 100
        assert previews.parse_filename(r["file"]) == (94, 1, "r", r["field"], "fits.png")
        assert r["file"] == "frame-r-000094-1-%04d.fits.png" % r["field"]
        rec = want[2][i]
        assert lines(dt.previews_file)[rows.index(r)] == previews.format_row((94, 1, "r", r["field"]), bin, rec, r["file"])
        assert (r["status"], r["bin"], r["n_cells"], r["n_empty"]) == (int(rec["status"]), bin, int(rec["n_cells"]), int(rec["n_empty"]))
        assert r["lo"] == float(rec["lo_f"]) and r["hi"] == float(rec["hi_f"])
        png = debugio.read_png(os.path.join(dt.preview_dir, r["file"]))
        expect = previews.overlay(want[0][i], segments_of(r["field"]), bin, **draw)
        assert png.shape == expect.shape and png.tobytes() == expect.tobytes(), r["field"]


def test_pictures_rows_and_nothing_else_changes(tmp_path):
    from lfd_amd import masks, results as results_mod
    tree(tmp_path)
    base, b_out = run(tmp_path, "base")
    found = results_mod.read_results(base.results)
    by_field = {int(r["field"]): r for r in found}
    assert len(found) >= 2 and not os.path.exists(b_out / "previews.txt") and not os.path.exists(b_out / "previews")

    def segments_of(field):
        r = by_field.get(field)
        return masks.segments([] if r is None else [(0, r["x1"], r["y1"], r["x2"], r["y2"], masks.half_width(float("nan")))])

    for batch in (1, 4):
        dt, out = run(tmp_path, "det%d" % batch, batch=batch, previews="detections")
        assert dt.previews_file == str(out / "previews.txt") and dt.preview_dir == str(out / "previews")
        check_pictures(dt, out, case()[2], 4, sorted(by_field), segments_of)
        for name in ("results.txt", "errors.txt", "results.txt.progress"):
            assert read(out / name) == read(b_out / name), (batch, name)
        assert sorted(os.listdir(out)) == sorted(os.listdir(b_out) + ["previews.txt", "previews"])
        dt, out = run(tmp_path, "all%d" % batch, batch=batch, previews="all")
        check_pictures(dt, out, case()[2], 4, list(range(100, 100 + N_FIELDS)), segments_of)
        assert read(out / "results.txt") == read(b_out / "results.txt") and read(out / "errors.txt") == read(b_out / "errors.txt")
    # the parameters reach the library and the overlay; bad ones are refused at construction
    params = {"bin": 8, "mode": "given", "limits": (-0.05, 0.3), "kind": "sqrt", "color": (0, 255, 0), "thick": 2.0}
    dt, out = run(tmp_path, "given", previews="all", preview_params=params)
    check_pictures(dt, out, case()[3], 8, list(range(100, 100 + N_FIELDS)), segments_of, color=(0, 255, 0), thick=2.0)
    from lfd_amd.detecttrails import DetectTrails
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(out), previews="some", **KW)
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(out), previews="all", preview_params={"bin": 3}, **KW)
    with pytest.raises(TypeError):
        DetectTrails(savepath=str(out), previews="all", preview_params={"binning": 4}, **KW)


def test_a_resumed_run_leaves_the_first_runs_files_alone(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    tree(tmp_path)
    dt, out = run(tmp_path, "one", previews="all")
    rows = lines(dt.previews_file)
    names = sorted(os.listdir(dt.preview_dir))
    assert len(rows) == len(names) == N_FIELDS
    stamp = {n: (os.stat(os.path.join(dt.preview_dir, n)).st_mtime_ns, read(os.path.join(dt.preview_dir, n))) for n in names}
    os.utime(os.path.join(dt.preview_dir, names[0]), ns=(1, 1))              # a file the resumed runs must not write again
    again = DetectTrails(savepath=str(out), previews="all", **KW)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == N_FIELDS and lines(dt.previews_file) == rows
    assert os.stat(os.path.join(dt.preview_dir, names[0])).st_mtime_ns == 1
    # with the mark of the last frame taken away, only that frame is done, and written, again
    marks = lines(out / "results.txt.progress")
    with open(out / "results.txt.progress", "w") as f:
        f.write("\n".join(marks[:-1]) + "\n")
    for n in names[:-1]:
        os.utime(os.path.join(dt.preview_dir, n), ns=(1, 1))
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == N_FIELDS - 1 and lines(dt.previews_file) == rows + rows[-1:]
    for n in names[:-1]:
        assert os.stat(os.path.join(dt.preview_dir, n)).st_mtime_ns == 1, n
    assert sorted(os.listdir(dt.preview_dir)) == names
    assert all(read(os.path.join(dt.preview_dir, n)) == stamp[n][1] for n in names)


def test_the_trails_of_the_later_rounds_are_drawn_too(tmp_path):
    """with max_trails the picture of a frame carries every found trail of trails.txt: its own row's line and the later rounds'"""
    from lfd_amd import masks, previews, results as results_mod, rounds
    from lfd_amd.detecttrails import debugio
    tree(tmp_path)
    dt, out = run(tmp_path, "rounds", previews="detections", max_trails=3)
    res = {int(r["field"]): r for r in results_mod.read_results(dt.results)}
    later = {}
    for r in rounds.read_trails(dt.trails_file):
        if r["round"] >= 1:
            later.setdefault(r["field"], []).append(r)
    half = masks.half_width(float("nan"))
    rows = previews.read_previews(dt.previews_file)
    assert [r["field"] for r in rows] == sorted(res)
    for r in rows:
        f = r["field"]
        segs = masks.segments([(0, s["x1"], s["y1"], s["x2"], s["y2"], half) for s in [res[f]] + later.get(f, [])])
        png = debugio.read_png(os.path.join(dt.preview_dir, r["file"]))
        assert png.tobytes() == previews.overlay(case()[2][0][f - 100], segs, 4).tobytes(), f
