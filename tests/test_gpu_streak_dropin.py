"""DetectTrails(streaks=True) end to end on a small synthetic selection: the streaks.txt rows against the numpy restatement
(tests/streak_ref.py) on the frames as the detect call leaves them (the oracle's remove_stars), every other output byte for
byte what a run without the option writes, two ranks' files that concatenate to the one run's, a resumed run, and the
frame-at-a-time path."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streak_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (372, 512)
N_FIELDS = 4
KW = {"run": 94, "camcol": 1, "filter": "r"}


def make_tree(tmp_path):
    """fields 100 .. 103: noise; one 64 px streak; the trail the detector finds; two streaks"""
    import inject_ref as IR
    from lfd_amd import inject as I, synth
    rng = np.random.default_rng(31)
    frames = rng.normal(0, 0.025, (N_FIELDS, *SHAPE)).astype(np.float32)
    short = np.zeros(3, IR.TRAIL_DTYPE)
    for k, (frame, deg, x0, y0) in enumerate(((1, 115.0, 250.0, 180.0), (3, 30.0, 120.0, 100.0), (3, 100.0, 380.0, 260.0))):
        th = math.radians(deg)
        t = -x0 * math.sin(th) + y0 * math.cos(th)
        short[k] = (frame, 0, x0 * math.cos(th) + y0 * math.sin(th), th, t - 32.0, t + 32.0, 0.06)
    table, step = I.gaussian_table(1.5)
    IR.inject(frames, short, I.normalise_peak(table).astype(np.float32), step)
    th = math.radians(115.0)
    bright = np.zeros(1, IR.TRAIL_DTYPE)
    bright[0] = (2, 0, 256 * math.cos(th) + 186 * math.sin(th), th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, bright, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, SHAPE)[1] for k in range(N_FIELDS)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r")
    return frames, cats


def restated_rows(frames, cats, **params):
    """the rows streaks.txt has to hold: the restatement on every frame without its catalogue's stars"""
    from lfd_amd import streaks
    from lfd_amd.detecttrails import default_params
    from oracle import lfd_oracle as O
    prs = {k: v for k, v in default_params()[2].items() if k != "debug"}
    rows = []
    for i in range(N_FIELDS):
        f = frames[i].copy()
        O.remove_stars(f, cats[i], O.rs_params("r", **prs))
        recs, n = S.rounds(f, 0.025, **params)
        rows += [streaks.format_row((94, 1, "r", 100 + i), k, recs[k]) for k in range(n)]
    return rows


def lines_of(path):
    return [ln for ln in open(path).read().splitlines() if ln.strip()]


def test_dropin_writes_streaks_and_leaves_the_other_files(tmp_path):
    from lfd_amd import streaks
    from lfd_amd.detecttrails import DetectTrails
    frames, cats = make_tree(tmp_path)
    off, on, par = tmp_path / "off", tmp_path / "on", tmp_path / "par"
    for d in (off, on, par):
        d.mkdir()
    a = DetectTrails(savepath=str(off), **KW)
    a.process(batch=4)
    b = DetectTrails(savepath=str(on), streaks=True, **KW)
    b.process(batch=4)
    assert not a.streaks and not os.path.exists(a.streaks_file) and b.streaks_file == str(on / "streaks.txt")
    for name in ("results", "errors"):
        assert open(getattr(a, name)).read() == open(getattr(b, name)).read(), name
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["streaks.txt"])
    for name in os.listdir(off):                                      # every other output, byte for byte
        if os.path.isfile(off / name):
            assert open(off / name, "rb").read() == open(on / name, "rb").read(), name
    assert lines_of(a.results) and open(a.errors).read() == ""
    want = restated_rows(frames, cats)
    rows = lines_of(b.streaks_file)
    print("streaks.txt", rows)
    assert rows == want
    got = streaks.read_streaks(b.streaks_file)
    fields = [r["field"] for r in got]
    assert 101 in fields and fields.count(103) >= 2 and 100 not in fields
    assert all(len(ln.split()) == len(streaks.STREAK_COLUMNS) for ln in rows)
    # other parameters reach the call
    p = {"length": 16, "max_streaks": 2, "threshold": 9.0}
    c = DetectTrails(savepath=str(par), streaks=True, streaks_params=p, **KW)
    c.process(batch=4)
    assert lines_of(c.streaks_file) == restated_rows(frames, cats, **p)
    assert open(c.results).read() == open(a.results).read()


def test_ranks_resume_and_the_frame_at_a_time_path(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    frames, cats = make_tree(tmp_path)
    want = restated_rows(frames, cats)
    one, two, single = tmp_path / "one", tmp_path / "two", tmp_path / "single"
    for d in (one, two, single):
        d.mkdir()
    dt = DetectTrails(savepath=str(one), streaks=True, **KW)
    dt.process(batch=4)
    assert lines_of(dt.streaks_file) == want
    results_one = open(dt.results).read()                             # (the cut-short run below appends to this file again)
    # two ranks: their files, in rank order, are the one run's
    for rank in (0, 1):
        DetectTrails(savepath=str(two), streaks=True, **KW).process(batch=2, rank=rank, world_size=2)
    for name in ("streaks.txt", "results.txt"):
        assert lines_of(two / (name + ".rank0")) + lines_of(two / (name + ".rank1")) == lines_of(one / name), name
    # resume: a finished run adds nothing
    again = DetectTrails(savepath=str(one), streaks=True, **KW)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == N_FIELDS and lines_of(dt.streaks_file) == want
    # a run that stopped after its first field adds the rest
    progress = dt.results + ".progress"
    marks = lines_of(progress)
    open(progress, "w").write("\n".join(marks[:2]) + "\n")
    first = [ln for ln in want if ln.split()[3] == marks[1].split()[3]]
    open(dt.streaks_file, "w").write("".join(ln + "\n" for ln in first))
    again = DetectTrails(savepath=str(one), streaks=True, **KW)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 1 and sorted(lines_of(dt.streaks_file)) == sorted(want)
    # frame at a time: the same rows
    s = DetectTrails(savepath=str(single), streaks=True, **KW)
    s.process(batch=1)
    assert lines_of(s.streaks_file) == want
    assert open(s.results).read() == results_one
