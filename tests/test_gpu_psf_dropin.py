"""``DetectTrails(seeing=True)`` over a small tree: seeing.txt carries the restatement's rows (tests/psf_ref.py after
tests/stars_ref.py), every other file stays byte for byte what it is without the option, the defocus fits get their frame's
seeing (and stay free for a frame with too few stars), two ranks and a resumed run give the same rows, and the rows do not
depend on ``find_stars``."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (372, 512)
N_FIELDS = 6
FEW = 0                                                    # the field with too few stars for SEE (10 used), and a bright streak
SEE = {"seeing": True, "seeing_params": {"min_stars": 11}}
KW = dict(run=94, camcol=1, filter="r")


def read(path):
    return open(path, "rb").read() if os.path.exists(path) else b""


def lines(path):
    return read(path).decode().splitlines()


@functools.lru_cache(maxsize=None)
def case():
    """6 fields of the recipe with their photoObj catalogues (bright, none, bright, dim, bright, bright streaks); the
    restatement's seeing.txt rows of them with min_stars = 11, which the first field misses by one star"""
    from lfd_amd import defocus, psf, synth
    made = [synth.make_frame(k, shape=SHAPE) for k in (4, 5, 8, 9, 10)] + [synth.make_frame(6, shape=SHAPE)]
    frames = np.stack([m[0] for m in made])
    cats = [m[1] for m in made]
    _, fr, _, _ = R.measure_seeing(frames, 0.025, min_stars=11)
    assert fr["status"].tolist() == [R.SEEING_FEW] + [R.SEEING_OK] * 5 and fr["n_used"][0] == 10
    grid = defocus.default_params()["seeings"]
    see = psf.to_bank_seeing(fr["fwhm_px"], 0.396, 7, grid)
    see[FEW] = np.nan
    rows = [psf.format_row((94, 1, "r", 100 + i), fr[i], 0.396, see[i]) for i in range(N_FIELDS)]
    frames.setflags(write=False)
    return frames, cats, fr, see, rows, grid


def tree(tmp_path, photoobj=True):
    from lfd_amd import synth
    from lfd_amd.detecttrails import sdssfiles
    frames, cats = case()[:2]
    synth.write_boss_tree(tmp_path / "tree", list(frames), cats, field0=100, filter="r")
    if not photoobj:
        for f in range(100, 100 + N_FIELDS):
            os.remove(sdssfiles.filename("photoObj", run=94, camcol=1, field=f))


def run(tmp_path, name, batch=4, **kw):
    from lfd_amd.detecttrails import DetectTrails
    out = tmp_path / name
    out.mkdir(exist_ok=True)
    dt = DetectTrails(savepath=str(out), **KW, **kw)
    dt.process(batch=batch)
    return dt, out


def test_rows_equal_the_restatement_and_nothing_else_changes(tmp_path):
    from lfd_amd import psf
    rows = case()[4]
    tree(tmp_path)
    base, b_out = run(tmp_path, "base", trail_profiles=True)
    assert len(lines(base.results)) >= 3 and not os.path.exists(b_out / "seeing.txt")
    for batch in (1, 4):
        dt, out = run(tmp_path, "see%d" % batch, batch=batch, trail_profiles=True, **SEE)
        assert dt.seeing_file == str(out / "seeing.txt") and lines(dt.seeing_file) == rows, batch
        for name in ("results.txt", "errors.txt", "profiles.txt"):
            assert read(out / name) == read(b_out / name), (batch, name)
        assert sorted(os.listdir(out)) == sorted(os.listdir(b_out) + ["seeing.txt"])
    got = psf.read_seeing(dt.seeing_file)
    assert [r["field"] for r in got] == list(range(100, 106)) and got[FEW]["status"] == psf.SEEING_FEW and np.isnan(got[FEW]["seeing_arcsec"])
    # other parameters reach the library, and bad ones are refused at construction
    dt, out = run(tmp_path, "win5", trail_profiles=True, seeing=True, seeing_params={"win": 5, "min_stars": 1})
    assert lines(dt.seeing_file) != rows and [r["status"] for r in psf.read_seeing(dt.seeing_file)] == [0] * N_FIELDS
    from lfd_amd.detecttrails import DetectTrails
    with pytest.raises(ValueError):
        DetectTrails(savepath=str(out), seeing=True, seeing_params={"win": 17}, **KW)
    with pytest.raises(TypeError):
        DetectTrails(savepath=str(out), seeing=True, seeing_params={"radius": 3}, **KW)


def test_the_defocus_fits_get_their_frames_seeing(tmp_path):
    from lfd_amd import defocus
    _, _, fr, see, rows, grid = case()
    tree(tmp_path)
    free, f_out = run(tmp_path, "free", defocus=True)
    pinned, p_out = run(tmp_path, "pinned", defocus=True, **SEE)
    assert lines(pinned.seeing_file) == rows
    for name in ("results.txt", "errors.txt", "profiles.txt"):
        assert read(p_out / name) == read(f_out / name), name
    a, b = defocus.read_defocus(free.defocus_file), defocus.read_defocus(pinned.defocus_file)
    assert len(a) == len(b) >= 3 and [r["field"] for r in a] == [r["field"] for r in b]
    assert 100 + FEW in [r["field"] for r in b]
    checked = 0
    for ra, rb, la, lb in zip(a, b, lines(free.defocus_file), lines(pinned.defocus_file)):
        i = rb["field"] - 100
        if i == FEW:
            assert la == lb                                # too few stars: the fit stays free, the row as it was
            continue
        if rb["status"] != 0:
            continue
        d = np.abs(grid - see[i])
        nearest = grid[np.flatnonzero(d == d.min())[0]]    # (a tie: the lower)
        assert rb["seeing_arcsec"] == pytest.approx(nearest, abs=1e-9), (i, rb, see[i])
        checked += 1
    assert checked >= 2


def test_two_ranks_and_a_resumed_run(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    rows = case()[4]
    tree(tmp_path)
    one, o_out = run(tmp_path, "one", **SEE)
    two = tmp_path / "two"
    two.mkdir()
    for r in (0, 1):
        DetectTrails(savepath=str(two), **SEE, **KW).process(batch=2, rank=r, world_size=2)
    for name in ("seeing.txt", "results.txt"):
        whole = read(o_out / name)
        assert whole and read(two / (name + ".rank0")) + read(two / (name + ".rank1")) == whole, name
    assert lines(o_out / "seeing.txt") == rows
    # a complete run resumed appends nothing; with the marks of the last two frames taken away it does those again, and only those
    dt = DetectTrails(savepath=str(o_out), **SEE, **KW)
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS and lines(o_out / "seeing.txt") == rows
    marks = lines(o_out / "results.txt.progress")
    with open(o_out / "results.txt.progress", "w") as f:
        f.write("\n".join(marks[:-2]) + "\n")
    dt.process(batch=4, resume=True)
    assert dt.last_stats["skipped_by_resume"] == N_FIELDS - 2 and lines(o_out / "seeing.txt") == rows + rows[-2:]


def test_the_rows_do_not_depend_on_find_stars(tmp_path):
    rows = case()[4]
    tree(tmp_path, photoobj=False)
    for batch in (1, 4):
        dt, out = run(tmp_path, "found%d" % batch, batch=batch, find_stars=True, **SEE)
        assert lines(dt.seeing_file) == rows and len(lines(dt.stars_file)) == N_FIELDS and not lines(dt.errors), batch
