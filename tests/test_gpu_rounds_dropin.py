"""``DetectTrails(max_trails=3)`` end to end on the GPU: a small ``synth.write_boss_tree`` selection with two-streak frames.
results.txt, errors.txt and masks.txt are byte-identical to the run without ``max_trails``; trails.txt holds the rows
tests/rounds_ref.py gives on the oracle; a two-rank split, the frame-at-a-time path and a resumed run give the same rows;
``max_trails`` unset or 1 writes no trails.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_cases as RC  # noqa: E402
import rounds_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
LAYOUT = ((0, 2), (1,), (), (0, 2), (1, 2))
KW = dict(run=94, camcol=1, filter="r", trail_masks=True)
RP = {"half": RC.HALF}


def lines_of(path):
    with open(path) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


@pytest.fixture(scope="module")
def tree(tmp_path_factory, oracle):
    from lfd_amd import rounds, synth
    from lfd_amd.detecttrails import default_params
    root = tmp_path_factory.mktemp("rounds_tree")
    frames, cats = RC.frames(LAYOUT)
    synth.write_boss_tree(root, list(frames), cats, field0=100)
    pb, pd, prs = default_params()
    rs = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    want = []
    for i in range(len(LAYOUT)):
        recs, nf, dup = RR.rounds(frames[i], RR.oracle_detect(oracle, pb, pd, cats[i], rs), 3, RC.HALF)
        want += [rounds.format_row((94, 1, "r", 100 + i), k, recs[k], dup[k]) for k in range(nf)]
    return root, want


def test_the_drop_in(tree):
    from lfd_amd import rounds
    from lfd_amd.detecttrails import DetectTrails
    root, want = tree
    assert [int(r.split()[4]) for r in want].count(1) >= 3                 # (several frames have a second trail)
    plain, multi = root / "plain", root / "multi"
    plain.mkdir()
    multi.mkdir()
    DetectTrails(savepath=str(plain), **KW).process(batch=4)
    dt = DetectTrails(savepath=str(multi), max_trails=3, rounds_params=RP, **KW)
    dt.process(batch=4)
    assert sorted(os.listdir(multi)) == sorted(os.listdir(plain) + ["trails.txt"])
    for name in os.listdir(plain):
        if os.path.isfile(plain / name):
            assert open(multi / name, "rb").read() == open(plain / name, "rb").read(), name
    assert lines_of(plain / "results.txt")
    assert lines_of(dt.trails_file) == want
    rows = rounds.read_trails(dt.trails_file)
    assert [r["field"] for r in rows if r["round"] == 0] == [int(ln.split()[3]) for ln in lines_of(plain / "results.txt")]
    # max_trails = 1: nothing differs and no file appears
    one = root / "one"
    one.mkdir()
    DetectTrails(savepath=str(one), max_trails=1, **KW).process(batch=4)
    assert sorted(os.listdir(one)) == sorted(os.listdir(plain))
    # two ranks, rows in selection order
    two = root / "two"
    two.mkdir()
    for r in (0, 1):
        DetectTrails(savepath=str(two), max_trails=3, rounds_params=RP, **KW).process(batch=2, rank=r, world_size=2)
    assert lines_of(two / "trails.txt.rank0") + lines_of(two / "trails.txt.rank1") == want
    assert lines_of(two / "results.txt.rank0") + lines_of(two / "results.txt.rank1") == lines_of(plain / "results.txt")
    # the frame-at-a-time path
    single = root / "single"
    single.mkdir()
    DetectTrails(savepath=str(single), max_trails=3, rounds_params=RP, **KW).process(batch=1)
    assert lines_of(single / "trails.txt") == want
    # resume: a finished run adds nothing; a run that stopped after field 101 adds the rest
    again = DetectTrails(savepath=str(multi), max_trails=3, rounds_params=RP, **KW)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == len(LAYOUT) and lines_of(dt.trails_file) == want
    progress = dt.results + ".progress"
    marks = lines_of(progress)
    with open(progress, "w") as f:
        f.write("\n".join(marks[:3]) + "\n")                                # the header and the marks of fields 100, 101
    for path in (dt.trails_file, dt.results, dt.masks_file):
        kept = [ln for ln in lines_of(path) if ln.split()[3] in ("100", "101")]
        with open(path, "w") as f:
            f.write("".join(ln + "\n" for ln in kept))
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 2
    assert lines_of(dt.trails_file) == want and lines_of(dt.results) == lines_of(plain / "results.txt")


def test_bad_arguments():
    from lfd_amd.detecttrails import DetectTrails
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError):
            DetectTrails(run=94, camcol=1, filter="r", max_trails=bad)
    with pytest.raises(ValueError):
        DetectTrails(run=94, camcol=1, filter="r", rounds_params={"half": 3.0})
    with pytest.raises(TypeError):
        DetectTrails(run=94, camcol=1, filter="r", max_trails=2, rounds_params={"width": 3.0})
