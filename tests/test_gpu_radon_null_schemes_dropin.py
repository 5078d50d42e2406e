"""DetectTrails(radon_null=K, radon_null_scheme=, radon_null_rounds=) end to end on the three-frame tree of
test_gpu_radon_wide_dropin.py, in the manner of test_gpu_radon_null_dropin.py: the defaults spelled out give every file byte for
byte, "signflip" fills radon_null.txt and radon_fap.txt with the restatement's rows (tests/radon_null_schemes_ref.py),
``radon_null_rounds=True`` writes radon_null_rounds.txt and takes the radon_fap.txt rows of lines k >= 1 from round k's peaks,
rounds without the sign flip are refused, and a resumed run and a two-rank split give the same rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_null_schemes_ref as NS  # noqa: E402
import test_gpu_radon_wide_dropin as TD  # noqa: E402
from test_gpu_radon_null_dropin import lines_of  # noqa: E402

pytestmark = pytest.mark.gpu

K = 4
THRESHOLD = 7.5      # field 101's second line scores 7.9: below the default threshold, found at this one
KW = {"run": 94, "camcol": 1, "filter": "r", "radon": True, "radon_lines": 3, "radon_params": {"threshold": THRESHOLD}}


def restated(frames, rounds):
    """(radon_null.txt, radon_fap.txt, radon_null_rounds.txt rows) of the restatement under the sign flip: fields 100 and 101"""
    from lfd_amd import radon
    null_rows, fap_rows, round_rows = [], [], []
    for i in (0, 1):
        f = frames[i]
        key = (94, 1, "r", 100 + i)
        recs, n_lines = L.search_lines(f, 0.025, max_lines=3, threshold=THRESHOLD)
        if rounds:
            null = NS.null_rounds(f[None], [recs], [n_lines], K, "lines", 0.025, seeds=[radon.null_seed(*key)], threshold=THRESHOLD)[0]
        else:
            null = NS.null_snr(f[None], K, "lines", 0.025, seeds=[radon.null_seed(*key)], scheme="signflip")
        null_rows.append(radon.format_null_row(key, "lines", null[0]))
        for k in range(1, min(n_lines, 2) + 1 if rounds else 0):
            round_rows.append(radon.format_null_rounds_row(key, "lines", k, null[k]))
        for k in range(n_lines):
            fap_rows.append(radon.format_fap_row(key, "lines", k, recs[k]["snr"], null[k] if rounds else null[0]))
    return null_rows, fap_rows, round_rows


def test_the_defaults_spelled_out_change_no_byte(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    TD.make_tree(tmp_path)
    for name, kw in (("base", {}), ("spelled", {"radon_null_scheme": "scramble", "radon_null_rounds": False})):
        d = tmp_path / name
        d.mkdir()
        DetectTrails(savepath=str(d), radon_null=K, **KW, **kw).process(batch=4)
    assert sorted(os.listdir(tmp_path / "base")) == sorted(os.listdir(tmp_path / "spelled")) and "radon_null_rounds.txt" not in os.listdir(tmp_path / "base")
    for name in os.listdir(tmp_path / "base"):
        assert (tmp_path / "spelled" / name).read_bytes() == (tmp_path / "base" / name).read_bytes(), name
    for scheme in ("scramble", "rowshift", "colshift"):
        with pytest.raises(ValueError):
            DetectTrails(savepath=str(tmp_path), radon_null=K, radon_null_scheme=scheme, radon_null_rounds=True, **KW)


def test_signflip_rows_and_rounds(tmp_path):
    from lfd_amd import radon
    from lfd_amd.detecttrails import DetectTrails
    frames, cats, _ = TD.make_tree(tmp_path)
    want = {False: restated(frames, False), True: restated(frames, True)}
    runs = {}
    for name, kw in (("base", {}), ("flip", {"radon_null_scheme": "signflip"}), ("rounds", {"radon_null_scheme": "signflip", "radon_null_rounds": True})):
        d = tmp_path / name
        d.mkdir()
        runs[name] = DetectTrails(savepath=str(d), radon_null=K, **KW, **kw)
        runs[name].process(batch=4)
    flip, rounds = runs["flip"], runs["rounds"]
    assert lines_of(flip.radon_null_file) == want[False][0] and lines_of(flip.radon_fap_file) == want[False][1]
    assert not os.path.exists(flip.radon_null_rounds_file)
    assert lines_of(flip.radon_null_file) != lines_of(runs["base"].radon_null_file)      # another scheme, other peaks
    # rounds: round 0's rows are the sign flip's, the new file has a row per round k >= 1 that ran, line k's estimate is round k's
    assert lines_of(rounds.radon_null_file) == want[True][0] == want[False][0]
    assert lines_of(rounds.radon_null_rounds_file) == want[True][2] and lines_of(rounds.radon_fap_file) == want[True][1]
    rr = radon.read_null_rounds(rounds.radon_null_rounds_file)
    assert [(r["field"], r["kind"], r["round"], r["K"]) for r in rr] == [(101, "lines", 1, K), (101, "lines", 2, K)]
    fap = radon.read_fap(rounds.radon_fap_file)
    assert [(r["field"], r["line"]) for r in fap] == [(101, 0), (101, 1)] and all(r["fap"] == (1 + r["n_ge"]) / (K + 1) for r in fap)
    # line 0 is held against round 0, line 1 against round 1, whose peaks are others (field 101 lost its first line's band)
    assert want[True][1][0] == want[False][1][0] and want[True][2][0].split()[7:] != want[True][0][1].split()[6:]
    assert lines_of(rounds.radon_fap_file)[1] == radon.format_fap_row((94, 1, "r", 101), "lines", 1, fap[1]["snr"], np.array(
        [rr[0]["null_max"]] * K, np.float32))                              # (above every peak of round 1: the row only needs its maximum)
    # every other output is byte for byte what it is without the new arguments
    assert sorted(os.listdir(tmp_path / "rounds")) == sorted(os.listdir(tmp_path / "base") + ["radon_null_rounds.txt"])
    for name in set(os.listdir(tmp_path / "base")) - {"radon_null.txt", "radon_fap.txt"}:
        assert (tmp_path / "rounds" / name).read_bytes() == (tmp_path / "base" / name).read_bytes(), name
    # two ranks: their files, in rank order, are the one run's
    d = tmp_path / "ranks"
    d.mkdir()
    kw = {"radon_null_scheme": "signflip", "radon_null_rounds": True}
    for rank in (0, 1):
        DetectTrails(savepath=str(d), radon_null=K, **KW, **kw).process(batch=4, rank=rank, world_size=2)
    for name, rows in (("radon_null.txt", want[True][0]), ("radon_fap.txt", want[True][1]), ("radon_null_rounds.txt", want[True][2])):
        assert lines_of(d / (name + ".rank0")) + lines_of(d / (name + ".rank1")) == rows, name
    # the frame-at-a-time path writes the same kinds of rows
    d = tmp_path / "single"
    d.mkdir()
    DetectTrails(savepath=str(d), radon_null=K, **KW, **kw).process(batch=1)
    assert [(r["field"], r["round"]) for r in radon.read_null_rounds(d / "radon_null_rounds.txt")] == [(r["field"], r["round"]) for r in rr]
    # resume: a finished run adds nothing; a run that stopped after field 100 adds the rest
    again = DetectTrails(savepath=str(tmp_path / "rounds"), radon_null=K, **KW, **kw)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 3
    assert lines_of(rounds.radon_null_rounds_file) == want[True][2]
    progress = rounds.results + ".progress"
    marks = lines_of(progress)
    with open(progress, "w") as f:
        f.write("\n".join(marks[:2]) + "\n")                               # the header and field 100's mark
    for path in (rounds.radon_null_file, rounds.radon_fap_file, rounds.radon_null_rounds_file):
        kept = [ln for ln in lines_of(path) if ln.split()[3] == "100"]
        with open(path, "w") as f:
            f.write("".join(ln + "\n" for ln in kept))
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 1
    assert lines_of(rounds.radon_null_file) == want[True][0] and lines_of(rounds.radon_fap_file) == want[True][1]
    assert lines_of(rounds.radon_null_rounds_file) == want[True][2]

