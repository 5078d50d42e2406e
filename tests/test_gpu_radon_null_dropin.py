"""DetectTrails(radon=True, radon_lines=2, radon_null=4) end to end on the three-frame tree of test_gpu_radon_wide_dropin.py:
radon_null.txt and radon_fap.txt against the restatement (tests/radon_null_ref.py on the frames the chunk's search reads: the
loader's frames, which the detect call's remove_stars blots only in its own device copy; seeded by ``radon.null_seed``), the same
files from a two-rank split and from a resumed run, the frame-at-a-time path's rows (there the search and the null read the
frame as that path's remove_stars left it), and every other output byte for byte what a run without ``radon_null`` writes; ``recovery.run(null=K)`` against the
restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_null_ref as NR  # noqa: E402
import radon_ref as R  # noqa: E402
import test_gpu_radon_wide_dropin as TD  # noqa: E402

pytestmark = pytest.mark.gpu

K = 4
KW = {"run": 94, "camcol": 1, "filter": "r", "radon": True, "radon_lines": 2}


def restated(frames, cats):
    """(radon_null.txt rows, radon_fap.txt rows) of the restatement: fields 100 and 101 (102 has a detection: not searched)"""
    from lfd_amd import radon
    null_rows, fap_rows = [], []
    for i in (0, 1):
        f = frames[i]
        key = (94, 1, "r", 100 + i)
        null = NR.null_snr(f[None], K, "lines", 0.025, seeds=[radon.null_seed(*key)])[0]
        null_rows.append(radon.format_null_row(key, "lines", null))
        recs, n_lines = L.search_lines(f, 0.025, max_lines=2)
        for k in range(n_lines):
            fap_rows.append(radon.format_fap_row(key, "lines", k, recs[k]["snr"], null))
    return null_rows, fap_rows


def lines_of(path):
    with open(path) as f:
        return [ln for ln in f.read().splitlines() if ln.strip()]


def test_dropin_writes_the_null_files_and_leaves_the_others(tmp_path):
    from lfd_amd import radon
    from lfd_amd.detecttrails import DetectTrails
    frames, cats, _ = TD.make_tree(tmp_path)
    want_null, want_fap = restated(frames, cats)
    runs = {}
    for name, kw in (("base", {}), ("null", {"radon_null": K})):
        d = tmp_path / name
        d.mkdir()
        runs[name] = DetectTrails(savepath=str(d), **KW, **kw)
        runs[name].process(batch=4)
    base, null = runs["base"], runs["null"]
    assert lines_of(null.radon_null_file) == want_null and lines_of(null.radon_fap_file) == want_fap
    assert len(want_null) == 2 and len(want_fap) >= 1                      # the faint wide trail of field 101 is found
    rows = radon.read_null(null.radon_null_file)
    assert [(r["field"], r["kind"], r["K"]) for r in rows] == [(100, "lines", K), (101, "lines", K)]
    assert all(3.5 < r["null_min"] <= r["null_median"] <= r["null_max"] < 8.0 for r in rows)
    fap = radon.read_fap(null.radon_fap_file)
    assert all(r["field"] == 101 and r["K"] == K and r["fap"] == (1 + r["n_ge"]) / (K + 1) for r in fap)
    assert fap[0]["n_ge"] == 0 and fap[0]["fap"] == 1 / (K + 1)
    # every other output is byte for byte what it is without radon_null
    assert sorted(os.listdir(tmp_path / "null")) == sorted(os.listdir(tmp_path / "base") + ["radon_null.txt", "radon_fap.txt"])
    for name in os.listdir(tmp_path / "base"):
        assert (tmp_path / "null" / name).read_bytes() == (tmp_path / "base" / name).read_bytes(), name
    # two ranks: their files, in rank order, are the one run's
    d = tmp_path / "ranks"
    d.mkdir()
    for rank in (0, 1):
        DetectTrails(savepath=str(d), radon_null=K, **KW).process(batch=4, rank=rank, world_size=2)
    for name, want in (("radon_null.txt", want_null), ("radon_fap.txt", want_fap)):
        assert lines_of(d / (name + ".rank0")) + lines_of(d / (name + ".rank1")) == want, name
    # the frame-at-a-time path
    d = tmp_path / "single"
    d.mkdir()
    DetectTrails(savepath=str(d), radon_null=K, **KW).process(batch=1)
    single = radon.read_null(d / "radon_null.txt")
    assert [(r["field"], r["kind"], r["K"]) for r in single] == [(100, "lines", K), (101, "lines", K)]
    assert all(3.5 < r["null_min"] <= r["null_max"] < 8.0 for r in single)
    sfap = radon.read_fap(d / "radon_fap.txt")
    assert [(r["field"], r["line"]) for r in sfap] == [(r["field"], r["line"]) for r in fap]
    assert all(r["fap"] == (1 + r["n_ge"]) / (K + 1) for r in sfap)
    # resume: a finished run adds nothing; a run that stopped after field 100 adds the rest
    again = DetectTrails(savepath=str(tmp_path / "null"), radon_null=K, **KW)
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 3
    assert lines_of(null.radon_null_file) == want_null and lines_of(null.radon_fap_file) == want_fap
    progress = null.results + ".progress"
    marks = lines_of(progress)
    with open(progress, "w") as f:
        f.write("\n".join(marks[:2]) + "\n")                               # the header and field 100's mark
    for path in (null.radon_null_file, null.radon_fap_file):
        kept = [ln for ln in lines_of(path) if ln.split()[3] == "100"]
        with open(path, "w") as f:
            f.write("".join(ln + "\n" for ln in kept))
    again.process(batch=4, resume=True)
    assert again.last_stats["skipped_by_resume"] == 1
    assert lines_of(null.radon_null_file) == want_null and lines_of(null.radon_fap_file) == want_fap


def test_every_kind_that_is_on_gets_its_rows(tmp_path):
    from lfd_amd import radon
    from lfd_amd.detecttrails import DetectTrails
    TD.make_tree(tmp_path)
    d = tmp_path / "all"
    d.mkdir()
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(d), radon=True, radon_short=True, radon_wide=True, radon_null=2)
    dt.process(batch=4)
    rows = radon.read_null(dt.radon_null_file)
    assert [(r["field"], r["kind"]) for r in rows] == [(f, k) for f in (100, 101) for k in ("lines", "short", "wide")]
    fap = radon.read_fap(dt.radon_fap_file)
    wide = radon.read_wide(dt.radon_wide_file)
    assert [(r["field"], r["line"], r["snr"]) for r in fap if r["kind"] == "wide"] == [(r["field"], r["line"], r["snr"]) for r in wide]
    assert len(wide) >= 1 and all(r["fap"] == 1 / 3 for r in fap if r["kind"] == "wide")


def test_recovery_reports_the_false_alarm_estimate_of_its_trails(gpu_ctx):
    """full crossings of peak 0.03 on 256 x 384 noise at bin 2: ``run(null=K)`` returns the rows it returns without and each
    trail's estimate, which is the restatement's; the table gets its median over the recovered trails"""
    from lfd_amd import inject as I, radon, recovery as RC
    shape, n = (256, 384), 4
    frames = np.random.default_rng(41).normal(0, 0.025, (n, *shape)).astype(np.float32)
    plan = RC.draw_trails(n, shape, 5, [0.03, 0.001])
    table, step = I.gaussian_table(2.0)
    table = I.normalise_peak(table)
    kw = {"radon_params": {"bin": 2, "min_len": 64}, "sigma": 0.025, "detector": "radon"}
    with __import__("lfd_amd")._native.Context(0, *shape, n) as ctx:
        rows = RC.run(ctx, frames, None, None, plan, table, step, **kw)
        rows2, fap = RC.run(ctx, frames, None, None, plan, table, step, null=K, **kw)
        work = frames.copy()
        ctx.inject_trails(work, RC.to_inject(plan), np.asarray(table, np.float32), step, subsample=4)      # what run() searches
    assert rows.tobytes() == rows2.tobytes() and fap.shape == (n,) and fap.dtype == np.float64
    want = [radon.false_alarm(R.search(work[i], 0.025, bin=2, min_len=64)["snr"],
                              NR.null_snr(work[i:i + 1], K, "lines", 0.025, seeds=[i], bin=2, min_len=64)[0]) for i in range(n)]
    assert fap.tolist() == want
    assert rows["matched"][::2].all() and (fap[::2] == 1 / (K + 1)).all()   # peak 0.03 is found, above every null peak
    t = RC.completeness(rows, RC.peak_edges([0.03, 0.001]), fap=fap)
    assert t[1]["median_fap"] == 1 / (K + 1) and "median_fap" in RC.format_table(t).splitlines()[0]
