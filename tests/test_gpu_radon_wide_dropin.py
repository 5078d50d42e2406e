"""DetectTrails(radon=True, radon_wide=...) end to end: the radon_wide.txt rows against the numpy restatement
(tests/radon_wide_ref.py) on the frames as the detect call leaves them (the oracle's remove_stars), and every other output
file byte for byte what a run without the option writes."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_wide_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (512, 768)


def make_tree(tmp_path):
    """test_gpu_radon_short's three-frame tree with a wide faint trail (Gaussian sigma 6 px, peak 0.006: a quarter of the sky
    sigma) in field 101 instead of its short one; field 100 is noise, field 102 has the trail the detector finds"""
    import inject_ref as IR
    from lfd_amd import inject as I, synth
    rng = np.random.default_rng(14)
    frames = rng.normal(0, 0.025, (3, *SHAPE)).astype(np.float32)
    th = math.radians(115.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    wide = np.zeros(1, IR.TRAIL_DTYPE)
    wide[0] = (1, 0, rho, th, -np.inf, np.inf, 0.006)
    table, step = I.gaussian_table(6.0)
    IR.inject(frames, wide, I.normalise_peak(table).astype(np.float32), step)
    bright = np.zeros(1, IR.TRAIL_DTYPE)
    bright[0] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, bright, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, SHAPE)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r")
    return frames, cats, (rho, th)


def restated(frames, cats, **params):
    """{field: (records, n_lines)} of the restatement on the frames without their catalogue's stars"""
    from lfd_amd.detecttrails import default_params
    from oracle import lfd_oracle as O
    prs = {k: v for k, v in default_params()[2].items() if k != "debug"}
    out = {}
    for i in (0, 1):                                       # (field 102 has a detection: it is not searched)
        f = frames[i].copy()
        O.remove_stars(f, cats[i], O.rs_params("r", **prs))
        recs, n_lines, _ = W.search_wide(f, 0.025, **params)
        out[100 + i] = (recs, n_lines)
    return out


def same_rows(rows, ref):
    want = [(field, k, recs[k]) for field, (recs, n) in sorted(ref.items()) for k in range(n)]
    assert [(r["field"], r["line"]) for r in rows] == [(f, k) for f, k, _ in want]
    for r, (_, _, rec) in zip(rows, want):
        for key in ("width", "n_pix", "seg_n_pix"):
            assert r[key] == int(rec[key]), key
        for key in ("width_px", "ex1", "ey1", "ex2", "ey2"):
            assert r[key] == float(rec[key]), key
        for key in ("snr", "seg_snr"):
            assert r[key] == float(np.float32(rec[key])), key


def test_dropin_writes_radon_wide_and_leaves_the_other_files(tmp_path):
    from lfd_amd import radon, stack
    from lfd_amd.detecttrails import DetectTrails
    frames, cats, (rho, th) = make_tree(tmp_path)
    c, s = math.cos(th), math.sin(th)
    outs = {}
    for name, kw in (("one", {"radon": True}), ("wide", {"radon": True, "radon_wide": True}),
                     ("lines", {"radon": True, "radon_lines": 2}),
                     ("both", {"radon": True, "radon_lines": 2, "radon_wide": {"max_lines": 2, "max_width": 16},
                               "radon_profiles": True})):
        d = tmp_path / name
        d.mkdir()
        dt = outs[name] = DetectTrails(run=94, camcol=1, filter="r", savepath=str(d), **kw)
        dt.process(batch=4)
    one, wide, lines, both = (outs[k] for k in ("one", "wide", "lines", "both"))
    # the default leaves no radon_wide.txt; with it every other file is byte for byte what it was (radon.txt comes from the
    # wide call's plain records there)
    assert not os.path.exists(one.radon_wide_file) and not os.path.exists(lines.radon_wide_file)
    for name in ("results", "errors", "radon_file"):
        assert open(getattr(wide, name)).read() == open(getattr(one, name)).read(), name
        assert open(getattr(both, name)).read() == open(getattr(lines, name)).read(), name
    assert open(both.radon_segments_file).read() == open(lines.radon_segments_file).read()
    assert not os.path.exists(wide.radon_segments_file) and not os.path.exists(wide.radon_short_file)
    assert sorted(os.listdir(tmp_path / "wide")) == sorted(os.listdir(tmp_path / "one") + ["radon_wide.txt"])
    # the rows are the restatement's
    rows = radon.read_wide(wide.radon_wide_file)
    print("radon_wide.txt", rows)
    same_rows(rows, restated(frames, cats))
    assert [(r["field"], r["line"]) for r in rows] == [(101, 0)]
    r = rows[0]
    assert r["snr"] >= 8.0 and r["width"] >= 4 and 0.7 * 2 * r["width"] <= r["width_px"] <= 2 * r["width"]
    for x, y in ((r["ex1"], r["ey1"]), (r["ex2"], r["ey2"])):                         # the segment lies along the trail
        assert abs(x * c + y * s - rho) <= 6.0
    assert len(open(wide.radon_wide_file).read().split()) == len(radon.WIDE_COLUMNS)
    # with other parameters, the lines and the profiles: rows tagged by their source, the wide ones measured on the band's segment
    rows2 = radon.read_wide(both.radon_wide_file)
    same_rows(rows2, restated(frames, cats, max_lines=2, max_width=16))
    tags = [ln.split()[-1] for ln in open(both.radon_profiles_file).read().splitlines() if ln.strip()]
    assert set(tags) <= {"lines", "wide"} and tags.count("wide") == len(rows2) >= 1
    assert tags.count("lines") == len(radon.read_segments(both.radon_segments_file))
    prof = stack.read_profiles(both.radon_profiles_file)
    assert len(prof) == len(tags) and all(p["field"] == 101 for p in prof)

