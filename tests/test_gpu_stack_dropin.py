"""DetectTrails(radon=True, radon_lines=K, radon_profiles=True) end to end, after test_gpu_radon_lines' drop-in test: the
radon_profiles.txt rows are ``format_row`` of the restatement (tests/stack_ref.py) on the segments radon_segments.txt carries, and
results.txt, errors.txt, radon.txt and radon_segments.txt do not change with the flag."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import stack_ref as S  # noqa: E402
import test_gpu_radon as TG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", [1, 4])
def test_dropin_profiles(tmp_path, batch):
    """three frames: noise, two faint trails, one bright trail; catalogues whose one object is too faint to be blotted, so the
    frames the search and the measurement see are the files' pixels whichever path (and byte order) they take"""
    from lfd_amd import _native, inject as I, radon, stack, synth
    from lfd_amd.detecttrails import DetectTrails, default_params
    from oracle import lfd_oracle as O
    shape = (512, 768)
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (3, *shape)).astype(np.float32)
    tr = np.zeros(3, IR.TRAIL_DTYPE)
    th, th2 = math.radians(115.0), math.radians(30.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    tr[0] = (1, 0, rho, th, -np.inf, np.inf, 0.03)
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    tr[2] = (1, 0, 400 * math.cos(th2) + 240 * math.sin(th2), th2, -np.inf, np.inf, 0.025)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cat = {k: v[:1].copy() for k, v in synth.make_portable_frame(0, shape)[1].items()}
    cat["PSFMAG"][:] = 30.0
    prs = default_params()[2]
    blot = frames[1].copy()
    O.remove_stars(blot, cat, O.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"}))
    assert np.array_equal(blot.view(np.uint32), frames[1].view(np.uint32))
    synth.write_boss_tree(tmp_path, list(frames), [cat] * 3, field0=100, filter="r", bz2_fields=(101,) if batch > 1 else ())
    outs = {}
    sp = {"step": 0.25, "n_iter": 1}
    for name, kw in (("lines", {}), ("prof", {"radon_profiles": True}), ("params", {"radon_profiles": True, "stack_params": sp}),
                     ("fit", {"radon_profiles": True, "defocus": True, "defocus_params": {"heights": [80.0, 120.0], "radii": [0.0]}})):
        d = tmp_path / name
        d.mkdir()
        dt = outs[name] = DetectTrails(run=94, camcol=1, filter="r", savepath=str(d), radon=True, radon_lines=3, **kw)
        dt.process(batch=batch)
    base = outs["lines"]
    assert not os.path.exists(base.radon_profiles_file) and not os.path.exists(base.radon_defocus_file)
    segs = radon.read_segments(base.radon_segments_file)
    assert [(s["field"], s["line"]) for s in segs] == [(101, 0), (101, 1)]
    for name in ("prof", "params", "fit"):
        dt = outs[name]
        assert TG.lines(dt.results) == TG.lines(base.results) and open(dt.radon_file).read() == open(base.radon_file).read()
        assert open(dt.radon_segments_file).read() == open(base.radon_segments_file).read()
        if name != "fit":
            assert open(dt.errors).read() == open(base.errors).read() and not os.path.exists(dt.radon_defocus_file)
        want = []
        for s in segs:
            rec = S.measure(frames[1], (s["ex1"], s["ey1"], s["ex2"], s["ey2"]), **(sp if name == "params" else {}))[0]
            want.append(stack.format_row((94, 1, "r", 101), s["line"], rec))
        assert TG.lines(dt.radon_profiles_file) == want
    rows = stack.read_profiles(outs["prof"].radon_profiles_file)
    assert [r["status"] for r in rows] == [S.OK, S.OK] and all(3.0 <= r["fwhm"] <= 6.0 and r["snr"] > 8 for r in rows)
    fits = [ln.split() for ln in TG.lines(outs["fit"].radon_defocus_file)]
    assert [f[:6] for f in fits] == [["94", "1", "r", "101", "0", str(_native.DEFOCUS_OK)], ["94", "1", "r", "101", "1", str(_native.DEFOCUS_OK)]]
