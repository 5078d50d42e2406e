"""DetectTrails(defocus=True): defocus.txt has one row per results.txt row, each the fit the restatement (tests/defocus_ref.py)
gives for that run's profiles.txt row; plain files, .fits.bz2 files and two Jobs workers write the same file; with the option
off no defocus file appears."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defocus_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = {"heights": [70.0, 90.0, 120.0, 160.0, 250.0], "radii": [0.0, 1.0], "seeings": [1.0, 1.4, 1.8]}


def boss_tree(root, n=6, bz2_all=False):
    from lfd_amd import synth
    frames, cats = zip(*[synth.make_frame(40 + k)[:2] for k in range(n)])
    synth.write_boss_tree(root, list(frames), list(cats), field0=100, bz2_all=bz2_all)


def profile_rows(path):
    from lfd_amd import _native
    nf = len(_native.TRAIL_DTYPE.names)
    out = []
    for line in open(path):
        f = line.split()
        if not f:
            continue
        tr = np.zeros(1, _native.TRAIL_DTYPE)[0]
        for name, v in zip(_native.TRAIL_DTYPE.names, f[4:4 + nf]):
            tr[name] = float(v)
        out.append((tuple(f[:4]), tr, np.array([float(x) for x in f[4 + nf:]], np.float32)))
    return out


def test_defocus_rows_equal_the_restatement(tmp_path):
    from lfd_amd import _native, defocus
    from lfd_amd.detecttrails import DetectTrails
    boss_tree(tmp_path / "boss")
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir()
    off.mkdir()
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(on), defocus=True, defocus_params=GRID)
    assert dt.trail_profiles
    dt.process(batch=4)
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=4)
    assert not os.path.exists(off / "defocus.txt") and not os.path.exists(off / "profiles.txt")
    assert open(on / "results.txt", "rb").read() == open(off / "results.txt", "rb").read()
    keys = [tuple(ln.split()[:4]) for ln in open(on / "results.txt") if ln.strip()]
    rows = defocus.read_defocus(on / "defocus.txt")
    prof = profile_rows(on / "profiles.txt")
    assert len(keys) >= 2
    assert [(str(r["run"]), str(r["camcol"]), r["filter"], str(r["field"])) for r in rows] == keys == [p[0] for p in prof]
    g = R.Grid()
    c32, c64, models = R.bank(g, GRID["heights"], GRID["radii"], GRID["seeings"])
    ns = 2 * g.S + 1
    fitted = 0
    for (key, tr, v), row in zip(prof, rows):
        if tr["status"] != _native.TRAIL_OK:
            assert row["status"] == _native.DEFOCUS_NOT_MEASURED and math.isnan(row["chi2"])
            continue
        chi2, curve = R.fit(g, c64, models, len(GRID["heights"]), GRID["seeings"], tr, v)
        assert row["status"] == _native.DEFOCUS_OK, (key, row)
        col = [j for j, m in enumerate(models)
               if (m["h"], m["R"], m["seeing"]) == (row["h_km"], row["radius_m"], row["seeing_arcsec"])][0] * ns + row["shift"] + g.S
        cmin = np.nanmin(chi2)
        assert chi2[col] <= cmin + 1e-4 * abs(cmin), (key, chi2[col], cmin)
        assert abs(row["chi2"] - chi2[col]) <= 1e-6 * abs(chi2[col]), key
        assert row["dof"] == 2 * g.K - 1
        scale = float(((v - v.mean()) ** 2).sum() / tr["noise"] ** 2)
        assert abs(row["chi2_focus"] - curve[-1]) <= 1e-5 * scale + 1e-3, key
        fitted += 1
    assert fitted >= 2


def test_bz2_tree_and_jobs_give_the_same_defocus_file(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    from lfd_amd.jobs import Jobs
    plain, packed, jobs = tmp_path / "plain", tmp_path / "bz2", tmp_path / "jobs"
    boss_tree(plain / "boss")
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain), defocus=True, defocus_params=GRID).process(batch=4)
    want = open(plain / "defocus.txt", "rb").read()
    assert want.count(b"\n") >= 2
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain / "one"), defocus=True, defocus_params=GRID,
                 results=str(plain / "r1.txt"), errors=str(plain / "e1.txt"), profiles=str(plain / "p1.txt"),
                 defocus_file=str(plain / "d1.txt")).process(batch=1)
    assert open(plain / "d1.txt", "rb").read() == want
    boss_tree(packed / "boss", bz2_all=True)
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(packed), defocus=True, defocus_params=GRID).process(batch=4)
    assert open(packed / "defocus.txt", "rb").read() == want
    jobs.mkdir()
    Jobs(2, devices=[0, 0], run=94, camcol=1, filter="r", savepath=str(jobs), defocus=True,
         defocus_params=GRID).launch(batch=4, timeout=600)
    assert open(jobs / "defocus.txt", "rb").read() == want
    assert not os.path.exists(str(jobs / "defocus.txt") + ".rank0")
