"""The defocus model's restatement (tests/defocus_ref.py) in its limits, the Python side of the defocus fit without a GPU: the
ctypes mirrors against include/lfdmi.h, the default grid, parameter checks, the grid's fields, and defocus.txt rows."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defocus_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_components_integrate_to_one_on_the_fine_grid():
    g = R.Grid()
    to, ti, rho = R.angles(g, 100.0, 2.0)
    assert abs(R.defocus_raw(to, ti, g.delta).sum() * g.delta - 1) < 1e-4
    assert abs(R.disk_raw(rho, g.delta).sum() * g.delta - 1) < 1e-3
    sigma = 1.035 / R.FWHM2SIGMA * 1.43
    assert abs(R.seeing_raw(1.43, g.delta).sum() * g.delta / (math.sqrt(2 * math.pi) * sigma) - 1) < 1e-3  # 4 sigma: 0.99994
    assert R.box_raw(g.F).sum() == pytest.approx(g.F, rel=1e-12)    # 1 px of fine steps
    assert R.tri_raw(g.F).sum() == pytest.approx(g.F, rel=1e-12)
    for w in (R.unit(R.defocus_raw(to, ti, g.delta)), R.kernel(g, 1.43), R.od(g, 100.0, 2.0)):
        assert w.sum() == pytest.approx(1.0, abs=1e-12)


def test_defocus_is_symmetric_with_a_central_dip():
    g = R.Grid()
    to, ti, _ = R.angles(g, 100.0, 0.0)
    d = R.defocus_raw(to, ti, g.delta)
    assert np.array_equal(d, d[::-1])
    c = len(d) // 2
    assert d[c] < d.max()


def test_far_models_approach_the_focus_model():
    g = R.Grid()
    focus = R.model(g, np.inf, 0.0, 1.43)["samp"]
    prev = None
    for h in (200.0, 2000.0, 20000.0):
        d = np.abs(R.model(g, h, 0.0, 1.43)["samp"] - focus).max() / focus.max()
        if prev is not None:
            assert d < prev
        prev = d
    assert prev < 1e-3


def test_defocus_fwhm_scales_as_one_over_h():
    g = R.Grid(ovs=16)
    w = {h: R.model(g, h, 0.0, 1.43)["dfwhm"] for h in (80.0, 160.0)}
    assert w[80.0] / w[160.0] == pytest.approx(2.0, rel=0.01)
    assert R.model(g, np.inf, 0.0, 1.43)["dfwhm"] == 0.0


def test_a_disk_of_radius_zero_is_the_point():
    g = R.Grid()
    a, b = R.model(g, 100.0, 0.0, 1.43), R.model(g, 100.0, 1e-12, 1.43)
    assert np.array_equal(a["samp"], b["samp"])
    assert R.model(g, 100.0, 2.0, 1.43)["dfwhm"] > a["dfwhm"]


def test_validity_follows_the_profile_window():
    g = R.Grid()
    assert not R.model(g, 60.0, 0.0, 2.2)["valid"]
    assert R.model(g, 100.0, 0.0, 1.43)["valid"]
    assert R.model(g, np.inf, 0.0, 2.2)["valid"]


def test_ctypes_mirrors_match_the_header():
    from lfd_amd import _native
    assert C.sizeof(_native.DefocusParams) == 5 * 8 + 6 * 4 + 3 * 8 + 8 == 96
    assert _native.DEFOCUS_MODEL_DTYPE.itemsize == 56
    assert _native.DEFOCUS_DTYPE.itemsize == 4 * 4 + 11 * 8
    with open(os.path.join(ROOT, "include", "lfdmi.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    def fields(name):
        body = re.search(r"typedef struct \{([^{}]*?)\} " + name + ";", text, re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [re.sub(r"^\*", "", x.strip().split()[-1]) for x in decl.split(",")]
        return out

    assert fields("lfdmi_defocus_params") == [k for k, _ in _native.DefocusParams._fields_]
    assert fields("lfdmi_defocus_fit") == list(_native.DEFOCUS_DTYPE.names)
    assert fields("lfdmi_defocus_model") == list(_native.DEFOCUS_MODEL_DTYPE.names)


def test_default_params():
    from lfd_amd import defocus
    d = defocus.default_params()
    assert len(d["heights"]) == 128 and d["heights"][0] == 60.0 and d["heights"][-1] == pytest.approx(300.0, rel=1e-12)
    assert np.allclose(np.diff(np.log(d["heights"])), math.log(5) / 127)
    assert list(d["radii"]) == [0, 0.1, 0.5, 1, 2, 5, 10]
    assert len(d["seeings"]) == 29 and d["seeings"][0] == 0.8 and d["seeings"][-1] == pytest.approx(2.2)
    assert d["instrument"] == defocus.SDSS == (1250.0, 585.0)
    assert (d["ovs"], d["max_shift"], d["delta_chi2"]) == (8, 5, 10.0)
    assert (d["pixscale"], d["prof_half"], d["prof_step"], d["wing"]) == (0.396, 24.0, 0.1, 8)
    assert defocus.LSST == (4180.0, 2558.0) and defocus.SDSSSEEING == 1.43 and defocus.LSSTSEEING == 0.67
    assert defocus.RAD2ARCSEC == R.RAD2ARCSEC and defocus.FWHM2SIGMA == R.FWHM2SIGMA


def test_parameter_checks_raise():
    from lfd_amd import _native, defocus
    with pytest.raises(TypeError):
        defocus.make_params(no_such_param=1)
    with pytest.raises(ValueError):
        defocus.make_params(heights=[])
    p, keep = defocus.make_params(heights=[90.0, 110.0], radii=[0.0], seeings=[1.2], instrument=defocus.LSST, prof_step=0.2)
    assert (p.n_h, p.n_r, p.n_seeing, p.Ro, p.Ri, p.prof_step, p.delta_chi2) == (2, 1, 1, 4180.0, 2558.0, 0.2, 5.0)
    assert p.heights[1] == 110.0
    # without a GPU the library refuses the context, so no bank can be built on the CPU
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeError):
            _native.Context(0, 64, 64, 1)


def test_grid_has_the_sampler_fields():
    from lfd_amd import defocus
    assert defocus.GRID_DTYPE.names == ("h", "radius", "sfwhm", "dfwhm", "ofwhm", "depth", "valid")


def test_defocus_rows_round_trip(tmp_path):
    from lfd_amd import _native, defocus
    fit = np.zeros(3, _native.DEFOCUS_DTYPE)
    fit["status"] = [0, 4, 1]
    fit["h_km"] = [101.25, np.nan, np.nan]
    fit["h_lo"], fit["h_hi"] = [90.0, np.nan, np.nan], [np.inf, np.nan, np.nan]
    fit["shift"], fit["dof"] = [-3, 0, 0], [479, 0, 0]
    fit["chi2"] = [1 / 3, np.nan, np.nan]
    meta = [(94, 1, "r", 12), (94, 1, "r", 13), (1000, 6, "i", 400)]
    path = tmp_path / "defocus.txt"
    with open(path, "w") as f:
        f.write(" ".join(defocus.DEFOCUS_COLUMNS) + "\n")
        for m, r in zip(meta, fit):
            f.write(defocus.format_row(m, r) + "\n")
    rows = defocus.read_defocus(path)
    assert len(rows) == 3
    for m, r, row in zip(meta, fit, rows):
        assert (row["run"], row["camcol"], row["filter"], row["field"]) == m
        for k in defocus.DEFOCUS_COLUMNS[4:]:
            a, b = row[k], r[k].item()
            assert a == b or (math.isnan(a) and math.isnan(b)), k
    assert "-3 " in open(path).read().splitlines()[1] and "0.3333333333333333" in open(path).read()


# ---- the inputs of tests/test_gpu_defocus_shapes.py: their conditions hold by the restatement alone --------------------------
import defocus_cases as DC  # noqa: E402

NON_DECISIVE_CAP = 0.25


@pytest.mark.parametrize("name", list(DC.GEOMS))
def test_shape_geometries_meet_their_conditions(name):
    """the tile property each geometry is there for, a valid and an invalid model in every bank, and at most a quarter of the
    fitted rows non-decisive (a row is decisive when the acceptance rule leaves the device one column to return)"""
    rb, trails, prof = DC.fit_inputs(name)
    facts = DC.tile_facts(rb)
    for k, v in DC.GEOMS[name]["expect"].items():
        assert facts[k] == v, (k, facts[k], v)
    assert DC.PROPERTIES[name](facts), facts
    assert 0 < facts["n_valid"] < facts["n_models"]
    share, J = DC.non_decisive_share(rb, trails, prof)
    band = int((~J["must_ok"] & ~J["must_none"]).sum())
    print(f"{name}: non-decisive share {share:.3f}, rows where either status is accepted {band}, NO_MODEL required "
          f"{int(J['must_none'].sum())} of {len(prof)}")
    assert share <= NON_DECISIVE_CAP
    assert J["must_ok"].sum() >= len(prof) // 2


def test_largest_geometry_is_largest_by_groups_and_padded_bins():
    facts = {n: DC.tile_facts(DC.restated(n)) for n in DC.GEOMS}
    assert all(facts[DC.LARGEST][k] >= f[k] for f in facts.values() for k in ("n_groups", "nbp"))


def test_row_test_inputs_meet_the_cap():
    rb = DC.restated("two_k_steps")
    for n, seed in ((127, 134), (128, 135), (129, 136), (4096, 4103), (300, 21), (128, 31)):
        share, _ = DC.non_decisive_share(rb, *DC.make_rows(rb, n, seed)[:2])
        assert share <= NON_DECISIVE_CAP, (n, share)
    for seeings in ([1.0, 2.0], [2.0, 1.0], [1.0, 1.0, 2.0]):
        rv = DC.restate(DC.variant("two_k_steps", seeings=seeings))
        share, _ = DC.non_decisive_share(rv, *DC.make_rows(rv, 200, 41)[:2])
        assert share <= NON_DECISIVE_CAP, (seeings, share)


def test_tie_rows_are_decisive_and_name_the_lowest_copy():
    for name, (ge, rb, trails, prof, want) in DC.tie_cases().items():
        J = R.judge(rb, trails, prof)
        assert J["decisive"].all() and J["must_ok"].all(), name
        assert np.array_equal(J["want"], want), name
        dup = np.bincount(rb.cls[rb.vcol])
        assert dup.max() >= 2, name     # the bank does hold bit-identical valid columns


def test_seeing_slice_rule():
    assert [R.seeing_slice([1.0, 2.0], s) for s in (0.9, 1.5, 1.6, np.nan)] == [0, 0, 1, None]
    assert R.seeing_slice([2.0, 1.0], 1.5) == 1 and R.seeing_slice([1.0, 1.0, 2.0], 1.1) == 0


def test_score_bound_covers_float32_dot_products_in_any_order():
    """the derived bound against float32 sums in ascending, descending, pairwise and random order, and against the rounded v~"""
    rng = np.random.default_rng(0)
    rb = DC.restated("fractional_F")
    trails, prof, _ = DC.make_rows(rb, 40, 9)
    vt = R.centre(prof, rounded=True)
    assert np.array_equal(vt, vt.astype(np.float32)) and not np.array_equal(vt, R.centre(prof))
    e = R.score_bound(rb.nbp, vt)
    cols = np.flatnonzero(rb.vcol)[::7]
    exact = vt @ rb.c64[cols].T
    worst = 0.0
    for order in (np.arange(rb.nb), np.arange(rb.nb)[::-1], rng.permutation(rb.nb)):
        acc = np.zeros(exact.shape, np.float32)
        for k in order:
            acc = (acc + (vt[:, k, None].astype(np.float32) * rb.c32[cols][None, :, k]).astype(np.float32)).astype(np.float32)
        worst = max(worst, float((np.abs(acc - exact) / e[:, None]).max()))
    pair = (vt.astype(np.float32)[:, None, :] * rb.c32[cols][None]).sum(axis=2, dtype=np.float32)
    worst = max(worst, float((np.abs(pair - exact) / e[:, None]).max()))
    assert 0 < worst <= 1.0, worst
