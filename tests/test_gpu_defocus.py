"""The defocus bank and fit on the device against the numpy restatement of include/lfdmi.h (tests/defocus_ref.py): the bank's
columns within 1 float32 ulp, the fit's choice at the restatement's minimum, the documented statuses, the seeing slice, and the
recovery of the height of rendered trails end to end (measure_trails, then fit_defocus)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defocus_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

HEIGHTS = [60.0, 80.0, 100.0, 130.0, 200.0]
RADII = [0.0, 0.5, 2.0]
SEEINGS = [0.9, 1.43, 2.0]


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2**31) - ai, ai)
    bi = np.where(bi < 0, np.int64(-2**31) - bi, bi)
    return np.abs(ai - bi)


def rel_same(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (a == b) | (np.abs(a - b) <= tol * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


@pytest.fixture(scope="module")
def small():
    from lfd_amd import _native, defocus
    ctx = _native.Context(0, 1489, 2048, 8)
    bank = defocus.DefocusBank(ctx, heights=HEIGHTS, radii=RADII, seeings=SEEINGS)
    g = R.Grid()
    c32, c64, models = R.bank(g, HEIGHTS, RADII, SEEINGS)
    yield ctx, bank, g, c32, c64, models
    bank.close()
    ctx.close()


def test_bank_equals_the_restatement(small):
    ctx, bank, g, c32, c64, models = small
    cols = bank.columns()
    assert cols.shape == c32.shape
    ns = 2 * g.S + 1
    valid = np.array([m["valid"] for m in models])
    grid = bank.grid
    assert np.array_equal(grid["valid"], valid)
    assert valid.any() and not valid.all()
    vcol = np.repeat(valid, ns)
    assert ulp_diff(cols[vcol], c32[vcol]).max() <= 1
    assert not cols[~vcol].any()
    for k, rk in (("dfwhm", "dfwhm"), ("ofwhm", "ofwhm"), ("depth", "depth")):
        assert rel_same(grid[k], [m[rk] for m in models], 1e-9), k
    assert np.array_equal(grid["h"], [m["h"] for m in models])
    assert np.array_equal(grid["radius"], [m["R"] for m in models])
    assert np.array_equal(grid["sfwhm"], [m["seeing"] for m in models])


_MEAS = {}


def measured(n=256):
    if n in _MEAS:
        return _MEAS[n]
    from lfd_amd import _native, synth
    from lfd_amd.detecttrails import default_params
    pb, pd, prs = default_params()
    frames, cats = zip(*[synth.make_frame(k)[:2] for k in range(n)])
    frames = np.stack(frames)
    packed = synth.pack_catalogs(list(cats))
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    with _native.Context(0, *synth.SDSS_SHAPE, 16) as ctx:
        recs = ctx.detect_batch(frames, pb, pd, packed, rs)
        out, prof = ctx.measure_trails(frames, recs, packed, rs)
    _MEAS[n] = (out, prof)
    return _MEAS[n]


def test_fit_equals_the_restatement(small):
    from lfd_amd import _native
    ctx, bank, g, c32, c64, models = small
    trails, prof = measured(256)
    trails, prof = trails.copy(), prof.copy()
    ok = np.flatnonzero(trails["status"] == _native.TRAIL_OK)
    assert len(ok) >= 100
    gap, quiet = ok[0], ok[1]
    prof[gap, 7] = np.nan
    trails["noise"][quiet] = 0.0
    fit, cbh = ctx.fit_defocus(bank, trails, prof, chi2_by_height=True)
    for i in range(len(trails)):
        if trails["status"][i] != _native.TRAIL_OK:
            assert fit["status"][i] == _native.DEFOCUS_NOT_MEASURED and math.isnan(fit["chi2"][i]), i
            assert np.isnan(cbh[i]).all()
    assert fit["status"][gap] == _native.DEFOCUS_GAPS and math.isnan(fit["h_km"][gap])
    assert fit["status"][quiet] == _native.DEFOCUS_NO_NOISE and fit["column"][quiet] == -1
    checked = 0
    for i in ok:
        if i in (gap, quiet):
            continue
        chi2, curve = R.fit(g, c64, models, len(HEIGHTS), SEEINGS, trails[i], prof[i])
        f = fit[i]
        if np.isnan(chi2).all():
            assert f["status"] == _native.DEFOCUS_NO_MODEL
            continue
        assert f["status"] == _native.DEFOCUS_OK, (i, f)
        cmin = np.nanmin(chi2)
        col = f["column"]
        assert chi2[col] <= cmin + 1e-4 * abs(cmin), (i, chi2[col], cmin)
        assert rel_same(f["chi2"], chi2[col], 1e-6), (i, f["chi2"], chi2[col])
        m = models[col // (2 * g.S + 1)]
        assert (f["h_km"], f["radius_m"], f["seeing_arcsec"], f["shift"]) == (m["h"], m["R"], m["seeing"], col % (2 * g.S + 1) - g.S)
        assert f["dof"] == 2 * g.K - 1
        assert rel_same(f["model_ofwhm"], m["ofwhm"], 1e-9) and rel_same(f["model_depth"], m["depth"], 1e-9)
        # chi2 by height from float32 scores: close to the double restatement
        scale = float(np.nansum((prof[i] - prof[i].mean()) ** 2) / trails["noise"][i] ** 2)
        assert np.array_equal(np.isnan(cbh[i]), np.isnan(curve))
        assert np.nanmax(np.abs(cbh[i] - curve)) <= 1e-5 * scale + 1e-3, (i, cbh[i], curve)
        assert abs(f["chi2_focus"] - curve[-1]) <= 1e-5 * scale + 1e-3
        cm, lo, hi = R.interval(curve, HEIGHTS, bank.delta_chi2)
        if (f["h_lo"], f["h_hi"]) != (lo, hi):  # only where a height's value lies on the threshold within float32 rounding
            hs = np.array(HEIGHTS + [np.inf])
            for h in (f["h_lo"], f["h_hi"], lo, hi):
                j = int(np.flatnonzero(hs == h)[0])
                if h not in (lo, hi) or h not in (f["h_lo"], f["h_hi"]):
                    assert abs(curve[j] - (cm + bank.delta_chi2)) <= 1e-5 * scale + 1e-3, (i, f, lo, hi)
        checked += 1
    assert checked >= 100


def test_fixed_seeing_restricts_the_fit_to_its_slice(small):
    from lfd_amd import _native
    ctx, bank, g, c32, c64, models = small
    trails, prof = measured(256)
    ok = np.flatnonzero(trails["status"] == _native.TRAIL_OK)[:40]
    seeing = np.full(len(trails), np.nan, np.float32)
    seeing[ok[:20]] = 1.5      # nearest: 1.43
    seeing[ok[20:]] = 1.2      # nearest: 1.43
    fit = ctx.fit_defocus(bank, trails, prof, seeing=seeing)
    free = ctx.fit_defocus(bank, trails, prof)
    for i in ok:
        assert fit["status"][i] == _native.DEFOCUS_OK
        assert fit["seeing_arcsec"][i] == 1.43
        chi2, _ = R.fit(g, c64, models, len(HEIGHTS), SEEINGS, trails[i], prof[i], seeing=float(seeing[i]))
        cmin = np.nanmin(chi2)
        assert chi2[fit["column"][i]] <= cmin + 1e-4 * abs(cmin)
        assert fit["chi2"][i] >= free["chi2"][i] * (1 - 1e-9)
    rest = np.setdiff1d(np.flatnonzero(trails["status"] == _native.TRAIL_OK), ok)
    assert np.array_equal(fit["column"][rest], free["column"][rest])


def test_bank_refuses_bad_params():
    from lfd_amd import _native, defocus
    with _native.Context(0, 64, 64, 1) as ctx:
        for kw in ({"heights": [-1.0]}, {"seeings": [0.0]}, {"radii": [np.nan]}, {"instrument": (500.0, 600.0)},
                   {"prof_step": 0.07}, {"wing": 24}):
            with pytest.raises(_native.NativeError):
                defocus.DefocusBank(ctx, **kw)
        # the context stays usable, and a bank of another context is refused
        b = defocus.DefocusBank(ctx, heights=[100.0], radii=[0.0], seeings=[1.4])
        with _native.Context(0, 64, 64, 1) as other:
            with pytest.raises(ValueError):
                other.fit_defocus(b, np.zeros(1, _native.TRAIL_DTYPE), np.zeros((1, b.n_bins), np.float32))
        b.close()


def test_a_bank_may_outlive_its_context():
    """Context.close() closes the context's banks first; a closed bank refuses reads and closes again harmlessly"""
    from lfd_amd import _native, defocus
    with _native.Context(0, 64, 64, 1) as ctx:
        b = defocus.DefocusBank(ctx, heights=[100.0], radii=[0.0], seeings=[1.4])
        kept = defocus.DefocusBank(ctx, heights=[120.0], radii=[0.0], seeings=[1.4])
        assert b.columns().shape == (b.n_columns, b.n_bins)
        b.close()
    assert not kept._b
    with pytest.raises(ValueError):
        kept.columns()
    kept.close()
    del kept


# ---- recovery end to end ----------------------------------------------------------------------------------------------------
def physical_profile(g, h, fwhm):
    """O (x) D (x) S on the fine grid (what the sky shows, before the pixel): (values, half-width in fine steps)"""
    o = np.ones(1) if not np.isfinite(h) else R.od(g, h, 0.0)
    y = np.convolve(o, R.unit(R.seeing_raw(fwhm, g.delta)))
    return y, (len(y) - 1) // 2


def render(g, h, fwhm, theta, rho, rng, shape=(1489, 2048), peak=2.0, sky=1.0):
    """a trail along x cos(theta) + y sin(theta) = rho of the flipped frame (buffer row H-1-y), the model at the signed
    distance averaged over 8 x 8 sub-pixel points, peak `peak` sky sigmas, plus Gaussian sky noise"""
    H, W = shape
    y, c = physical_profile(g, h, fwhm)
    xs = (np.arange(len(y)) - c) * g.delta / g.pixscale  # px
    img = rng.normal(0.0, sky, shape).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    fy = (H - 1 - yy).astype(np.float64)
    ct, st = math.cos(theta), math.sin(theta)
    d0 = xx * ct + fy * st - rho
    near = np.abs(d0) < xs[-1] + 2
    acc = np.zeros(near.sum())
    sub = (np.arange(8) + 0.5) / 8 - 0.5
    dn = d0[near]
    for a in sub:
        for b in sub:   # column offset a, buffer-row offset b (flipped y offset -b)
            acc += np.interp(dn + a * ct - b * st, xs, y, left=0.0, right=0.0)
    acc /= 64
    img[near] += acc * (peak * sky / acc.max())
    return img.astype(np.float32)


def test_recovery_of_rendered_trails():
    from lfd_amd import _native, defocus
    g = R.Grid()
    rng = np.random.default_rng(7)
    cases = []
    for h in (80.0, 100.0, 150.0, np.inf):
        for theta in (0.35, 1.2, 2.4):
            cases.append((h, theta))
    frames, recs = [], np.zeros(len(cases), _native.RESULT_DTYPE)
    for k, (h, theta) in enumerate(cases):
        th = float(np.float32(theta))
        rho = float(np.float32(1024 * math.cos(th) + 744 * math.sin(th)))  # through the frame's centre
        frames.append(render(g, h, 1.43, th, rho, rng))
        recs[k]["found"] = 1
        recs[k]["rho"], recs[k]["theta"] = rho, th
    frames = np.stack(frames)
    with _native.Context(0, 1489, 2048, 4) as ctx:
        trails, prof = ctx.measure_trails(frames, recs)
        assert (trails["status"] == _native.TRAIL_OK).all(), trails["status"]
        assert (trails["n_pos"] >= 1000).all()
        # the default grid with the true heights added, so that h_lo <= h <= h_hi can hold exactly
        heights = np.union1d(defocus.default_params()["heights"], [80.0, 100.0, 150.0])
        with defocus.DefocusBank(ctx, heights=heights) as bank:
            fit = ctx.fit_defocus(bank, trails, prof)
            dchi = bank.delta_chi2
    report = "\n".join("h %s theta %s: h_fit %.2f [%.2f, %.2f] seeing %.2f chi2 %.1f chi2_focus %.1f" % (
        h, th, f["h_km"], f["h_lo"], f["h_hi"], f["seeing_arcsec"], f["chi2"], f["chi2_focus"]) for (h, th), f in zip(cases, fit))
    print(report)
    # the seeing of the one known outlier, measured and reported in include/lfdmi.h ("defocus fit": recovery)
    outlier = {(150.0, 2.4): 0.30}
    # the known cases whose interval (delta_chi2 = 1 / prof_step) misses the true height: the fit lands on the next grid
    # height, 0.4-0.9 % off, and the interval is narrower than that step (measured, reported in include/lfdmi.h)
    interval_misses = {(100.0, 0.35), (150.0, 1.2), (150.0, 2.4)}
    for (h, theta), f in zip(cases, fit):
        assert f["status"] == _native.DEFOCUS_OK, report
        if np.isfinite(h):
            assert abs(f["h_km"] - h) / h <= 0.10, report
            if (h, theta) in interval_misses:
                assert abs(f["h_km"] - h) / h <= 0.01 and not f["h_lo"] <= h <= f["h_hi"], report
            else:
                assert f["h_lo"] <= h <= f["h_hi"], report
            assert abs(f["seeing_arcsec"] - 1.43) <= outlier.get((h, theta), 0.15), report
            assert f["chi2_focus"] - f["chi2"] >= 100, report
        else:
            assert f["h_hi"] == np.inf, report
            assert f["chi2_focus"] - f["chi2"] <= dchi, report
