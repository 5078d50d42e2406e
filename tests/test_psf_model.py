"""What the frame seeing measures, on the restatement (tests/psf_ref.py, after tests/stars_ref.py), with the default parameters:
372 x 512 frames of sky sigma 0.025 with Gaussian stars of sigma 1.0, 1.5, 2.0 and 3.0 px, noise alone, a bright streak, and
stars rendered with the defocus bank's PSF.  Each asserted bound is the extreme measured here plus a quarter of it, as
tests/test_sub_model.py has it; ``python tests/test_psf_model.py`` prints the figures (README: frame seeing)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as R  # noqa: E402
import stars_ref as S  # noqa: E402

SHAPE = (372, 512)
SIGMA = 0.025
PIXSCALE = 0.396
N_STAR = 60
STAR_SIGMAS = (1.0, 1.5, 2.0, 3.0)
BANK_SEEINGS = (1.0, 1.4, 2.0)                             # of the default grid 0.8 .. 2.2 in steps of 0.05
GRID = np.arange(0.8, 2.2 + 1e-9, 0.05)
# the extremes measured (below) plus a quarter
# |fwhm_px / (2.3548 sigma) - 1|: measured +0.00045, -0.00019, -0.00138 and -0.04689 (at 3 px the window of half-width 7 cuts
# the wings at 2.3 sigma)
GAUSS_BOUND = {1.0: 0.00045 * 1.25, 1.5: 0.00019 * 1.25, 2.0: 0.00138 * 1.25, 3.0: 0.04689 * 1.25}
BANK_BOUND = 0.00367 * 1.25                                # |to_bank_seeing - truth|, arcsec: measured 0.00039, 0.00021, 0.00367


def sky(seed):
    return np.random.default_rng(seed).normal(0.0, SIGMA, SHAPE).astype(np.float32)


def gauss_frame(sig, seed):
    from lfd_amd import synth
    rng = np.random.default_rng(seed)
    img = sky(seed + 1000)
    ys, xs = rng.uniform(0, SHAPE[0], N_STAR), rng.uniform(0, SHAPE[1], N_STAR)
    synth._add_stars(img, ys, xs, np.exp(rng.uniform(np.log(50.0), np.log(2000.0), N_STAR)), sig)
    return img


def bank_frame(seeing, seed):
    from lfd_amd import psf
    rng = np.random.default_rng(seed)
    img = sky(seed + 1000)
    half = 14
    for _ in range(N_STAR):
        y, x = rng.uniform(half + 1, SHAPE[0] - half - 2), rng.uniform(half + 1, SHAPE[1] - half - 2)
        iy, ix = int(round(y)), int(round(x))
        flux = np.exp(rng.uniform(np.log(50.0), np.log(2000.0)))
        img[iy - half:iy + half + 1, ix - half:ix + half + 1] += (flux * psf.render_bank_psf(seeing, PIXSCALE, half, y - iy, x - ix)).astype(np.float32)
    return img


def measure(img):
    out, fr, rec, frec = R.measure_seeing(img[None], SIGMA)
    return out[0], fr[0], rec[0], frec[0]


@functools.lru_cache(maxsize=None)
def gauss_figures():
    return {sig: measure(gauss_frame(sig, 100 + k))[1] for k, sig in enumerate(STAR_SIGMAS)}


@functools.lru_cache(maxsize=None)
def bank_figures():
    return {s: measure(bank_frame(s, 200 + k))[1] for k, s in enumerate(BANK_SEEINGS)}


def test_gaussian_stars_give_their_width():
    for sig, fr in gauss_figures().items():
        err = float(fr["fwhm_px"]) / (2.3548 * sig) - 1.0
        print("sigma %.1f px: n_cand %d n_ok %d n_used %d fwhm_px %.4f (2.3548 sigma %.4f, %+.4f) scatter %.4f ell %.4f"
              % (sig, fr["n_cand"], fr["n_ok"], fr["n_used"], fr["fwhm_px"], 2.3548 * sig, err, fr["scatter"], fr["ell"]))
        assert fr["status"] == R.SEEING_OK and fr["n_used"] >= 10
        assert abs(err) <= GAUSS_BOUND[sig], (sig, err)


def test_noise_alone_has_no_candidate():
    for seed in (1, 2, 3):
        _, fr, _, _ = measure(sky(seed))
        assert fr["n_cand"] == 0 and fr["status"] == R.SEEING_FEW and np.isnan(fr["fwhm_px"])


def test_no_ridge_maximum_of_a_streak_is_used():
    from lfd_amd import synth
    img = gauss_frame(1.5, 300)
    clean = measure(img)[1]
    synth._add_streak(img, 180.0, 250.0, 30.0, 2.0, 2.0)
    out, fr, rec, frec = measure(img)
    ext = rec[:frec["n_out"]]["flags"] & S.EXTENDED
    assert np.count_nonzero(ext) >= 20                     # the ridge's maxima are there, and flagged
    used = rec[out[:fr["n_packed"]]["index"]]
    assert not (used["flags"] != 0).any()
    d = (used["x"] - 250.0) * np.sin(np.deg2rad(30.0)) - (used["y"] - 180.0) * np.cos(np.deg2rad(30.0))
    # nor a star that sits on the streak: the ridge's maxima lie at most 2 sep + 1 = 7 px apart along it, so a peak within
    # sqrt(12^2 - 4.5^2) - 1 > 10 px of the line has one of them within iso = 12 and is CROWDED
    assert np.abs(d).min() > 10
    print("streak: fwhm_px %.4f, without it %.4f" % (fr["fwhm_px"], clean["fwhm_px"]))


def test_bank_stars_give_the_bank_seeing():
    from lfd_amd import psf
    for s, fr in bank_figures().items():
        got = psf.to_bank_seeing(float(fr["fwhm_px"]), PIXSCALE, 7, GRID)
        print("seeing %.2f\": n_used %d fwhm_px %.4f (%.4f\") -> bank seeing %.4f\" (%+.4f)"
              % (s, fr["n_used"], fr["fwhm_px"], fr["fwhm_px"] * PIXSCALE, got, got - s))
        assert fr["status"] == R.SEEING_OK
        assert abs(got - s) <= BANK_BOUND, (s, got)


def test_to_bank_seeing_inverts_its_own_table():
    """the noise-free round trip: the bank's PSF at a seeing, measured, lands within half a grid step (0.025") of it"""
    from lfd_amd import psf
    grid = np.arange(0.8, 2.2 + 1e-9, 0.05)
    tab = psf.bank_table(0.396, 7, grid)
    assert np.all(np.diff(tab) > 0)
    for s in (0.8, 1.0, 1.23, 1.4, 1.77, 2.2):
        w = psf.stamp_fwhm(psf.render_bank_psf(s, 0.396, 12), 7)
        assert abs(psf.to_bank_seeing(w, 0.396, 7, grid) - s) <= 0.025, s
    # the relation is not that of an untruncated Gaussian sampled at points: the pixel widens, the window truncates
    w = psf.stamp_fwhm(psf.render_bank_psf(1.4, 0.396, 12), 7)
    assert abs(w * 0.396 - 1.4) > 0.01
    # clamped at the ends, NaN stays NaN, arrays go through
    got = psf.to_bank_seeing(np.array([0.1, np.nan, 50.0]), 0.396, 7, grid)
    assert got[0] == grid[0] and np.isnan(got[1]) and got[2] == grid[-1]
    assert np.isnan(psf.to_bank_seeing(float("nan"), 0.396, 7, grid))


def test_the_150_km_case_with_free_and_with_pinned_seeing():
    """Recorded, not asserted: the header's hard case (include/lfdmi.h, defocus fit: 150 km, where defocus and seeing widen the
    profile alike) through tests/defocus_ref.py.  The profile is the model without the pixel and the bilinear triangle, as the
    header's recovery renders it, at seeing 1.4", with noise of 2 % of its peak; the bank has the default seeings, 25 geometric
    heights 60 .. 300 km plus the true one, and the point object.  The fit runs with the seeing free and with it pinned to
    what ``to_bank_seeing`` gives for stars of that seeing (test_bank_stars_give_the_bank_seeing)."""
    import defocus_ref as D
    from lfd_amd import psf
    g = D.Grid()
    hs = sorted(set(np.geomspace(60.0, 300.0, 25).tolist() + [150.0]))
    _, cols64, models = D.bank(g, hs, (0.0,), GRID)
    o = D.od(g, 150.0, 0.0)
    sraw = D.unit(D.seeing_raw(1.4, g.delta))
    M = np.convolve(o, sraw)
    c = (len(M) - 1) // 2
    idx = (np.arange(2 * g.K + 1) - g.K) * g.ovs + c
    v = np.where((idx >= 0) & (idx < len(M)), M[np.clip(idx, 0, len(M) - 1)], 0.0)
    v = v / v.max()
    noise = 0.02
    v = v + np.random.default_rng(150).normal(0.0, noise, v.shape)
    measured = psf.to_bank_seeing(float(bank_figures()[1.4]["fwhm_px"]), PIXSCALE, 7, GRID)
    ns = 2 * g.S + 1
    for name, see in (("free", None), ("pinned", measured)):
        chi2, curve = D.fit(g, cols64, models, len(hs), GRID, {"noise": noise}, v, seeing=see)
        m = models[int(np.nanargmin(chi2)) // ns]
        cmin, lo, hi = D.interval(curve, hs, 1.0 / g.step)
        print("150 km, seeing 1.40\", %s%s: h %.1f km [%.1f, %.1f], seeing %.2f\", chi2 %.1f"
              % (name, "" if see is None else " at %.4f\"" % see, m["h"], lo, hi, m["seeing"], cmin))
        assert np.isfinite(cmin)


if __name__ == "__main__":
    test_gaussian_stars_give_their_width()
    test_bank_stars_give_the_bank_seeing()
    test_the_150_km_case_with_free_and_with_pinned_seeing()
