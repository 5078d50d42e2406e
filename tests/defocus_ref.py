"""numpy restatement of the defocus model, bank and fit of include/lfdmi.h ("defocus fit"), all in double.  The components
follow lfd/analysis/profiles (defocusing.py Eq. 6, objectprofiles.py's disk, seeing.py's Gaussian) as the header states them."""
import math

import numpy as np

RAD2ARCSEC = 206264.806247
FWHM2SIGMA = 2.436


class Grid:
    """The fine grid of a bank: delta arcsec per step, F steps per px, K bins each side, S shifts."""

    def __init__(self, pixscale=0.396, prof_half=24.0, prof_step=0.1, wing=8, ovs=8, max_shift=5, instrument=(1250., 585.)):
        self.pixscale, self.P, self.step, self.wing, self.ovs, self.S = pixscale, prof_half, prof_step, wing, ovs, max_shift
        self.Ro, self.Ri = instrument
        self.K = int(round(prof_half / prof_step))
        self.delta = prof_step * pixscale / ovs
        self.F = ovs / prof_step
        self.jcap = self.K * ovs


def unit(w):
    return w / w.sum()


def defocus_raw(to, ti, delta):
    """D(x_j) over |j| <= floor(theta_o / delta), not normalised"""
    n = int(math.floor(to / delta))
    x = np.arange(-n, n + 1) * delta
    outer = np.sqrt(np.maximum(to * to - x * x, 0.0))
    inner = np.where(np.abs(x) < ti, np.sqrt(np.maximum(ti * ti - x * x, 0.0)), 0.0)
    return 2.0 / (math.pi * (to * to - ti * ti)) * (outer - inner)


def disk_raw(rho, delta):
    n = int(math.floor(rho / delta))
    x = np.arange(-n, n + 1) * delta
    return 2.0 * np.sqrt(np.maximum(rho * rho - x * x, 0.0)) / (math.pi * rho * rho)


def seeing_raw(fwhm, delta):
    sigma = 1.035 / FWHM2SIGMA * fwhm
    n = int(math.floor(4 * sigma / delta))
    x = np.arange(-n, n + 1) * delta
    return np.exp(-(x * x) / (2 * sigma * sigma))


def box_raw(F):
    n = int(math.ceil(F / 2 - 0.5))
    j = np.arange(-n, n + 1, dtype=np.float64)
    return np.maximum(0.0, np.minimum(j + 0.5, F / 2) - np.maximum(j - 0.5, -F / 2))


def tri_raw(F):
    n = int(math.ceil(F)) - 1
    j = np.arange(-n, n + 1, dtype=np.float64)
    return 1.0 - np.abs(j) / F


def angles(g, h, R):
    """(theta_o, theta_i, rho) in arcsec; h = inf: all 0"""
    if not np.isfinite(h):
        return 0.0, 0.0, 0.0
    return g.Ro / (h * 1e6) * RAD2ARCSEC, g.Ri / (h * 1e6) * RAD2ARCSEC, R / (2 * h * 1000) * RAD2ARCSEC


def od(g, h, R):
    """O (x) D on the fine grid (normalised components), or None when its half-width exceeds K ovs"""
    to, ti, rho = angles(g, h, R)
    point = (not np.isfinite(h)) or R == 0
    nD = int(math.floor(to / g.delta))
    nO = 0 if point else int(math.floor(rho / g.delta))
    if nD + nO > g.jcap:
        return None
    D = np.ones(1) if not np.isfinite(h) else unit(defocus_raw(to, ti, g.delta))
    O = np.ones(1) if point else unit(disk_raw(rho, g.delta))
    return np.convolve(O, D)


def kernel(g, fwhm):
    """(S (x) B) (x) T"""
    return np.convolve(np.convolve(unit(seeing_raw(fwhm, g.delta)), unit(box_raw(g.F))), unit(tri_raw(g.F)))


def fwhm_rule(y, c, dx):
    peak = y.max()
    idx = np.nonzero(y >= peak / 2)[0]
    l, r = idx[0], idx[-1]
    return 0.0 if l == r else abs((r - c) * dx) + abs((l - c) * dx)


def model(g, h, R, fwhm):
    """dict: samp (2K+2S+1 samples, None when OD does not fit), valid, dfwhm, ofwhm, depth"""
    to, ti, rho = angles(g, h, R)
    sigma = 1.035 / FWHM2SIGMA * fwhm
    o = od(g, h, R)
    valid = o is not None and (to + rho) / g.pixscale + 4 * sigma / g.pixscale + 1 + g.S * g.step <= g.P - g.wing
    if o is None:
        return {"samp": None, "valid": False, "dfwhm": np.nan, "ofwhm": np.nan, "depth": np.nan}
    hw = (len(o) - 1) // 2
    ks = kernel(g, fwhm)
    nk = (len(ks) - 1) // 2
    M = np.convolve(o, ks)
    c = hw + nk
    q = np.arange(2 * g.K + 2 * g.S + 1)
    idx = (q - g.K - g.S) * g.ovs + c
    ok = (idx >= 0) & (idx < len(M))
    samp = np.where(ok, M[np.clip(idx, 0, len(M) - 1)], 0.0)
    v = samp[g.S:g.S + 2 * g.K + 1]
    return {"samp": samp, "valid": bool(valid), "dfwhm": fwhm_rule(o, hw, g.delta),
            "ofwhm": fwhm_rule(v, g.K, g.step * g.pixscale), "depth": (v.max() - v[g.K]) / v.max() * 100.0}


def column(g, samp, s):
    """the double column of shift s (centred, unit norm) and its un-normalised samples t"""
    t = samp[g.S - s:g.S - s + 2 * g.K + 1]
    c = t - t.mean()
    return c / np.sqrt((c * c).sum()), t


def bank(g, heights, radii, seeings):
    """restated bank: float32 columns [n_col, 2K+1] (0 for invalid models), double columns, models (list of dicts with h, R,
    seeing), in the header's index order"""
    hs = list(heights) + [np.inf]
    ns = 2 * g.S + 1
    nb = 2 * g.K + 1
    models, cols64 = [], []
    for fw in seeings:
        for h in hs:
            for R in radii:
                m = model(g, h, R, fw)
                m.update(h=h, R=R, seeing=fw)
                models.append(m)
                for s in range(-g.S, g.S + 1):
                    if m["valid"]:
                        cols64.append(column(g, m["samp"], s)[0])
                    else:
                        cols64.append(np.zeros(nb))
    cols64 = np.array(cols64)
    assert cols64.shape == (len(models) * ns, nb)
    return cols64.astype(np.float32), cols64, models


def fit(g, cols64, models, n_h, seeings, trail, v, seeing=None, delta_chi2=None):
    """chi2 of every column in double (least squares a, b; NaN for columns not allowed), and the per-height curve, chi2_min,
    h_lo, h_hi, chi2_focus as the header defines them (from double scores)"""
    delta_chi2 = 1.0 / g.step if delta_chi2 is None else delta_chi2
    v = np.asarray(v, np.float64)
    vt = v - v.mean()
    nz2 = trail["noise"] ** 2
    ns = 2 * g.S + 1
    allowed = np.repeat(np.array([m["valid"] for m in models]), ns)
    if seeing is not None and np.isfinite(seeing):
        d = np.abs(np.asarray(seeings) - seeing)
        best = min(range(len(seeings)), key=lambda j: (d[j], seeings[j]))
        allowed &= np.repeat(np.array([m["seeing"] == seeings[best] for m in models]), ns)
    c = cols64 @ vt
    chi2 = np.where(allowed, ((vt * vt).sum() - c * c) / nz2, np.nan)
    chi2[allowed & (c <= 0)] = np.nan
    nh1 = n_h + 1
    per = len(models) // len(seeings)           # models per seeing slice: nh1 * n_r
    n_r = per // nh1
    hidx = np.repeat((np.arange(len(models)) // n_r) % nh1, ns)
    cm = np.where(allowed, np.maximum(c, 0.0), -1.0)
    curve = np.full(nh1, np.nan)
    for ih in range(nh1):
        sel = hidx == ih
        if allowed[sel].any():
            curve[ih] = ((vt * vt).sum() - cm[sel].max() ** 2) / nz2
    return chi2, curve


def interval(curve, heights, delta_chi2):
    hs = np.array(list(heights) + [np.inf])
    cmin = np.nanmin(curve)
    sel = curve <= cmin + delta_chi2
    return cmin, hs[sel].min(), hs[sel].max()
