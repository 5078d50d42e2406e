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


def centre(v, rounded=False):
    """v - mean(v) in double; rounded: the float32 v~ of the header's step 6, widened back to double"""
    v = np.asarray(v, np.float64)
    vt = v - v.mean(axis=-1, keepdims=True)
    return vt.astype(np.float32).astype(np.float64) if rounded else vt


def seeing_slice(seeings, seeing):
    """index of the seeing slice of a fixed seeing (nearest value; a tie: the lower value; equal values: the first), None: free"""
    if seeing is None or np.isnan(seeing):
        return None
    d = np.abs(np.asarray(seeings, np.float64) - float(seeing))
    return min(range(len(seeings)), key=lambda j: (d[j], seeings[j], j))


def fit(g, cols64, models, n_h, seeings, trail, v, seeing=None, delta_chi2=None, rounded=False):
    """chi2 of every column in double (least squares a, b; NaN for columns not allowed), and the per-height curve, chi2_min,
    h_lo, h_hi, chi2_focus as the header defines them (from double scores).  rounded: v~ is the float32 of step 6."""
    delta_chi2 = 1.0 / g.step if delta_chi2 is None else delta_chi2
    vt = centre(v, rounded)
    nz2 = trail["noise"] ** 2
    ns = 2 * g.S + 1
    allowed = np.repeat(np.array([m["valid"] for m in models]), ns)
    best = seeing_slice(seeings, seeing)
    per = len(models) // len(seeings)           # models per seeing slice: nh1 * n_r
    if best is not None:
        allowed &= np.repeat(np.arange(len(models)) // per == best, ns)
    c = cols64 @ vt
    chi2 = np.where(allowed, ((vt * vt).sum() - c * c) / nz2, np.nan)
    chi2[allowed & (c <= 0)] = np.nan
    nh1 = n_h + 1
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


# ---- acceptance of a device fit against the double restatement --------------------------------------------------------------
STATUS_OK, STATUS_NO_MODEL = 0, 4   # LFDMI_DEFOCUS_OK / _NO_MODEL


def score_bound(nbp, vt):
    """e = (nbp + 2) 2^-24 |v~|_2: no float32 dot product of v~ with a bank column, in any summation order, fused or not, lies
    further than e from the double product v~ . t of the same (unrounded) column.

    With u = 2^-24 and t the double column of unit norm, t^ = t (1 + d_k), |d_k| <= u, its float32 rounding:
      rounding the column:  |v~ . t^ - v~ . t| = |sum v~_k t_k d_k| <= u |v~| |t| = u |v~|            (Cauchy-Schwarz)
      the float32 sum:      |fl(v~ . t^) - v~ . t^| <= gamma_n sum |v~_k t^_k| <= gamma_n |v~| |t^|    (Higham, Accuracy and
        Stability, eq. 3.5: n = nbp terms, products and sums each rounded once or fused, any order; gamma_n = n u / (1 - n u))
    and |t^| <= 1 + u.  With n <= 1040, gamma_n (1 + u) <= (n + 1) u, so the two add to at most (nbp + 2) u |v~|.  The padded
    bins are 0 on both sides and only make the bound larger than needed."""
    vt = np.asarray(vt, np.float64)
    return (nbp + 2) * 2.0 ** -24 * np.sqrt((vt * vt).sum(axis=-1))


class Restated:
    """A restated bank with what the acceptance rule needs: per-column model / height index, validity and the classes of
    columns whose float32 values are bit-identical."""

    def __init__(self, g, heights, radii, seeings):
        self.g, self.heights, self.radii, self.seeings = g, list(heights), list(radii), list(seeings)
        self.c32, self.c64, self.models = bank(g, heights, radii, seeings)
        self.ns, self.nb = 2 * g.S + 1, 2 * g.K + 1
        self.nbp = (self.nb + 15) // 16 * 16
        self.n_h, self.n_r, self.n_se = len(self.heights), len(self.radii), len(self.seeings)
        self.group = self.n_r * self.ns
        self.ncol = len(self.c32)
        self.valid = np.array([m["valid"] for m in self.models])
        self.vcol = np.repeat(self.valid, self.ns)
        mi = np.arange(len(self.models))
        self.col_slice = np.repeat(mi // ((self.n_h + 1) * self.n_r), self.ns)
        self.col_h = np.repeat((mi // self.n_r) % (self.n_h + 1), self.ns)
        _, self.cls = np.unique(self.c32.view(np.uint32), axis=0, return_inverse=True)
        self.cls = self.cls.reshape(-1)
        self.hs = np.array(self.heights + [np.inf])


def judge(rb, trails, prof, seeing=None):
    """What the acceptance rule needs of every row, from double scores of the float32 v~: dict of arrays over the rows.
    c [n, ncol], allowed [n, ncol], e, cmax, must_ok, must_none, decisive, want (the column a decisive row must return),
    curve [n, n_h + 1], m (the clipped maximum per height) and vn2."""
    with np.errstate(all="ignore"):
        return _judge(rb, trails, np.asarray(prof, np.float32), seeing)


def _judge(rb, trails, prof, seeing):
    n = len(prof)
    vt = centre(prof, rounded=True)
    e = score_bound(rb.nbp, vt)
    c = vt @ rb.c64.T
    vn2 = (vt * vt).sum(axis=1)
    allowed = np.broadcast_to(rb.vcol, (n, rb.ncol)).copy()
    if seeing is not None:
        for i, s in enumerate(np.broadcast_to(np.asarray(seeing, np.float32), (n,))):
            j = seeing_slice(rb.seeings, s)
            if j is not None:
                allowed[i] &= rb.col_slice == j
    ca = np.where(allowed, c, -np.inf)
    cmax = ca.max(axis=1)
    jstar = ca.argmax(axis=1)
    must_ok = cmax > 2 * e
    must_none = ~(ca > -2 * e[:, None]).any(axis=1)
    same = allowed & (rb.cls[None, :] == rb.cls[jstar][:, None])
    rest = np.where(allowed & ~same, c, -np.inf).max(axis=1)
    decisive = must_none | (must_ok & (cmax - rest > 2 * e))
    want = np.where(must_ok, same.argmax(axis=1), -1)
    nz2 = np.asarray(trails["noise"], np.float64) ** 2
    nh1 = rb.n_h + 1
    curve, m = np.full((n, nh1), np.nan), np.full((n, nh1), np.nan)
    for ih in range(nh1):
        sel = rb.col_h == ih
        any_ = allowed[:, sel].any(axis=1)
        mm = np.maximum(np.where(allowed[:, sel], c[:, sel], -np.inf).max(axis=1), 0.0)
        m[:, ih] = np.where(any_, mm, np.nan)
        curve[:, ih] = np.where(any_, (vn2 - mm * mm) / nz2, np.nan)
    return {"c": c, "allowed": allowed, "e": e, "cmax": cmax, "must_ok": must_ok, "must_none": must_none, "decisive": decisive,
            "want": want, "curve": curve, "m": m, "vn2": vn2}


def rel_close(a, b, tol):
    a, b = float(a), float(b)
    return a == b or abs(a - b) <= tol * max(abs(a), abs(b))


def least_squares(rb, col, v, noise):
    """(a, b, chi2) of column col for the float32 row v, in double, as step 6 states them"""
    t = column(rb.g, rb.models[col // rb.ns]["samp"], col % rb.ns - rb.g.S)[1]
    v = np.asarray(v, np.float64)
    tc, vc = t - t.mean(), v - v.mean()
    a = (vc * tc).sum() / (tc * tc).sum()
    b = v.mean() - a * t.mean()
    r = v - a * t - b
    return a, b, (r * r).sum() / noise ** 2


def is_blank(f, status):
    return (f["status"] == status and f["shift"] == 0 and f["dof"] == 0 and f["column"] == -1 and
            all(np.isnan(f[k]) for k in ("h_km", "radius_m", "seeing_arcsec", "amplitude", "offset", "chi2", "h_lo", "h_hi",
                                         "chi2_focus", "model_ofwhm", "model_depth")))


def accept(rb, J, i, trail, v, f, cbh, delta_chi2):
    """The acceptance rule for row i of judge()'s J: the device's record f and chi2_by_height row cbh.  Raises AssertionError;
    returns 'band' when the row lies where either status is accepted, else 'ok'."""
    e, c, allowed = J["e"][i], J["c"][i], J["allowed"][i]
    tag = (i, int(f["status"]), int(f["column"]))
    if J["must_ok"][i]:
        assert f["status"] == STATUS_OK, tag
    elif J["must_none"][i]:
        assert f["status"] == STATUS_NO_MODEL, tag
    else:
        assert f["status"] in (STATUS_OK, STATUS_NO_MODEL), tag
    nz2 = float(trail["noise"]) ** 2
    # chi2 by height from float32 scores: each maximum within e of the double one, then one float32 rounding
    curve, m = J["curve"][i], J["m"][i]
    bound = (2 * m * e + e * e) / nz2 + 2.0 ** -23 * np.abs(curve)
    assert np.array_equal(np.isnan(cbh), np.isnan(curve)), (tag, cbh, curve)
    fin = ~np.isnan(curve)
    assert (np.abs(cbh[fin].astype(np.float64) - curve[fin]) <= bound[fin]).all(), (tag, cbh, curve, bound)
    if f["status"] == STATUS_NO_MODEL:
        assert is_blank(f, STATUS_NO_MODEL), (tag, f)
        return "ok" if J["must_none"][i] else "band"
    col = int(f["column"])
    assert 0 <= col < rb.ncol and allowed[col], tag
    assert c[col] >= J["cmax"][i] - 2 * e, (tag, c[col], J["cmax"][i], e)
    if J["decisive"][i]:
        assert col == J["want"][i], (tag, int(J["want"][i]))
    a, b, chi2 = least_squares(rb, col, v, float(trail["noise"]))
    assert rel_close(f["chi2"], chi2, 1e-9) and rel_close(f["amplitude"], a, 1e-9) and rel_close(f["offset"], b, 1e-9), \
        (tag, f["chi2"], chi2, f["amplitude"], a, f["offset"], b)
    mod = rb.models[col // rb.ns]
    assert (f["h_km"], f["radius_m"], f["seeing_arcsec"], f["shift"]) == (mod["h"], mod["R"], mod["seeing"], col % rb.ns - rb.g.S), tag
    assert f["dof"] == 2 * rb.g.K - 1
    assert rel_close(f["model_ofwhm"], mod["ofwhm"], 1e-9) and rel_close(f["model_depth"], mod["depth"], 1e-9), tag
    assert abs(f["chi2_focus"] - curve[-1]) <= bound[-1] or (np.isnan(f["chi2_focus"]) and np.isnan(curve[-1])), tag
    cm, lo, hi = interval(curve, rb.heights, delta_chi2)
    if (f["h_lo"], f["h_hi"]) != (lo, hi):  # only where a height's value lies on the threshold within the bound
        assert (np.abs(curve[fin] - (cm + delta_chi2)) <= bound[fin]).any(), (tag, f["h_lo"], f["h_hi"], lo, hi, curve)
    return "ok" if J["must_ok"][i] else "band"
