"""CPU restatement of the trail-profile measurement (include/lfdmi.h, "trail profiles"; device: lfd_amd/csrc/k_trail.h).

Written from the definition, in numpy and plain Python, for the tests to check lfdmi_measure_trails against; the product never
imports it.  Values follow the definition's precision and operation order step by step (float32 samples, double statistics,
sequential sums), so the device's records and profiles equal these exactly (values, not bits: -0.0 == 0.0, NaN where NaN).

``star_mask`` is a boolean h x w array in BUFFER orientation (True: a pixel remove_stars zeroes for the frame's catalogue);
the GPU tests take it from the library's own remove_stars run on a plane of ones.
"""
import math

import numpy as np

OK, NOT_FOUND, TOO_SHORT, TOO_FAINT = 0, 1, 2, 3
DEFAULTS = dict(half_width=32, seg_len=64, n_iter=3, wing=8, k_sig=5.0, prof_half=24.0, prof_step=0.1, pixscale=0.396)
FIELDS = ("status", "n_pos", "n_seg", "min_valid", "rho", "theta", "x1", "y1", "x2", "y2", "background", "noise", "peak",
          "fwhm", "fwhm_arcsec", "depth")


def n_bins(params=None):
    p = dict(DEFAULTS, **(params or {}))
    return 2 * int(round(p["prof_half"] / p["prof_step"])) + 1


def lowmed(v):
    """lower median: rank floor((m-1)/2) of the ascending values (NaN for none)"""
    v = np.sort(np.asarray(v))
    return v[(len(v) - 1) // 2] if len(v) else np.nan


def sample(img, star, x, y):
    """bilinear float32 samples at double coordinates (x, y) of the flipped frame; NaN where not valid (step 2)"""
    h, w = img.shape
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    xf, yf = np.floor(x), np.floor(y)
    ok = (xf >= 0) & (xf <= w - 2) & (yf >= 0) & (yf <= h - 2)
    x0 = np.where(ok, xf, 0).astype(np.int64)
    y0 = np.where(ok, yf, 0).astype(np.int64)
    r0 = h - 1 - y0
    r1 = r0 - 1
    v00, v10, v01, v11 = img[r0, x0], img[r0, x0 + 1], img[r1, x0], img[r1, x0 + 1]
    ok &= np.isfinite(v00) & np.isfinite(v10) & np.isfinite(v01) & np.isfinite(v11)
    if star is not None:
        ok &= ~(star[r0, x0] | star[r0, x0 + 1] | star[r1, x0] | star[r1, x0 + 1])
    a = (x - xf).astype(np.float32)
    b = (y - yf).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        top = v00 + a * (v10 - v00)
        bot = v01 + a * (v11 - v01)
        val = top + b * (bot - top)
    return np.where(ok, val, np.float32(np.nan)).astype(np.float32)


def positions(h, w, f, d, L):
    """(tmin, npos, nseg) of the line f + t d (step 2)"""
    lo, hi = -math.inf, math.inf
    for fa, da, mx in ((f[0], d[0], float(w - 1)), (f[1], d[1], float(h - 1))):
        if da != 0.0:
            t1, t2 = (0.0 - fa) / da, (mx - fa) / da
            lo, hi = max(lo, min(t1, t2)), min(hi, max(t1, t2))
        elif fa < 0.0 or fa > mx:
            return 0, 0, 0
    if not lo <= hi:
        return 0, 0, 0
    a, b = math.ceil(lo), math.floor(hi)
    if a > b:
        return 0, 0, 0
    npos = b - a + 1
    return a, npos, n_segments(npos, L)


def n_segments(npos, L):
    """segments of npos positions: the full ones, and a last partial one of at least L/2 positions (step 4)"""
    return npos // L + (1 if 2 * (npos % L) >= L else 0)


def wing_values(md, R, wing):
    """the wings |u| > R - wing of one segment's m_s(u), u = -R .. R, in index order (step 4)"""
    return np.concatenate([md[:wing], md[2 * R + 1 - wing:]])


def longest_run(flags):
    """(first segment, length) of the longest run of consecutive significant segments; a tie: the first (step 4)"""
    best0 = bestn = cur0 = curn = 0
    for sg, f in enumerate(flags):
        if f:
            if curn == 0:
                cur0 = sg
            curn += 1
            if curn > bestn:
                bestn, best0 = curn, cur0
        else:
            curn = 0
    return best0, bestn


def medians(img, star, f, d, ts, us):
    """m(u) for every u of `us` over the positions `ts` (step 3); also the valid counts"""
    nx, ny = d[1], -d[0]
    t = np.asarray(ts, np.float64)[None, :]
    u = np.asarray(us, np.float64)[:, None]
    x = f[0] + t * d[0] + u * nx
    y = f[1] + t * d[1] + u * ny
    v = sample(img, star, x, y)
    out = np.full(len(us), np.nan, np.float32)
    cnt = np.zeros(len(us), np.int64)
    for i in range(len(us)):
        ok = v[i][~np.isnan(v[i])]
        cnt[i] = len(ok)
        if len(ok):
            out[i] = lowmed(ok)
    return out, cnt


def _segment(m, R, wing, k_sig):
    """(significant, A, c) of one segment's m_s(u), u = -R .. R (step 4)"""
    if np.isnan(m).any():
        return False, 0.0, 0.0
    md = m.astype(np.float64)
    wings = wing_values(md, R, wing)
    b = float(lowmed(wings))
    sd = 1.4826 * float(lowmed(np.abs(wings - b)))
    A = float(np.max(md - b))
    if not (A > k_sig * sd and A > 0.0):
        return False, A, 0.0
    wu = np.maximum((md - b) - A * 0.5, 0.0)
    u = np.arange(-R, R + 1, dtype=np.float64)
    sw = su = 0.0
    for i in range(2 * R + 1):
        sw = sw + float(wu[i])
        su = su + float(u[i]) * float(wu[i])
    return True, A, su / sw


def measure(img, rho, theta, found=1, star_mask=None, **params):
    """One frame (h x w float32, buffer orientation) and its detection record's rho / theta (float32) -> (record dict,
    profile float32 [2K+1])."""
    p = dict(DEFAULTS, **params)
    R, L, wing = int(p["half_width"]), int(p["seg_len"]), int(p["wing"])
    K = int(round(p["prof_half"] / p["prof_step"]))
    nb = 2 * K + 1
    rec = {k: math.nan for k in FIELDS}
    rec.update(status=NOT_FOUND, n_pos=0, n_seg=0, min_valid=0)
    prof = np.full(nb, np.nan, np.float32)
    if not found:
        return rec, prof
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    th, r = float(np.float32(theta)), float(np.float32(rho))
    c, s = math.cos(th), math.sin(th)
    f = [r * c, r * s]
    d = [-s, c]
    us = np.arange(-R, R + 1)
    for it in range(int(p["n_iter"]) + 1):
        tmin, npos, nseg = positions(h, w, f, d, L)
        if npos < 2 * L:
            rec["status"] = TOO_SHORT
            return rec, prof
        seg = []
        for sg in range(nseg):
            ts = tmin + np.arange(sg * L, min(sg * L + L, npos))
            m, _ = medians(img, star_mask, f, d, ts, us)
            seg.append(_segment(m, R, wing, p["k_sig"]))
        best0, bestn = longest_run([sg[0] for sg in seg])
        if bestn < 2:
            rec["status"] = TOO_FAINT
            return rec, prof
        s0, s1 = best0, best0 + bestn - 1
        if it == int(p["n_iter"]):
            break
        S = St = Stt = Sc = Stc = 0.0
        for sg in range(s0, s1 + 1):
            ns = min(L, npos - sg * L)
            tm = float(tmin + sg * L) + float(ns - 1) * 0.5
            wg, cc = seg[sg][1], seg[sg][2]
            S = S + wg
            St = St + wg * tm
            Stt = Stt + wg * tm * tm
            Sc = Sc + wg * cc
            Stc = Stc + wg * tm * cc
        bb = (S * Stc - St * Sc) / (S * Stt - St * St)
        aa = (Sc - bb * St) / S
        nx, ny = d[1], -d[0]
        f = [f[0] + aa * nx, f[1] + aa * ny]
        ex, ey = d[0] + bb * nx, d[1] + bb * ny
        ln = math.sqrt(ex * ex + ey * ey)
        d = [ex / ln, ey / ln]
    j0, j1 = s0 * L, min(s1 * L + L, npos)
    ts = tmin + np.arange(j0, j1)
    ub = (np.arange(nb) - K).astype(np.float64) * p["prof_step"]
    m, cnt = medians(img, star_mask, f, d, ts, ub)
    wing_bins = (np.abs(ub) >= p["prof_half"] - wing) & ~np.isnan(m)
    bg = np.float32(lowmed(m[wing_bins].astype(np.float64))) if wing_bins.any() else np.float32(np.nan)
    v = (m - bg).astype(np.float32)
    noise = 1.4826 * float(lowmed(np.abs(v[wing_bins].astype(np.float64)))) if wing_bins.any() else math.nan
    peak = np.float32(np.nanmax(v)) if (~np.isnan(v)).any() else np.float32(-np.inf)
    if not peak > 0:
        rec["status"] = TOO_FAINT
        return rec, prof
    fw = calc_fwhm(v, ub, peak)
    nx, ny = d[1], -d[0]
    if ny < 0.0 or (ny == 0.0 and nx < 0.0):
        nx, ny = -nx, -ny
    ta, tb = float(ts[0]), float(ts[-1])
    rec.update(status=OK, n_pos=int(j1 - j0), n_seg=int(s1 - s0 + 1), min_valid=int(cnt.min()),
               rho=f[0] * nx + f[1] * ny, theta=math.atan2(ny, nx),
               x1=f[0] + ta * d[0], y1=f[1] + ta * d[1], x2=f[0] + tb * d[0], y2=f[1] + tb * d[1],
               background=float(bg), noise=noise, peak=float(peak), fwhm=fw, fwhm_arcsec=fw * p["pixscale"],
               depth=depth(v, peak))
    return rec, v


def calc_fwhm(v, scale, peak=None):
    """ConvolutionObject.calc_fwhm (lfd/analysis/profiles/convolutionobj.py:160-178) on a profile and its offsets"""
    v = np.asarray(v)
    peak = np.float32(np.nanmax(v)) if peak is None else peak
    idx = np.where(v >= peak / v.dtype.type(2))[0]
    left, right = idx[0], idx[-1]
    if left == right:
        return 0.0
    return abs(float(scale[right])) + abs(float(scale[left]))


def depth(v, peak=None):
    """the sampler's depth (lfd/analysis/profiles/samplers.py:158-162): (peak - obj[len/2]) / peak * 100"""
    v = np.asarray(v)
    peak = np.float32(np.nanmax(v)) if peak is None else peak
    mid = v[int(len(v) / 2)]
    return (float(peak) - float(mid)) / float(peak) * 100.0
