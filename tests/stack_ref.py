"""CPU restatement of the stacked cross-sections (include/lfdmi.h, "stacked cross-sections"; device: lfd_amd/csrc/stack/).

Written from the definition, in numpy and plain Python, for the tests to check lfdmi_stack_profiles against; the product never
imports it.  Values follow the definition's precision and operation order step by step (double geometry and bin index,
sequential float32 sums per block and per half, double statistics), so the device's records, rows, sums and counts equal these
bit for bit.
"""
import math

import numpy as np

OK, BAD_SEGMENT, TOO_SHORT, TOO_FAINT = 0, 1, 2, 3
DEFAULT_SIGMA = float(np.float32(0.025))
DEFAULTS = dict(wing=8, n_iter=2, min_cols=64, clip=0.125, prof_half=24.0, step=0.5, box=4.0, max_shift=8.0, k_sig=6.0, k_ref=4.0,
                pixscale=0.396)
INT_FIELDS = ("status", "n_col", "min_valid", "n_pass")
F64_FIELDS = ("rho", "theta", "x1", "y1", "x2", "y2", "background", "noise", "peak", "fwhm", "fwhm_arcsec", "depth", "flux",
              "flux_err", "snr", "shift", "tilt")
FIELDS = INT_FIELDS + F64_FIELDS


def n_bins(params=None):
    p = dict(DEFAULTS, **(params or {}))
    return 2 * int(round(p["prof_half"] / p["step"])) + 1


def lowmed(v):
    """lower median: rank floor((m-1)/2) of the ascending values (NaN for none)"""
    v = np.sort(np.asarray(v, np.float64))
    return float(v[(len(v) - 1) // 2]) if len(v) else math.nan


def cosphi_of(g):
    return 1.0 / math.sqrt(1.0 + g * g)


class Line:
    def __init__(self, a1, b1, g):
        self.a1, self.b1, self.g, self.cosphi = a1, b1, g, cosphi_of(g)

    def bc(self, a):
        return self.b1 + self.g * (a - self.a1)


def geometry(seg, shape, min_cols):
    """step 2: (status, xmajor, a_first, a_last, amid, Line) of a segment (x1, y1, x2, y2)"""
    h, w = shape
    x1, y1, x2, y2 = (float(v) for v in seg)
    if not all(math.isfinite(v) and abs(v) <= 1e6 for v in (x1, y1, x2, y2)):
        return BAD_SEGMENT, 0, 0, -1, 0, None
    dx, dy = x2 - x1, y2 - y1
    if dx == 0.0 and dy == 0.0:
        return BAD_SEGMENT, 0, 0, -1, 0, None
    xmajor = abs(dx) >= abs(dy)
    a1, b1, a2, b2 = (x1, y1, x2, y2) if xmajor else (y1, x1, y2, x2)
    A = w if xmajor else h
    line = Line(a1, b1, (b2 - b1) / (a2 - a1))
    a_first = int(max(math.ceil(min(a1, a2)), 0.0))
    a_last = int(min(math.floor(max(a1, a2)), float(A - 1)))
    amid = (a_first + a_last + 1) >> 1
    return (TOO_SHORT if a_last - a_first + 1 < min_cols else OK), int(xmajor), a_first, a_last, amid, line


def valid_pixels(v, clip):
    """step 1 on float32 values"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v != 0) & (np.abs(v) <= np.float32(clip))


def block_sums(img, xmajor, line, a_lo, a_hi, K, step, clip):
    """steps 3 and 4 for one block of columns: (float32 sums [2K+1], counts)"""
    h, w = img.shape
    nb = 2 * K + 1
    B = h if xmajor else w
    reach = (K * step + step / 2.0) / line.cosphi
    c = [line.bc(float(a_lo)), line.bc(float(a_hi))]
    b0 = max(int(math.floor(min(c) - reach)) - 3, 0)        # (no pixel outside this window can reach a bin)
    b1 = min(int(math.ceil(max(c) + reach)) + 3, B - 1)
    if b1 < b0:
        return np.zeros(nb, np.float32), np.zeros(nb, np.int64)
    aa = np.arange(a_lo, a_hi + 1)[:, None]
    bb = np.arange(b0, b1 + 1)[None, :]
    x, y = (aa, bb) if xmajor else (bb, aa)
    v = img[h - 1 - y, x]
    v = np.broadcast_to(v, (aa.shape[0], bb.shape[1]))
    bc = line.b1 + line.g * (aa.astype(np.float64) - line.a1)
    t = (bb.astype(np.float64) - bc) * line.cosphi * (1.0 / step) + (K + 0.5)
    ok = valid_pixels(v, clip) & (t >= 0.0) & (t < float(nb))
    ks = np.floor(t[ok]).astype(np.int64)                   # C order: columns ascending, b ascending within a column
    vs = v[ok].astype(np.float32)
    cnt = np.bincount(ks, minlength=nb)
    order = np.argsort(ks, kind="stable")
    ks, vs = ks[order], vs[order]
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    mat = np.zeros((nb, max(int(cnt.max()), 1)), np.float32)
    mat[ks, np.arange(len(ks)) - start[ks]] = vs            # (trailing +0 leave a sequential sum as it is)
    return np.cumsum(mat, axis=1, dtype=np.float32)[:, -1], cnt


def pass_sums(img, xmajor, line, a_first, a_last, amid, K, step, clip):
    """step 4: (A [2, 2K+1] float32, N [2, 2K+1] int32) of one pass: left and right half"""
    nb = 2 * K + 1
    A = np.zeros((2, nb), np.float32)
    N = np.zeros((2, nb), np.int64)
    for hf, (lo, hi) in enumerate(((a_first, amid - 1), (amid, a_last))):
        a = lo
        while a <= hi:
            end = min(hi, a | 31)
            s, c = block_sums(img, xmajor, line, a, end, K, step, clip)
            A[hf] = A[hf] + s                                # (one float32 addition per bin, blocks ascending)
            N[hf] += c
            a = end + 1
    return A, N.astype(np.int32)


def half_centre(A, N, K, p):
    """step 5 for one half: (shift, score) or None"""
    nb = 2 * K + 1
    ub = (np.arange(nb) - K).astype(np.float64) * p["step"]
    Ad, Nd = A.astype(np.float64), N.astype(np.float64)
    wing = (np.abs(ub) >= p["prof_half"] - float(p["wing"])) & (N > 0)
    if not wing.any():
        return None
    bkg = lowmed(Ad[wing] / Nd[wing])
    hb = int(math.floor(p["box"] / (2.0 * p["step"])))
    best, score = -1, 0.0
    for k in range(nb):
        if not abs(float(ub[k])) <= p["max_shift"]:
            continue
        SA = SN = 0.0
        for j in range(max(k - hb, 0), min(k + hb, 2 * K) + 1):
            SA = SA + float(Ad[j])
            SN = SN + float(Nd[j])
        if not SN > 0.0:
            continue
        sc = (SA - bkg * SN) / math.sqrt(SN)
        if best < 0 or sc > score:
            best, score = k, sc
    if best < 0:
        return None
    return float(best - K) * p["step"], score


def refine(line, a_first, a_last, amid, A, N, K, p, sigma):
    """step 5: the next pass's Line, or None when refinement stops"""
    L, R = half_centre(A[0], N[0], K, p), half_centre(A[1], N[1], K, p)
    if L is None or R is None:
        return None
    thr = p["k_ref"] * sigma
    if not L[1] >= thr or not R[1] >= thr:
        return None
    aL, aR = (float(a_first) + float(amid - 1)) * 0.5, (float(amid) + float(a_last)) * 0.5
    bL, bR = line.bc(aL) + L[0] / line.cosphi, line.bc(aR) + R[0] / line.cosphi
    g = (bR - bL) / (aR - aL)
    if not abs(g) <= 2.0:
        return None
    return Line(aL, bL, g)


def scores(img, seg, sigma=DEFAULT_SIGMA, **params):
    """the two halves' first-pass box scores over sigma (what k_ref is compared with), or None"""
    p = dict(DEFAULTS, **params)
    K = int(round(p["prof_half"] / p["step"]))
    img = np.ascontiguousarray(img, np.float32)
    status, xmajor, a_first, a_last, amid, line = geometry(seg, img.shape, p["min_cols"])
    if status != OK:
        return None
    A, N = pass_sums(img, xmajor, line, a_first, a_last, amid, K, p["step"], p["clip"])
    L, R = half_centre(A[0], N[0], K, p), half_centre(A[1], N[1], K, p)
    return None if L is None or R is None else (L[1] / sigma, R[1] / sigma)


def finalize(rec, xmajor, a_first, a_last, line0, line, A, N, K, p):
    """step 6: fills rec, returns the row"""
    nb = 2 * K + 1
    a = A[0] + A[1]
    n = N[0].astype(np.int64) + N[1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.where(n > 0, a / np.maximum(n, 1).astype(np.float32), np.float32(np.nan)).astype(np.float32)
        ub = (np.arange(nb) - K).astype(np.float64) * p["step"]
        edge = p["prof_half"] - float(p["wing"])
        wb = (np.abs(ub) >= edge) & ~np.isnan(m)
        wings = bool(wb.any())
        bg = np.float32(lowmed(m[wb].astype(np.float64))) if wings else np.float32(np.nan)
        v = (m - bg).astype(np.float32)
        good = ~np.isnan(v)
        peak = np.float32(v[good].max()) if good.any() else np.float32(-np.inf)
        noise = 1.4826 * lowmed(np.abs(v[good & (np.abs(ub) >= edge)].astype(np.float64))) if wings else math.nan
        rec.update(n_col=a_last - a_first + 1, min_valid=int(n.min()), background=float(bg), noise=noise, peak=float(peak),
                   fwhm=math.nan, fwhm_arcsec=math.nan, depth=math.nan)
        if peak > 0:
            idx = np.where(v >= peak / np.float32(2))[0]
            left, right = int(idx[0]), int(idx[-1])
            fw = 0.0 if left == right else abs(float(ub[right])) + abs(float(ub[left]))
            rec.update(fwhm=fw, fwhm_arcsec=fw * p["pixscale"], depth=(float(peak) - float(v[K])) / float(peak) * 100.0)
        total, ncore = 0.0, 0
        for k in range(nb):
            if abs(float(ub[k])) < edge:
                total = total + float(v[k])
                ncore += 1
        flux = p["step"] * total
        flux_err = p["step"] * noise * math.sqrt(float(ncore))
        snr = float(np.float64(flux) / np.float64(flux_err))        # (IEEE division: a zero flux_err gives an infinity or NaN)
    rec.update(flux=flux, flux_err=flux_err, snr=snr,
               status=OK if (peak > 0 and float(peak) >= p["k_sig"] * noise) else TOO_FAINT)
    af, al = float(a_first), float(a_last)
    bf, bl = line.bc(af), line.bc(al)
    x1, y1, x2, y2 = (af, bf, al, bl) if xmajor else (bf, af, bl, al)
    dx, dy = x2 - x1, y2 - y1
    ln = math.sqrt(dx * dx + dy * dy)
    nx, ny = dy / ln, -(dx / ln)
    if ny < 0.0 or (ny == 0.0 and nx < 0.0):
        nx, ny = -nx, -ny
    am = (af + al) * 0.5
    rec.update(x1=x1, y1=y1, x2=x2, y2=y2, theta=math.atan2(ny, nx), rho=x1 * nx + y1 * ny,
               shift=(line.bc(am) - line0.bc(am)) * line0.cosphi, tilt=math.atan(line.g) - math.atan(line0.g))
    return v


def measure(img, seg, sigma=DEFAULT_SIGMA, **params):
    """One frame (h x w float32, buffer orientation) and one segment (x1, y1, x2, y2) of the flipped frame -> (record dict,
    float32 row [2K+1], float32 sums [2, 2K+1], int32 counts [2, 2K+1])."""
    p = dict(DEFAULTS, **params)
    K = int(round(p["prof_half"] / p["step"]))
    nb = 2 * K + 1
    img = np.ascontiguousarray(img, np.float32)
    rec = {k: math.nan for k in F64_FIELDS}
    rec.update(status=OK, n_col=0, min_valid=0, n_pass=0)
    row = np.full(nb, np.nan, np.float32)
    A, N = np.zeros((2, nb), np.float32), np.zeros((2, nb), np.int32)
    status, xmajor, a_first, a_last, amid, line = geometry(seg, img.shape, p["min_cols"])
    if status != OK:
        rec.update(status=status, n_col=max(0, a_last - a_first + 1) if status == TOO_SHORT else 0)
        return rec, row, A, N
    line0 = line
    for it in range(int(p["n_iter"]) + 1):
        A, N = pass_sums(img, xmajor, line, a_first, a_last, amid, K, p["step"], p["clip"])
        rec["n_pass"] = it + 1
        nxt = refine(line, a_first, a_last, amid, A, N, K, p, float(np.float32(sigma))) if it < int(p["n_iter"]) else None
        if nxt is None:
            break
        line = nxt
    row = finalize(rec, xmajor, a_first, a_last, line0, line, A, N, K, p)
    return rec, row, A, N
