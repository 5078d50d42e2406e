"""numpy restatement of the wide-trail search (include/lfdmi.h: faint-trail search, steps 13 - 16) on top of radon_ref and
radon_lines_ref: the last level of the transform summed over sliding bands of 1, 2, 4, .. max_width neighbouring lines, the
band's centre line and width, and the rounds with the extent and the peel of the several-lines search widened to the band.
Every float32 result is one rounded operation of the definition, so the device has to reproduce these records bit for bit."""
import math

import numpy as np

import radon_lines_ref as L
import radon_ref as R

WIDE_DEFAULTS = {"max_width": 8, "max_lines": 4, "peel_halfwidth": 8, "min_seg": 64, "wide_threshold": 8.0}
ZERO = dict(L.ZERO, width=0, width_px=0.0)


def bands(S, N, max_width):
    """step 13: yields (k, B_k, C_k) for k = 1, 2, 4, .. max_width from one orientation's planes [y + P - 1][s]"""
    B, Cn = np.asarray(S, np.float32), np.asarray(N, np.int64)
    rows = B.shape[0]
    k = 1
    while True:
        yield k, B, Cn
        if 2 * k > max_width:
            return
        up = np.concatenate([B, np.zeros((k, B.shape[1]), np.float32)])[k:k + rows]      # row y + k; above R-1: +0
        upn = np.concatenate([Cn, np.zeros((k, B.shape[1]), np.int64)])[k:k + rows]
        B = (B + up).astype(np.float32)                                                   # one float32 addition
        Cn = Cn + upn
        k *= 2


def centre_point(q, c, r, shape, b):
    """step 6's mapping of the working point (c, r), r between two rows, to pixels (doubles)"""
    h, w = shape
    hb, wb = -(-h // b), -(-w // b)
    i, j = ((float(c), r), (float(c), float(hb - 1) - r), (r, float(c)), (float(wb - 1) - r, float(c)))[q]
    return b * i + (b - 1) / 2.0, b * j + (b - 1) / 2.0


def band_line(q, y0, s, k, shape, b):
    """step 15: (x1, y1, x2, y2, rho, theta, width_px) of band (k, q, s, y0)"""
    h, w = shape
    hb, wb = -(-h // b), -(-w // b)
    P = R.pow2_at_least(wb if q < 2 else hb)
    mid = (k - 1) / 2.0
    x1, y1 = centre_point(q, 0, float(y0) + mid, shape, b)
    x2, y2 = centre_point(q, P - 1, float(y0 + s) + mid, shape, b)
    theta = math.atan2(-(x2 - x1), y2 - y1)
    if theta < 0.0:
        theta += math.pi
    if theta >= math.pi:
        theta -= math.pi
    rho = x1 * math.cos(theta) + y1 * math.sin(theta)
    width_px = float(k * b) * (float(P - 1) / math.sqrt(float((P - 1) * (P - 1) + s * s)))
    return x1, y1, x2, y2, rho, theta, width_px


def best_band(V, M, sigma, min_len, max_width, widths=None):
    """steps 13, 14: the best band of a prepared (V, M) as a dict (width, q, y0, s, n_pix, sum, snr), or None; ``widths``
    (a dict) receives the largest score of every width that has a candidate"""
    sg = np.float32(sigma)
    best = []
    for q in range(4):
        S = R.transform(R.orient(V, q))
        N = R.transform(R.orient(M, q))
        P = S.shape[1]
        for k, B, Cn in bands(S, N, max_width):
            cand = Cn >= k * int(min_len)
            if not cand.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                snr = B / (sg * np.sqrt(Cn.astype(np.float32)))        # float32 throughout: sqrt, multiply, divide
            snr = np.where(cand, snr, -np.inf).astype(np.float32)
            i = int(np.argmax(snr.T))                                  # [s][y] order: the first maximum is the lowest (s, y)
            s, yi = divmod(i, S.shape[0])
            best.append({"width": k, "q": q, "y0": yi - (P - 1), "s": s, "n_pix": int(Cn[yi, s]), "sum": np.float32(B[yi, s]),
                         "snr": np.float32(snr[yi, s])})
            if widths is not None:
                widths[k] = max(widths.get(k, -np.inf), float(snr[yi, s]))
    out = None
    for c in sorted(best, key=lambda c: (c["width"], c["q"])):       # ties to the lowest (k, q, ...)
        if out is None or c["snr"] > out["snr"]:
            out = c
    return out


def search_wide_vm(V, M, sigma, shape, b, min_len, max_width, wide_threshold, widths=None):
    """steps 13 - 15 on a prepared (V, M): the round's record without its segment"""
    rec = dict(ZERO)
    c = best_band(V, M, sigma, min_len, max_width, widths)
    if c is None:
        rec["status"] = R.NO_LINE
        return rec
    rec.update(c)
    rec["found"] = int(c["snr"] >= np.float32(wide_threshold))
    x1, y1, x2, y2, rho, theta, width_px = band_line(c["q"], c["y0"], c["s"], c["width"], shape, b)
    rec.update(x1=x1, y1=y1, x2=x2, y2=y2, rho=rho, theta=theta, width_px=width_px)
    return rec


def extent(V, M, rec, sigma, min_seg, shape, b):
    """step 16's extent: radon_lines_ref.extent with a_c, m_c summed over the band's k rows, rows ascending"""
    q, y0, s, k = rec["q"], rec["y0"], rec["s"], rec["width"]
    rows, Rr, C = L.line_rows(V, q, y0, s)
    Qv, Qm = R.orient(V, q), R.orient(M, q)
    cols = np.arange(C)
    a = np.zeros(C, np.float32)
    m = np.zeros(C, np.int64)
    for u in range(k):
        ru = rows + u
        ok = (ru >= 0) & (ru < Rr)
        au = np.zeros(C, np.float32)
        mu = np.zeros(C, np.int64)
        au[ok] = Qv[ru[ok], cols[ok]]
        mu[ok] = Qm[ru[ok], cols[ok]]
        a = au if u == 0 else (a + au).astype(np.float32)             # one float32 addition per further row
        m = m + mu
    pre = np.zeros(C + 1, np.float32)
    acc = np.float32(0)
    for c in range(C):                                  # one sequential float32 accumulator
        acc = np.float32(acc + a[c])
        pre[c + 1] = acc
    cnt = np.concatenate([[0], np.cumsum(m)])
    A = (pre[None, 1:] - pre[:C, None]).astype(np.float32)          # [c1][c2]
    N = cnt[None, 1:] - cnt[:C, None]
    cand = (N >= int(min_seg)) & (cols[None, :] >= cols[:, None])
    assert cand.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        score = A / (np.float32(sigma) * np.sqrt(N.astype(np.float32)))
    score = np.where(cand, score, -np.inf).astype(np.float32)
    c1, c2 = divmod(int(np.argmax(score)), C)           # row-major: the first maximum is the lowest (c1, c2)
    mid = (k - 1) / 2.0
    ex1, ey1 = centre_point(q, c1, float(int(rows[c1])) + mid, shape, b)
    ex2, ey2 = centre_point(q, c2, float(int(rows[c2])) + mid, shape, b)
    return {"c1": c1, "c2": c2, "seg_n_pix": int(N[c1, c2]), "seg_sum": np.float32(A[c1, c2]), "seg_snr": np.float32(score[c1, c2]),
            "ex1": ex1, "ey1": ey1, "ex2": ex2, "ey2": ey2}


def peel(V, M, rec, hw):
    """step 16's peel: copies of (V, M) without the band's rows y0 + d(c) .. y0 + d(c) + k-1 and hw cells beyond either edge"""
    q, k = rec["q"], rec["width"]
    V, M = V.copy(), M.copy()
    Qv, Qm = R.orient(V, q), R.orient(M, q)             # views: writing them writes V, M
    rows, Rr, C = L.line_rows(V, q, rec["y0"], rec["s"])
    r = np.arange(Rr)[:, None]
    band = (r >= rows[None, :] - hw) & (r <= rows[None, :] + (k - 1) + hw)
    Qv[band] = np.float32(0)
    Qm[band] = 0
    return V, M


def search_wide(frame, sigma=R.DEFAULT_SIGMA, max_width=8, max_lines=4, peel_halfwidth=8, min_seg=64, wide_threshold=8.0,
                widths=None, **params):
    """(max_lines records as dicts, n_lines, the plain search's record) of one frame; ``widths`` (a dict) receives round 0's
    largest score per width"""
    p = dict(R.DEFAULTS)
    p.update(params)
    b = int(p["bin"])
    shape = np.asarray(frame).shape
    V, M = R.prepare(frame, b, p["clip"])
    plain = L.search_vm(V, M, sigma, shape, p)
    plain = {k: plain[k] for k in ("status", "found", "q", "y0", "s", "n_pix", "sum", "snr", "x1", "y1", "x2", "y2", "rho", "theta")}
    hw = -(-int(peel_halfwidth) // b)
    recs, n_lines = [], 0
    for k in range(max_lines):
        rec = search_wide_vm(V, M, sigma, shape, b, p["min_len"], int(max_width), wide_threshold, widths if k == 0 else None)
        recs.append(rec)
        if rec["status"] != R.OK or not rec["found"]:
            break
        n_lines += 1
        rec.update(extent(V, M, rec, sigma, min_seg, shape, b))
        if k + 1 < max_lines:
            V, M = peel(V, M, rec, hw)
    recs += [dict(ZERO) for _ in range(max_lines - len(recs))]
    return recs, n_lines, plain
