"""numpy restatement of the several-lines search (include/lfdmi.h: faint-trail search, steps 7 - 9) on top of radon_ref: the
dyadic path, the peel rounds and the extent of every found line.  Every float32 result is one rounded operation of the
definition, so the device has to reproduce these records bit for bit."""
import numpy as np

import radon_ref as R

LINES_DEFAULTS = {"max_lines": 4, "peel_halfwidth": 8, "min_seg": 64}
ZERO = {"status": 0, "found": 0, "q": 0, "y0": 0, "s": 0, "n_pix": 0, "sum": np.float32(0), "snr": np.float32(0),
        "x1": 0.0, "y1": 0.0, "x2": 0.0, "y2": 0.0, "rho": 0.0, "theta": 0.0,
        "c1": 0, "c2": 0, "seg_n_pix": 0, "seg_sum": np.float32(0), "seg_snr": np.float32(0),
        "ex1": 0.0, "ey1": 0.0, "ex2": 0.0, "ey2": 0.0}


def dyadic_path(s, P):
    """step 7 by its recursion: d(c; s, P) for c = 0 .. P-1 (int64)"""
    if P == 1:
        return np.zeros(1, np.int64)
    half = dyadic_path(s >> 1, P // 2)
    return np.concatenate([half, ((s + 1) >> 1) + half])


def point_of(q, c, r, shape, b):
    """step 6's mapping of the working point (c, r) of orientation q to pixels"""
    h, w = shape
    hb, wb = -(-h // b), -(-w // b)
    i, j = ((c, r), (c, hb - 1 - r), (r, c), (wb - 1 - r, c))[q]
    return b * i + (b - 1) / 2.0, b * j + (b - 1) / 2.0


def search_vm(V, M, sigma, shape, p):
    """steps 3 - 6 on a prepared (V, M): radon_ref.search from its second line on"""
    b = int(p["bin"])
    sg = np.float32(sigma)
    best = None
    for q in range(4):
        S = R.transform(R.orient(V, q))
        N = R.transform(R.orient(M, q))
        P = S.shape[1]
        cand = N >= int(p["min_len"])
        if not cand.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = S / (sg * np.sqrt(N.astype(np.float32)))
        snr = np.where(cand, snr, -np.inf).astype(np.float32)
        k = int(np.argmax(snr.T))
        s, yi = divmod(k, S.shape[0])
        if best is None or snr[yi, s] > best["snr"]:
            best = {"q": q, "y0": yi - (P - 1), "s": s, "n_pix": int(N[yi, s]), "sum": np.float32(S[yi, s]), "snr": np.float32(snr[yi, s])}
    rec = dict(ZERO)
    if best is None:
        rec["status"] = R.NO_LINE
        return rec
    rec.update(best)
    rec["found"] = int(best["snr"] >= np.float32(p["threshold"]))
    x1, y1, x2, y2, rho, theta = R.line_of(best["q"], best["y0"], best["s"], shape, b)
    rec.update(x1=x1, y1=y1, x2=x2, y2=y2, rho=rho, theta=theta)
    return rec


def line_rows(V, q, y0, s):
    """(rows y0 + d(c) of the line in columns c = 0 .. C-1, R, C) of orientation q"""
    Rr, C = R.orient(V, q).shape
    return y0 + dyadic_path(s, R.pow2_at_least(C))[:C], Rr, C


def extent(V, M, rec, sigma, min_seg, shape, b):
    """step 9: the segment fields of a found record, on the arrays it was found in"""
    q, y0, s = rec["q"], rec["y0"], rec["s"]
    rows, Rr, C = line_rows(V, q, y0, s)
    ok = (rows >= 0) & (rows < Rr)
    cols = np.arange(C)
    a = np.zeros(C, np.float32)
    m = np.zeros(C, np.int64)
    a[ok] = R.orient(V, q)[rows[ok], cols[ok]]
    m[ok] = R.orient(M, q)[rows[ok], cols[ok]]
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
    ex1, ey1 = point_of(q, c1, int(rows[c1]), shape, b)
    ex2, ey2 = point_of(q, c2, int(rows[c2]), shape, b)
    return {"c1": c1, "c2": c2, "seg_n_pix": int(N[c1, c2]), "seg_sum": np.float32(A[c1, c2]), "seg_snr": np.float32(score[c1, c2]),
            "ex1": ex1, "ey1": ey1, "ex2": ex2, "ey2": ey2}


def peel(V, M, rec, hw):
    """step 8: copies of (V, M) without the band of half-width hw cells around the record's line"""
    q = rec["q"]
    V, M = V.copy(), M.copy()
    Qv, Qm = R.orient(V, q), R.orient(M, q)             # views: writing them writes V, M
    rows, Rr, C = line_rows(V, q, rec["y0"], rec["s"])
    r = np.arange(Rr)[:, None]
    band = np.abs(r - rows[None, :]) <= hw
    Qv[band] = np.float32(0)
    Qm[band] = 0
    return V, M


def search_lines(frame, sigma=R.DEFAULT_SIGMA, max_lines=4, peel_halfwidth=8, min_seg=64, **params):
    """(max_lines records as dicts, n_lines) of one frame"""
    p = dict(R.DEFAULTS)
    p.update(params)
    b = int(p["bin"])
    shape = np.asarray(frame).shape
    V, M = R.prepare(frame, b, p["clip"])
    hw = -(-int(peel_halfwidth) // b)
    recs, n_lines = [], 0
    for k in range(max_lines):
        rec = search_vm(V, M, sigma, shape, p)
        recs.append(rec)
        if rec["status"] != R.OK or not rec["found"]:
            break
        n_lines += 1
        rec.update(extent(V, M, rec, sigma, min_seg, shape, b))
        if k + 1 < max_lines:
            V, M = peel(V, M, rec, hw)
    recs += [dict(ZERO) for _ in range(max_lines - len(recs))]
    return recs, n_lines
