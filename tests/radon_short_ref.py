"""numpy restatement of the short-trail search (include/lfdmi.h: faint-trail search, steps 10 - 12) on top of radon_ref and
radon_lines_ref: every stored level of the transform scored strip by strip, the candidate's parent line, and the rounds with
the extent and the peel of the several-lines search on that parent.  Every float32 result is one rounded operation of the
definition, so the device has to reproduce these records bit for bit."""
import numpy as np
from numpy.lib.stride_tricks import as_strided

import radon_lines_ref as L
import radon_ref as R

SHORT_DEFAULTS = {"min_strip": 64, "max_lines": 4, "peel_halfwidth": 8, "min_seg": 32, "short_threshold": 8.5}
ZERO = dict(L.ZERO, level=0, strip=0, ys=0, ss=0)


def levels(Q):
    """step 4 level by level: yields (n, F_n) for n = 2, 4, .. P with F_n[j][y + P - 1][s], y in [-(P-1), R-1]; the dtype of Q is
    kept.  The last one is radon_ref.transform's result with a leading axis of one strip."""
    Q = np.asarray(Q)
    Rr, C = Q.shape
    P = R.pow2_at_least(C)
    rows = Rr + P - 1
    F = np.zeros((P, rows, 1), Q.dtype)
    F[:C, P - 1:P - 1 + Rr, 0] = Q.T
    n = 1
    while n < P:
        A = F[0::2]
        B = np.concatenate([F[1::2], np.zeros((P // (2 * n), n + 1, n), Q.dtype)], axis=1)
        sj, sy, st = B.strides
        D = as_strided(B, (B.shape[0], rows + 1, n), (sj, sy, sy + st), writeable=False)
        out = np.empty((P // (2 * n), rows, 2 * n), Q.dtype)
        out[:, :, 0::2] = A + D[:, :rows]
        out[:, :, 1::2] = A + D[:, 1:]
        F = out
        n *= 2
        yield n, F


def parent_of(level, j, y, s, P):
    """step 11: (y0, Sp) of the full dyadic line whose path over strip j of width ``level`` is candidate (y, s)'s"""
    sp = s * (P // level)
    return y - int(L.dyadic_path(sp, P)[j * level]), sp


def best_short(V, M, sigma, b, min_strip):
    """step 10: the frame's short candidate as a dict (level, q, strip, ys, ss, n_pix, sum, snr), or None"""
    sg = np.float32(sigma)
    best = []
    for q in range(4):
        Qv, Qm = R.orient(V, q), R.orient(M, q)
        P = R.pow2_at_least(Qv.shape[1])
        for (n, S), (_, N) in zip(levels(Qv), levels(Qm)):
            if n < min_strip or n > P // 2:
                continue
            cand = 2 * N >= n * b * b
            if not cand.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                snr = S / (sg * np.sqrt(N.astype(np.float32)))        # float32 throughout: sqrt, multiply, divide
            snr = np.where(cand, snr, -np.inf).astype(np.float32)
            k = int(np.argmax(snr.transpose(0, 2, 1)))                # [j][s][y] order: the first maximum is the lowest (j, s, y)
            j, rest = divmod(k, n * snr.shape[1])
            s, yi = divmod(rest, snr.shape[1])
            best.append({"level": n, "q": q, "strip": j, "ys": yi - (P - 1), "ss": s, "n_pix": int(N[j, yi, s]),
                         "sum": np.float32(S[j, yi, s]), "snr": np.float32(snr[j, yi, s])})
    out = None
    for c in sorted(best, key=lambda c: (c["level"], c["q"])):        # ties to the lowest (L, q, ...)
        if out is None or c["snr"] > out["snr"]:
            out = c
    return out


def search_short_vm(V, M, sigma, shape, b, min_strip, short_threshold):
    """steps 10, 11 and 6 on a prepared (V, M): the round's record without its segment"""
    rec = dict(ZERO)
    c = best_short(V, M, sigma, b, min_strip)
    if c is None:
        rec["status"] = R.NO_LINE
        return rec
    hb, wb = V.shape
    P = R.pow2_at_least(wb if c["q"] < 2 else hb)
    y0, sp = parent_of(c["level"], c["strip"], c["ys"], c["ss"], P)
    rec.update(c, y0=y0, s=sp)
    rec["found"] = int(c["snr"] >= np.float32(short_threshold))
    x1, y1, x2, y2, rho, theta = R.line_of(c["q"], y0, sp, shape, b)
    rec.update(x1=x1, y1=y1, x2=x2, y2=y2, rho=rho, theta=theta)
    return rec


def search_short(frame, sigma=R.DEFAULT_SIGMA, min_strip=64, max_lines=4, peel_halfwidth=8, min_seg=32, short_threshold=8.5,
                 **params):
    """(max_lines records as dicts, n_lines, the plain search's record) of one frame"""
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
        rec = search_short_vm(V, M, sigma, shape, b, int(min_strip), short_threshold)
        recs.append(rec)
        if rec["status"] != R.OK or not rec["found"]:
            break
        n_lines += 1
        rec.update(L.extent(V, M, rec, sigma, min_seg, shape, b))
        if k + 1 < max_lines:
            V, M = L.peel(V, M, rec, hw)
    recs += [dict(ZERO) for _ in range(max_lines - len(recs))]
    return recs, n_lines, plain
