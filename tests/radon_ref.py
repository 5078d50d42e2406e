"""numpy restatement of the faint-trail search (include/lfdmi.h: faint-trail search), level by level.  Every float32 result is
one rounded operation of the definition, so the device has to reproduce these records bit for bit."""
import math

import numpy as np
from numpy.lib.stride_tricks import as_strided

OK, NO_LINE = 0, 1
DEFAULTS = {"bin": 2, "clip": 0.125, "min_len": 256, "threshold": 8.0}
DEFAULT_SIGMA = 0.025


def pow2_at_least(c):
    p = 1
    while p < c:
        p *= 2
    return p


def prepare(frame, b, clip):
    """steps 1, 2: (V float32 [Hb, Wb], M int64 [Hb, Wb]) of one frame in buffer rows (row 0 of V is y = 0 of the flipped frame)"""
    x = np.asarray(frame, np.float32)[::-1]
    h, w = x.shape
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(x) & (x != 0) & (np.abs(x) <= np.float32(clip))
    v = np.where(valid, x, np.float32(0)).astype(np.float32)
    hb, wb = -(-h // b), -(-w // b)
    vp = np.zeros((hb * b, wb * b), np.float32)
    mp = np.zeros((hb * b, wb * b), np.int64)
    vp[:h, :w] = v
    mp[:h, :w] = valid
    V = np.zeros((hb, wb), np.float32)
    M = np.zeros((hb, wb), np.int64)
    for dy in range(b):
        for dx in range(b):
            V = V + vp[dy::b, dx::b]          # float32 + float32: one rounded addition each, rows then columns ascending
            M = M + mp[dy::b, dx::b]
    return V, M


def orient(V, q):
    """step 3: the working array Q of orientation q"""
    if q == 0:
        return V
    if q == 1:
        return V[::-1]
    if q == 2:
        return V.T
    return V[:, ::-1].T


def transform(Q):
    """step 4: S[y + P - 1][s] for y in [-(P-1), R-1], s in [0, P); the dtype of Q is kept (float32 sums, integer counts)"""
    Q = np.asarray(Q)
    R, C = Q.shape
    P = pow2_at_least(C)
    rows = R + P - 1
    F = np.zeros((P, rows, 1), Q.dtype)
    F[:C, P - 1:P - 1 + R, 0] = Q.T
    n = 1
    while n < P:
        A = F[0::2]
        B = np.concatenate([F[1::2], np.zeros((P // (2 * n), n + 1, n), Q.dtype)], axis=1)    # rows above R-1 read +0
        # D[j][y][t] = B[j][y + t][t], y = 0 .. rows: the diagonal as a view (a step of one row and one slope), not a gather
        sj, sy, st = B.strides
        D = as_strided(B, (B.shape[0], rows + 1, n), (sj, sy, sy + st), writeable=False)
        out = np.empty((P // (2 * n), rows, 2 * n), Q.dtype)
        out[:, :, 0::2] = A + D[:, :rows]                # s = 2t:     F_n[2j][y][t] + F_n[2j+1][y + t][t]
        out[:, :, 1::2] = A + D[:, 1:]                   # s = 2t + 1: F_n[2j][y][t] + F_n[2j+1][y + t + 1][t]
        F = out
        n *= 2
    return F[0, :rows, :]


def line_of(q, y0, s, shape, b):
    """step 6: (x1, y1, x2, y2, rho, theta) of working line (q, y0, s) for frames of ``shape`` at bin b"""
    h, w = shape
    hb, wb = -(-h // b), -(-w // b)
    C = wb if q < 2 else hb
    P = pow2_at_least(C)
    pts = []
    for c, r in ((0, y0), (P - 1, y0 + s)):
        if q == 0:
            i, j = c, r
        elif q == 1:
            i, j = c, hb - 1 - r
        elif q == 2:
            i, j = r, c
        else:
            i, j = wb - 1 - r, c
        pts.append((b * i + (b - 1) / 2.0, b * j + (b - 1) / 2.0))
    (x1, y1), (x2, y2) = pts
    theta = math.atan2(-(x2 - x1), y2 - y1)
    if theta < 0.0:
        theta += math.pi
    if theta >= math.pi:
        theta -= math.pi
    rho = x1 * math.cos(theta) + y1 * math.sin(theta)
    return x1, y1, x2, y2, rho, theta


def planes(frame, q, b=2, clip=0.125):
    """(S float32, N int64) of orientation q, each [R + P - 1, P]"""
    V, M = prepare(frame, b, clip)
    return transform(orient(V, q)), transform(orient(M, q))


def search(frame, sigma=DEFAULT_SIGMA, **params):
    """the record of one frame as a dict"""
    p = dict(DEFAULTS)
    p.update(params)
    b = int(p["bin"])
    V, M = prepare(frame, b, p["clip"])
    sg = np.float32(sigma)
    best = None
    for q in range(4):
        S = transform(orient(V, q))
        N = transform(orient(M, q))
        P = S.shape[1]
        cand = N >= int(p["min_len"])
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = S / (sg * np.sqrt(N.astype(np.float32)))          # float32 throughout: sqrt, multiply, divide
        snr = np.where(cand, snr, -np.inf).astype(np.float32)
        if not cand.any():
            continue
        k = int(np.argmax(snr.T))                                     # [s][y] order: the first maximum is the lowest (s, y)
        s, yi = divmod(k, S.shape[0])
        if best is None or snr[yi, s] > best["snr"]:
            best = {"q": q, "y0": yi - (P - 1), "s": s, "n_pix": int(N[yi, s]), "sum": np.float32(S[yi, s]), "snr": np.float32(snr[yi, s])}
    if best is None:
        return {"status": NO_LINE, "found": 0, "q": 0, "y0": 0, "s": 0, "n_pix": 0, "sum": np.float32(0), "snr": np.float32(0),
                "x1": 0.0, "y1": 0.0, "x2": 0.0, "y2": 0.0, "rho": 0.0, "theta": 0.0}
    best["status"] = OK
    best["found"] = int(best["snr"] >= np.float32(p["threshold"]))
    x1, y1, x2, y2, rho, theta = line_of(best["q"], best["y0"], best["s"], np.asarray(frame).shape, b)
    best.update(x1=x1, y1=y1, x2=x2, y2=y2, rho=rho, theta=theta)
    return best
