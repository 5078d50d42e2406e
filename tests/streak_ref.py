"""numpy restatement of the short-streak search (include/lfdmi.h: short-streak search).  Every sum is an integer and every float32
is one rounded operation of the definition, so the device has to reproduce these records in every integer and every bit."""
import math

import numpy as np

OK, NONE = 0, 1
DEFAULTS = {"bin": 2, "length": 32, "max_streaks": 4, "peel_halfwidth": 8, "clip": 0.125, "threshold": 8.0}
DEFAULT_SIGMA = 0.025
SCALE = 1048576.0          # 2^20
FIELDS = ("status", "found", "q", "s", "r0", "c0", "n_pix", "sum", "snr", "x1", "y1", "x2", "y2", "rho", "theta")


def prepare(frame, b, clip):
    """steps 1, 2: (G int64 [Hb, Wb], M int64 [Hb, Wb]); row 0 is y = 0 of the flipped frame"""
    x = np.asarray(frame, np.float32)[::-1]
    h, w = x.shape
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(x) & (x != 0) & (np.abs(x) <= np.float32(clip))
    g = np.zeros((h, w), np.int64)
    g[valid] = np.rint(x[valid].astype(np.float64) * SCALE).astype(np.int64)     # rint: to nearest, ties to even, as llrint
    hb, wb = -(-h // b), -(-w // b)
    gp = np.zeros((hb * b, wb * b), np.int64)
    mp = np.zeros((hb * b, wb * b), np.int64)
    gp[:h, :w] = g
    mp[:h, :w] = valid
    G = gp.reshape(hb, b, wb, b).sum(axis=(1, 3))
    M = mp.reshape(hb, b, wb, b).sum(axis=(1, 3))
    return G, M


def in_range(clip, b, L):
    """step 2's range rule"""
    return int(np.rint(np.float64(np.float32(clip)) * SCALE)) * b * b * L < 2 ** 31


def off(i, s, L):
    """step 4: the row offset of cell i of a segment of slope s"""
    a = (2 * abs(s) * i + (L - 1)) // (2 * (L - 1))
    return a if s >= 0 else -a


def orient(A, q):
    return A if q == 0 else A.T


def segment_sums(Q, s, L):
    """(sums [nr, nc], r_lo): the sum of every existing segment of slope s, anchors r0 = r_lo .. r_lo + nr - 1, c0 = 0 .. nc - 1;
    None when there is none"""
    R, C = Q.shape
    r_lo, r_hi = max(0, -s), min(R, R - s)
    nc = C - L + 1
    if nc < 1 or r_hi <= r_lo:
        return None, r_lo
    S = np.zeros((r_hi - r_lo, nc), np.int64)
    for i in range(L):
        o = off(i, s, L)
        S += Q[r_lo + o:r_hi + o, i:i + nc]
    return S, r_lo


def score(S, N, sigma):
    """step 5's float32 score of integer sums"""
    A = (S.astype(np.float64) * (1.0 / SCALE)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = A / (np.float32(sigma) * np.sqrt(N.astype(np.float32)))
    return A, snr.astype(np.float32)


def line_of(q, s, r0, c0, L, b):
    """step 6: (x1, y1, x2, y2, rho, theta)"""
    pts = []
    for c, r in ((c0, r0), (c0 + L - 1, r0 + s)):
        i, j = (c, r) if q == 0 else (r, c)
        pts.append((b * i + (b - 1) / 2.0, b * j + (b - 1) / 2.0))
    (x1, y1), (x2, y2) = pts
    theta = math.atan2(-(x2 - x1), y2 - y1)
    if theta < 0.0:
        theta += math.pi
    if theta >= math.pi:
        theta -= math.pi
    rho = x1 * math.cos(theta) + y1 * math.sin(theta)
    return x1, y1, x2, y2, rho, theta


def none_record():
    r = {k: 0 for k in FIELDS}
    r.update(status=NONE, sum=np.float32(0), snr=np.float32(0), x1=0.0, y1=0.0, x2=0.0, y2=0.0, rho=0.0, theta=0.0)
    return r


def search_arrays(G, M, sigma, L, b, threshold):
    """steps 3 - 6 on binned arrays: one record"""
    best = None
    for q in (0, 1):
        Q, QM = orient(G, q), orient(M, q)
        for s in range(-(L - 1), L):
            S, r_lo = segment_sums(Q, s, L)
            if S is None:
                continue
            N, _ = segment_sums(QM, s, L)
            cand = 2 * N >= L * b * b
            if not cand.any():
                continue
            A, snr = score(S, N, sigma)
            snr = np.where(cand, snr, -np.inf).astype(np.float32)
            k = int(np.argmax(snr))                                   # row-major: the first maximum is the lowest (r0, c0)
            ri, ci = divmod(k, snr.shape[1])
            if best is None or snr[ri, ci] > best["snr"]:                 # q, then s ascending: a tie keeps the earlier one
                best = {"q": q, "s": s, "r0": r_lo + ri, "c0": ci, "n_pix": int(N[ri, ci]), "sum": np.float32(A[ri, ci]),
                        "snr": np.float32(snr[ri, ci])}
    if best is None:
        return none_record()
    best["status"] = OK
    best["found"] = int(best["snr"] >= np.float32(threshold))
    x1, y1, x2, y2, rho, theta = line_of(best["q"], best["s"], best["r0"], best["c0"], L, b)
    best.update(x1=x1, y1=y1, x2=x2, y2=y2, rho=rho, theta=theta)
    return best


def peel_mask(shape, rec, L, hw):
    """step 7: the cells [Hb, Wb] a found record blots, as a boolean array"""
    hb, wb = shape
    q = rec["q"]
    R, C = (hb, wb) if q == 0 else (wb, hb)
    r = np.arange(R)[:, None]
    c = np.arange(C)[None, :]
    i = c - rec["c0"]
    ic = np.clip(i, 0, L - 1)
    offs = np.array([off(k, rec["s"], L) for k in range(L)])
    hit = (i >= -hw) & (i <= L - 1 + hw) & (np.abs(r - (rec["r0"] + offs[ic])) <= hw)
    return hit if q == 0 else hit.T


def check_params(p):
    b, L = int(p["bin"]), int(p["length"])
    if b not in (1, 2, 4) or L not in (8, 16, 32, 64) or not 1 <= int(p["max_streaks"]) <= 8 or int(p["peel_halfwidth"]) < 0:
        raise ValueError("streak parameters out of range")
    if not (math.isfinite(p["clip"]) and p["clip"] > 0 and math.isfinite(p["threshold"]) and p["threshold"] > 0):
        raise ValueError("streak parameters out of range")
    if not in_range(p["clip"], b, L):
        raise ValueError("clip * bin * bin * length does not fit int32")


def rounds(frame, sigma=DEFAULT_SIGMA, **params):
    """step 7: (records, n_streaks) of one frame; ``records`` has max_streaks entries, those after the stopping one all zero"""
    p = dict(DEFAULTS)
    p.update(params)
    check_params(p)
    b, L, K = int(p["bin"]), int(p["length"]), int(p["max_streaks"])
    hw = -(-int(p["peel_halfwidth"]) // b)
    G, M = prepare(frame, b, p["clip"])
    recs, n = [], 0
    for k in range(K):
        rec = search_arrays(G, M, sigma, L, b, p["threshold"])
        recs.append(rec)
        if rec["status"] != OK or not rec["found"]:
            break
        n += 1
        if k + 1 < K:
            hit = peel_mask(G.shape, rec, L, hw)
            G = np.where(hit, 0, G)
            M = np.where(hit, 0, M)
    zero = none_record()
    zero["status"] = 0
    recs += [dict(zero) for _ in range(K - len(recs))]
    return recs, n


def search(frame, sigma=DEFAULT_SIGMA, **params):
    """record 0 of one frame"""
    params = dict(params, max_streaks=1)
    return rounds(frame, sigma, **params)[0][0]
