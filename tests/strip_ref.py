"""numpy restatement of the trail strips of include/lfdmi.h ("trail strips"): float64 throughout, the header's expressions left to
right (numpy rounds every operation and never contracts), integer sums in int64.  The device reproduces it in every integer and
every bit of every double.  Steps 1 and the end points' geometry are the light curves' (tests/lc_ref.py), used unchanged."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402

SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"), ("half", "<f8")])
STRIP_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_off", "<i4"), ("K", "<i4"), ("n_ok", "<i4"), ("n_mom", "<i4"),
                        ("dev_section", "<i4"), ("pad", "<i4"), ("mean_centre", "<f8"), ("mean_width", "<f8"), ("max_dev", "<f8")])
SECTION_DTYPE = np.dtype([("status", "<i4"), ("n_geom", "<i4"), ("n_core", "<i4"), ("n_wing", "<i4"), ("t0", "<f8"), ("t1", "<f8"),
                          ("bkg", "<f8"), ("rate", "<f8"), ("rate_err", "<f8"), ("centre", "<f8"), ("width", "<f8")])
CELL_DTYPE = np.dtype([("n_geom", "<i4"), ("n", "<i4"), ("q", "<i8")])
OK, BAD_SEGMENT, TOO_LONG, EMPTY = 0, 1, 2, 3
SEC_OK, SEC_LOW, SEC_EMPTY = 0, 1, 2
MAX_SECTIONS = 1024
MAX_OFF = 129
DEFAULTS = {"sec_len": 8.0, "step": 1.0, "wing": 6.0, "k_mom": 5.0, "clip": 0.125, "min_core": 8, "min_wing": 8}
STRIP_DOUBLES = ("mean_centre", "mean_width", "max_dev")
SEC_DOUBLES = ("bkg", "rate", "rate_err", "centre", "width")
NAN = np.float64(np.nan)
FIX = np.float64(2.0 ** -30)


def segment(frame=0, x1=0.0, y1=0.0, x2=1.0, y2=0.0, half=14.0):
    s = np.zeros(1, SEGMENT_DTYPE)[0]
    s["frame"], s["x1"], s["y1"], s["x2"], s["y2"], s["half"] = frame, x1, y1, x2, y2, half
    return s


def geometry(s, p, max_sections, max_cells):
    """step 2 -> (status, (x1, y1, ex, ey, nx, ny, half, L, inv_s, inv_u, kc, n_sec, n_off, K) or None)"""
    x1, y1, x2, y2, half = (np.float64(s[k]) for k in ("x1", "y1", "x2", "y2", "half"))
    for v in (x1, y1, x2, y2):
        if not np.isfinite(v) or abs(v) > 1e6:
            return BAD_SEGMENT, None
    if not np.isfinite(half) or not half > 0:
        return BAD_SEGMENT, None
    dx = x2 - x1
    dy = y2 - y1
    L = np.sqrt(dx * dx + dy * dy)
    if L == 0:
        return BAD_SEGMENT, None
    inv_s = np.float64(1.0) / np.float64(p["sec_len"])
    inv_u = np.float64(1.0) / np.float64(p["step"])
    kk = np.ceil(half * inv_u - np.float64(0.5))
    if 2.0 * kk + 1.0 > MAX_OFF:
        return BAD_SEGMENT, None
    K = max(0, int(kk))
    n_off = 2 * K + 1
    ns = np.ceil(L * inv_s)
    if ns > max_sections:
        return TOO_LONG, None
    n_sec = max(1, int(ns))
    if n_sec * n_off > max_cells:
        return TOO_LONG, None
    ex, ey = dx / L, dy / L
    return OK, (x1, y1, ex, ey, -ey, ex, half, L, inv_s, inv_u, np.float64(K) + np.float64(0.5), n_sec, n_off, K)


def bins(u, t, g):
    """step 3 of arrays u, t (float64) -> (part, j, b)"""
    x1, y1, ex, ey, nx, ny, half, L, inv_s, inv_u, kc, n_sec, n_off, K = g
    part = (t >= 0) & (t <= L) & (np.abs(u) <= half)
    j = np.minimum(np.floor(np.where(part, t, 0.0) * inv_s).astype(np.int64), n_sec - 1)
    b = np.minimum(np.maximum(np.floor(np.where(part, u, 0.0) * inv_u + kc).astype(np.int64), 0), 2 * K)
    return part, j, b


def cells(frame, g, ok, q, full=False):
    """steps 3 and 4 over a whole frame (buffer-row order) -> int64 [n_sec, n_off, 3]: n_geom, n, q.  full=True evaluates every
    pixel of the frame, not only the segment's bounding box grown by half + 2 px (the sums do not change, only the time)."""
    x1, y1, ex, ey, nx, ny, half, L, inv_s, inv_u, kc, n_sec, n_off, K = g
    h, w = frame.shape
    x2, y2 = x1 + L * ex, y1 + L * ey
    grow = half + 2.0
    ca, cb = int(max(0, np.floor(min(x1, x2) - grow))), int(min(w, np.ceil(max(x1, x2) + grow) + 1))
    ya, yb = int(max(0, np.floor(min(y1, y2) - grow))), int(min(h, np.ceil(max(y1, y2) + grow) + 1))
    if full:
        ca, cb, ya, yb = 0, w, 0, h
    out = np.zeros((n_sec, n_off, 3), np.int64)
    if ca >= cb or ya >= yb:
        return out
    rows = np.arange(h - yb, h - ya)                                  # buffer row r is flipped row h-1-r
    ok, q = ok[rows[0]:rows[-1] + 1, ca:cb], q[rows[0]:rows[-1] + 1, ca:cb]
    x = np.arange(ca, cb, dtype=np.float64)[None, :]
    y = (h - 1 - rows).astype(np.float64)[:, None]
    ax, ay = x - x1, y - y1
    u = ax * nx + ay * ny
    t = ax * ex + ay * ey
    part, j, b = bins(u, t, g)
    np.add.at(out[:, :, 0], (j[part], b[part]), 1)
    np.add.at(out[:, :, 1], (j[part & ok], b[part & ok]), 1)
    np.add.at(out[:, :, 2], (j[part & ok], b[part & ok]), q[part & ok])
    return out


def section(j, c, g, p, sigma):
    """step 5, from the section's cells c (int64 [n_off, 3])"""
    x1, y1, ex, ey, nx, ny, half, L, inv_s, inv_u, kc, n_sec, n_off, K = g
    sec_len, step, wing = np.float64(p["sec_len"]), np.float64(p["step"]), np.float64(p["wing"])
    hw = half - wing
    ub = [np.float64(b - K) * step for b in range(n_off)]
    is_wing = [abs(ub[b]) >= hw for b in range(n_off)]
    o = np.zeros(1, SECTION_DTYPE)[0]
    o["n_geom"] = int(c[:, 0].sum())
    o["n_core"] = sum(int(c[b, 1]) for b in range(n_off) if not is_wing[b])
    o["n_wing"] = n_wing = sum(int(c[b, 1]) for b in range(n_off) if is_wing[b])
    q_wing = sum(int(c[b, 2]) for b in range(n_off) if is_wing[b])
    o["t0"] = np.float64(j) * sec_len
    o["t1"] = min(np.float64(j + 1) * sec_len, L)
    for k in SEC_DOUBLES:
        o[k] = NAN
    if o["n_geom"] == 0:
        o["status"] = SEC_EMPTY
        return o
    if o["n_core"] < p["min_core"] or o["n_wing"] < p["min_wing"]:
        o["status"] = SEC_LOW
        return o
    o["status"] = SEC_OK
    nw, sigma = np.float64(n_wing), np.float64(sigma)
    bkg = np.float64(q_wing) * FIX / nw
    S0 = S1 = S2 = R = np.float64(0.0)
    nc = 0
    for b in range(n_off):
        if is_wing[b] or c[b, 1] <= 0:
            continue
        nb = np.float64(c[b, 1])
        m = np.float64(c[b, 2]) * FIX / nb
        v = m - bkg
        S0 = S0 + v
        S1 = S1 + v * ub[b]
        S2 = S2 + v * ub[b] * ub[b]
        R = R + np.float64(1.0) / nb
        nc += 1
    rate = S0 * step
    rate_err = sigma * step * np.sqrt(R + np.float64(nc) * np.float64(nc) / nw)
    o["bkg"], o["rate"], o["rate_err"] = bkg, rate, rate_err
    if rate >= np.float64(p["k_mom"]) * rate_err:
        with np.errstate(all="ignore"):
            centre = S1 / S0
            d = S2 / S0 - centre * centre
        o["centre"], o["width"] = centre, np.sqrt(d if d > 0 else np.float64(0.0))
    return o


def record(rows, g):
    """step 6"""
    n_sec, n_off, K = g[-3:]
    o = np.zeros(1, STRIP_DTYPE)[0]
    o["n_sec"], o["n_off"], o["K"], o["dev_section"] = n_sec, n_off, K, -1
    for k in STRIP_DOUBLES:
        o[k] = NAN
    okj = [j for j in range(n_sec) if rows[j]["status"] == SEC_OK]
    mom = [j for j in okj if np.isfinite(rows[j]["centre"])]
    o["n_ok"], o["n_mom"] = len(okj), len(mom)
    o["status"] = OK if okj else EMPTY
    if not mom:
        return o
    nc = nw = den = np.float64(0.0)
    for j in mom:
        s = rows[j]
        nc = nc + np.float64(s["n_core"]) * s["centre"]
        nw = nw + np.float64(s["n_core"]) * s["width"]
        den = den + np.float64(s["n_core"])
    mean_centre = nc / den
    o["mean_centre"], o["mean_width"] = mean_centre, nw / den
    dev = None
    for j in mom:
        d = abs(rows[j]["centre"] - mean_centre)
        if dev is None or d > o["max_dev"]:
            dev, o["max_dev"] = j, d
    o["dev_section"] = dev
    return o


def cells_needed(segs, p, max_sections):
    """the largest n_sec * n_off of the segments that fit max_sections rows, at least 1"""
    most = 1
    for s in segs:
        status, g = geometry(s, p, max_sections, 1 << 40)
        if status == OK:
            most = max(most, g[-3] * g[-2])
    return most


def mean_map(c):
    """cells of one segment (CELL_DTYPE [n_sec * n_off] or int64 [.., 3]) -> float32 (float)(q * 2^-30 / n), NaN where n == 0"""
    n, q = (c["n"], c["q"]) if getattr(c, "dtype", None) is not None and c.dtype.names else (c[..., 1], c[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        m = q.astype(np.float64) * FIX / n.astype(np.float64)
    return np.where(n > 0, m, np.nan).astype(np.float32)


def trail_strips(frames, segs, mask=None, skip_bits=0, sigma=None, max_sections=256, max_cells=None, **params):
    """the whole call: frames float32 (or '>f4') [n, h, w] -> (STRIP_DTYPE records [n_seg], SECTION_DTYPE records [n_seg,
    max_sections], CELL_DTYPE records [n_seg, max_cells])"""
    p = dict(DEFAULTS, **params)
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
        mask = None if mask is None else np.asarray(mask).reshape(1, *frames.shape[1:])
    frames = frames.astype(np.float32)                                  # (a big-endian array: the same values, native)
    n = len(frames)
    sig = np.broadcast_to(np.asarray(0.025 if sigma is None else sigma, np.float32), (n,))
    segs = np.asarray(segs, SEGMENT_DTYPE).reshape(-1)
    if max_cells is None:
        max_cells = cells_needed(segs, p, max_sections)
    out = np.zeros(len(segs), STRIP_DTYPE)
    sec = np.zeros((len(segs), max_sections), SECTION_DTYPE)
    cel = np.zeros((len(segs), max_cells), CELL_DTYPE)
    cache = {}
    for i, s in enumerate(segs):
        f = int(s["frame"])
        assert 0 <= f < n
        status, g = geometry(s, p, max_sections, max_cells)
        if status != OK:
            out[i]["status"] = status
            for k in STRIP_DOUBLES:
                out[i][k] = NAN
            continue
        if f not in cache:
            ok = LR.valid(frames[f], p["clip"], None if mask is None else mask[f], skip_bits)
            cache[f] = (ok, np.where(ok, LR.fixed(np.where(ok, frames[f], np.float32(0))), 0))
        c = cells(frames[f], g, *cache[f])
        n_sec, n_off = g[-3], g[-2]
        flat = c.reshape(n_sec * n_off, 3)
        cel[i, :n_sec * n_off]["n_geom"], cel[i, :n_sec * n_off]["n"], cel[i, :n_sec * n_off]["q"] = flat[:, 0], flat[:, 1], flat[:, 2]
        for j in range(n_sec):
            sec[i, j] = section(j, c[j], g, p, sig[f])
        out[i] = record(sec[i], g)
    return out, sec, cel
