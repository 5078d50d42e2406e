"""numpy restatement of the trail subtraction of include/lfdmi.h ("trail subtraction"), built on the trail strips' cells
(tests/strip_ref.py): Python integers up to the model, so every division is spelled out as the truncating one; float64 with the
header's expressions left to right for the geometry; float32 operations, each rounded by numpy and never contracted, for the
interpolation.  The device equals it in every integer, every bit of every double and every bit of every pixel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lc_ref as LR  # noqa: E402
import strip_ref as SR  # noqa: E402

SEGMENT_DTYPE = SR.SEGMENT_DTYPE
SUB_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_off", "<i4"), ("K", "<i4"), ("n_usable", "<i4"), ("n_model", "<i4"),
                      ("n_pix", "<i4"), ("peak_section", "<i4"), ("q_removed", "<i8"), ("removed", "<f8"), ("peak", "<f8")])
OK, BAD_SEGMENT, TOO_LONG, EMPTY = 0, 1, 2, 3
MAX_SMOOTH = 8
DEFAULTS = {"sec_len": 32.0, "step": 1.0, "wing": 6.0, "clip": 0.125, "smooth": 2, "min_sec": 3, "min_n": 8, "min_wing": 8, "apply": 1}
NAN = np.float64(np.nan)
FIX = np.float64(2.0 ** -30)
segment = SR.segment


def tdiv(a, b):
    """C's integer division of Python integers: truncating toward zero (b > 0)"""
    a, b = int(a), int(b)
    return a // b if a >= 0 else -((-a) // b)


def wing_bins(g, p):
    """step 2: [n_off] booleans"""
    half, K, n_off = g[6], g[-1], g[-2]
    hw = half - np.float64(p["wing"])
    return [bool(abs(np.float64(b - K) * np.float64(p["step"])) >= hw) for b in range(n_off)]


def model(c, g, p):
    """steps 2 to 4 from a segment's cells c (int64 [n_sec, n_off, 3]) -> (m float32 [n_sec, n_off], M Python integers likewise,
    n_usable, n_model, the excesses X as a list of lists with None where absent)"""
    n_sec, n_off = g[-3], g[-2]
    R, min_sec, min_n, min_wing = int(p["smooth"]), int(p["min_sec"]), int(p["min_n"]), int(p["min_wing"])
    wing = wing_bins(g, p)
    X = [[None] * n_off for _ in range(n_sec)]
    n_usable = 0
    for j in range(n_sec):
        N = sum(int(c[j, b, 1]) for b in range(n_off) if wing[b])
        Q = sum(int(c[j, b, 2]) for b in range(n_off) if wing[b])
        if N < min_wing:
            continue
        n_usable += 1
        B = tdiv(Q, N)
        for b in range(n_off):
            if not wing[b] and int(c[j, b, 1]) >= min_n:
                X[j][b] = tdiv(c[j, b, 2], c[j, b, 1]) - B
    M = [[0] * n_off for _ in range(n_sec)]
    has = np.zeros((n_sec, n_off), bool)
    for j in range(n_sec):
        for b in range(n_off):
            if wing[b]:
                continue
            x = sorted(X[i][b] for i in range(max(0, j - R), min(n_sec - 1, j + R) + 1) if X[i][b] is not None)
            cnt = len(x)
            if cnt < min_sec:
                continue
            has[j, b] = True
            M[j][b] = x[(cnt - 1) // 2] if cnt % 2 else x[cnt // 2 - 1] + tdiv(x[cnt // 2] - x[cnt // 2 - 1], 2)
    m = (np.array(M, np.int64).astype(np.float64).reshape(n_sec, n_off) * FIX).astype(np.float32)
    return m, M, n_usable, has, X


def value(frame_shape, g, m, full=False):
    """step 5 over a frame (buffer-row order): (geom bool [h, w]: the pixel centre lies in the band; v float32 [h, w]).  Only the
    segment's bounding box grown by half + 2 px is evaluated unless ``full`` (outside it no centre lies in the band)."""
    x1, y1, ex, ey, nx, ny, half, L, inv_s, inv_u, kc, n_sec, n_off, K = g
    h, w = frame_shape
    geom_all, v_all = np.zeros((h, w), bool), np.zeros((h, w), np.float32)
    x2, y2 = x1 + L * ex, y1 + L * ey
    grow = half + 2.0
    ca, cb = int(max(0, np.floor(min(x1, x2) - grow))), int(min(w, np.ceil(max(x1, x2) + grow) + 1))
    ya, yb = int(max(0, np.floor(min(y1, y2) - grow))), int(min(h, np.ceil(max(y1, y2) + grow) + 1))
    if full:
        ca, cb, ya, yb = 0, w, 0, h
    if ca >= cb or ya >= yb:
        return geom_all, v_all
    rows = np.arange(h - yb, h - ya)                                  # buffer row r is flipped row h-1-r
    x = np.arange(ca, cb, dtype=np.float64)[None, :]
    y = (h - 1 - rows).astype(np.float64)[:, None]
    ax, ay = x - x1, y - y1
    u = ax * nx + ay * ny
    t = ax * ex + ay * ey
    geom = (t >= 0) & (t <= L) & (np.abs(u) <= half)
    a = np.where(geom, t, 0.0) * inv_s - np.float64(0.5)
    gg = np.where(geom, u, 0.0) * inv_u + np.float64(K)
    j0 = np.clip(np.floor(a).astype(np.int64), 0, n_sec - 1)
    j1 = np.minimum(j0 + 1, n_sec - 1)
    ft = np.minimum(np.maximum(a - j0.astype(np.float64), 0.0), 1.0).astype(np.float32)
    b0 = np.clip(np.floor(gg).astype(np.int64), 0, 2 * K)
    b1 = np.minimum(b0 + 1, 2 * K)
    fb = np.minimum(np.maximum(gg - b0.astype(np.float64), 0.0), 1.0).astype(np.float32)
    m = np.asarray(m, np.float32)
    v0 = m[j0, b0] + fb * (m[j0, b1] - m[j0, b0])
    v1 = m[j1, b0] + fb * (m[j1, b1] - m[j1, b0])
    v = v0 + ft * (v1 - v0)
    assert v.dtype == np.float32
    geom_all[rows[0]:rows[-1] + 1, ca:cb] = geom
    v_all[rows[0]:rows[-1] + 1, ca:cb] = np.where(geom, v, np.float32(0))
    return geom_all, v_all


def cells_needed(segs, p, max_sections):
    return SR.cells_needed(segs, p, max_sections)


def subtract_trails(frames, segs, mask=None, skip_bits=0, max_sections=256, max_cells=None, **params):
    """the whole call: frames float32 (or '>f4') [n, h, w] or [h, w], never changed -> (the cleaned frames as native float32 (the
    input's values with apply = 0), SUB_DTYPE records [n_seg], float32 tables [n_seg, max_cells])"""
    p = dict(DEFAULTS, **params)
    frames = np.asarray(frames)
    two_d = frames.ndim == 2
    if two_d:
        frames = frames[None]
        mask = None if mask is None else np.asarray(mask).reshape(1, *frames.shape[1:])
    orig = frames.astype(np.float32)                                    # (a copy; a big-endian array: the same values, native)
    clean = orig.copy()
    n = len(orig)
    segs = np.asarray(segs, SEGMENT_DTYPE).reshape(-1)
    if max_cells is None:
        max_cells = cells_needed(segs, p, max_sections)
    out = np.zeros(len(segs), SUB_DTYPE)
    tab = np.zeros((len(segs), max_cells), np.float32)
    cache = {}
    for i, s in enumerate(segs):                                        # ascending index: the order of a pixel's subtractions
        f = int(s["frame"])
        assert 0 <= f < n
        status, g = SR.geometry(s, p, max_sections, max_cells)
        if status != SR.OK:
            out[i]["status"] = status
            out[i]["removed"] = out[i]["peak"] = NAN
            continue
        if f not in cache:
            ok = LR.valid(orig[f], p["clip"], None if mask is None else mask[f], skip_bits)
            with np.errstate(invalid="ignore"):
                live = np.isfinite(orig[f]) & (orig[f] != 0)
            cache[f] = (ok, np.where(ok, LR.fixed(np.where(ok, orig[f], np.float32(0))), 0), live)
        ok, q, live = cache[f]
        c = SR.cells(orig[f], g, ok, q)                                 # step 1: from the frames as passed
        n_sec, n_off, K = g[-3:]
        m, M, n_usable, has, _ = model(c, g, p)
        o = out[i]
        o["n_sec"], o["n_off"], o["K"], o["n_usable"], o["n_model"] = n_sec, n_off, K, n_usable, int(has.sum())
        o["peak_section"], o["peak"] = -1, NAN
        if not has.any():
            o["status"] = EMPTY
            continue
        o["status"] = OK
        tab[i, :n_sec * n_off] = m.reshape(-1)
        best = None
        for j in range(n_sec):
            for b in range(n_off):
                if has[j, b] and (best is None or m[j, b] > m[best]):
                    best = (j, b)
        o["peak_section"], o["peak"] = best[0], np.float64(m[best])
        geom, v = value(orig[f].shape, g, m)
        hit = geom & live & (v != 0)
        o["n_pix"] = int(hit.sum())
        qr = int(LR.fixed(v[hit]).sum())
        o["q_removed"], o["removed"] = qr, np.float64(qr) * FIX
        if p["apply"]:
            clean[f][hit] = clean[f][hit] - v[hit]
    return (clean[0] if two_d else clean), out, tab
