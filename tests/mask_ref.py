"""numpy restatement of the trail masks of include/lfdmi.h ("trail masks"): float64 throughout, the header's expressions left
to right (numpy rounds every operation and never contracts), no hypot.  The device reproduces it byte for byte."""
import math

import numpy as np

SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("bits", "u1"), ("pad", "u1", (3,)), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"),
                          ("y2", "<f8"), ("half", "<f8"), ("cap", "<f8"), ("fill", "<f8")])
STAT_DTYPE = np.dtype([("status", "<i4"), ("n_pix", "<i4")])
OK, BAD_SEGMENT, EMPTY = 0, 1, 2
FILLS = ("none", "zero", "nan", "value")
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def segment(frame=0, x1=0.0, y1=0.0, x2=1.0, y2=0.0, half=0.0, cap=0.0, bits=1, fill=0.0):
    s = np.zeros(1, SEGMENT_DTYPE)[0]
    s["frame"], s["bits"], s["x1"], s["y1"], s["x2"], s["y2"] = frame, bits, x1, y1, x2, y2
    s["half"], s["cap"], s["fill"] = half, cap, fill
    return s


def geometry(s):
    """step 2 -> (x1, y1, ex, ey, nx, ny, half, lo, hi), or None for a bad segment"""
    x1, y1, x2, y2 = (np.float64(s[k]) for k in ("x1", "y1", "x2", "y2"))
    half, cap = np.float64(s["half"]), np.float64(s["cap"])
    for v in (x1, y1, x2, y2):
        if not np.isfinite(v) or abs(v) > 1e6:
            return None
    if not np.isfinite(half) or half < 0 or np.isnan(cap) or cap < 0:
        return None
    dx = x2 - x1
    dy = y2 - y1
    L = np.sqrt(dx * dx + dy * dy)
    if L == 0:
        return None
    ex, ey = dx / L, dy / L
    return x1, y1, ex, ey, -ey, ex, half, -cap, L + cap


def inside(s, h, w):
    """step 3 over a whole frame -> bool [h, w] in buffer-row order, or None for a bad segment"""
    g = geometry(s)
    if g is None:
        return None
    x1, y1, ex, ey, nx, ny, half, lo, hi = g
    x = np.arange(w, dtype=np.float64)[None, :]
    y = (h - 1 - np.arange(h)).astype(np.float64)[:, None]            # buffer row r is flipped row h-1-r
    ax, ay = x - x1, y - y1
    u = ax * nx + ay * ny
    t = ax * ex + ay * ey
    return (np.abs(u) <= half) & (t >= lo) & (t <= hi)


def mask_trails(segs, shape, frames=None, mask=None, fill="none", clear=True):
    """steps 4 - 6.  shape: (n, h, w); frames (float32, for a fill) and mask (uint8) are modified in place; mask None: a new
    plane set.  Returns (mask, stats, frame_counts)."""
    n, h, w = shape
    segs = np.asarray(segs, SEGMENT_DTYPE).reshape(-1)
    assert fill in FILLS and (fill == "none" or (frames is not None and frames.dtype == np.float32))
    if mask is None:
        mask = np.zeros(shape, np.uint8)
    elif clear:
        mask[...] = 0
    stats = np.zeros(len(segs), STAT_DTYPE)
    anyin = np.zeros(shape, bool)
    for i, s in enumerate(segs):                                       # ascending index: the first segment's fill stays
        f = int(s["frame"])
        assert 0 <= f < n and int(s["bits"]) != 0
        m = inside(s, h, w)
        if m is None:
            stats[i] = (BAD_SEGMENT, 0)
            continue
        k = int(m.sum())
        stats[i] = (OK if k else EMPTY, k)
        mask[f][m] |= np.uint8(s["bits"])
        new = m & ~anyin[f]
        if fill == "zero":
            frames[f][new] = np.float32(0.0)
        elif fill == "nan":
            frames[f][new] = QNAN
        elif fill == "value":
            frames[f][new] = np.float64(s["fill"]).astype(np.float32)
        anyin[f] |= m
    return mask, stats, anyin.reshape(n, -1).sum(axis=1).astype(np.int32)


def band_flux_fraction(half):
    """the share of a Gaussian trail's flux (sigma 2 px) within |u| <= half - 1: what a mask of half-width ``half`` holds at least,
    the 1 px being the pixel-centre rule (a pixel whose centre is inside reaches half a pixel further, one whose centre is
    outside was dropped whole)"""
    return math.erf((half - 1.0) / (2.0 * math.sqrt(2.0)))
