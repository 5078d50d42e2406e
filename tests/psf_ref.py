"""The frame seeing of include/lfdmi.h (frame seeing, steps 1 - 5) restated in numpy: the device matches its integers in every
bit and the library's host step its doubles (tests/test_gpu_psf.py); the CPU model tests measure the defaults with it."""
import math

import numpy as np

import stars_ref as S

STAR_DTYPE = np.dtype([("index", "<i4"), ("n_ring", "<i4"), ("Q0", "<i8"), ("Qx", "<i8"), ("Qy", "<i8"), ("Qxx", "<i8"),
                       ("Qyy", "<i8"), ("Qxy", "<i8"), ("Q_ring", "<i8")])
FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_cand", "<i4"), ("n_ok", "<i4"), ("n_packed", "<i4"), ("n_used", "<i4"),
                        ("n_not_candidate", "<i4"), ("n_clipped", "<i4"), ("n_crowded", "<i4"), ("n_bad_pixel", "<i4"),
                        ("pad", "<i4"), ("fwhm_px", "<f8"), ("scatter", "<f8"), ("ell", "<f8")])
OK, NOT_CANDIDATE, CLIPPED, CROWDED, BAD_PIXEL = 0, 1, 2, 3, 4
STATUS_FIELDS = {NOT_CANDIDATE: "n_not_candidate", CLIPPED: "n_clipped", CROWDED: "n_crowded", BAD_PIXEL: "n_bad_pixel"}
SEEING_OK, SEEING_FEW = 0, 1
MAX_SAT = 4096.0
DEFAULTS = {"k_peak": 50.0, "e_max": 0.2, "sat": MAX_SAT, "win": 7, "gap": 2, "ring": 3, "iso": 12, "rad_max": 16,
            "min_stars": 5, "max_used": 256, "pad": 0}
FWHM_PER_SIGMA = 2.3548200450309493


def fixed(v):
    """step 1: q of float32 values (the caller has refused the bad ones)"""
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * 2.0 ** 30).astype(np.int64)


def status_of(x, recs, n_out, i, floor, p):
    """step 2 for record i of a frame x (native float32)"""
    h, w = x.shape
    r = recs[i]
    H = p["win"] + p["gap"] + p["ring"]
    if r["flags"] != 0 or r["rad"] == 0 or r["rad"] > p["rad_max"] or not (r["s_peak"] >= floor):
        return NOT_CANDIDATE
    px, py = int(r["x"]), int(r["y"])
    if px - H < 0 or px + H > w - 1 or py - H < 0 or py + H > h - 1:
        return CLIPPED
    for j in range(n_out):
        if j != i and max(abs(int(recs[j]["x"]) - px), abs(int(recs[j]["y"]) - py)) <= p["iso"]:
            return CROWDED
    sq = x[py - H:py + H + 1, px - H:px + H + 1]
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(sq) | (sq == 0) | (np.abs(sq) > np.float32(p["sat"]))
    return BAD_PIXEL if bad.any() else OK


def sums_of(x, px, py, p):
    """step 3 for an OK record: (n_ring, Q_ring, Q0, Qx, Qy, Qxx, Qyy, Qxy) as Python integers"""
    win, inner = p["win"], p["win"] + p["gap"]
    H = inner + p["ring"]
    q = fixed(x[py - H:py + H + 1, px - H:px + H + 1])
    ax = np.arange(-H, H + 1, dtype=np.int64)
    dy, dx = np.meshgrid(ax, ax, indexing="ij")
    d = np.maximum(np.abs(dy), np.abs(dx))
    ring = d > inner
    n_ring, Q_ring = int(ring.sum()), int(q[ring].sum())
    b = abs(Q_ring) // n_ring * (1 if Q_ring >= 0 else -1)          # C's division truncates
    m = d <= win
    pv, wx, wy = q[m] - b, dx[m], dy[m]
    tot = [int(pv.sum()), int((pv * wx).sum()), int((pv * wy).sum()), int((pv * wx * wx).sum()), int((pv * wy * wy).sum()),
           int((pv * wx * wy).sum())]
    return (n_ring, Q_ring, *tot)


def shape_of(s):
    """step 5 for one packed star: None (not used for its sums) or (width, e)"""
    if s["Q0"] <= 0:
        return None
    q0 = float(s["Q0"])
    mx, my = float(s["Qx"]) / q0, float(s["Qy"]) / q0
    sxx, syy, sxy = float(s["Qxx"]) / q0 - mx * mx, float(s["Qyy"]) / q0 - my * my, float(s["Qxy"]) / q0 - mx * my
    if not sxx > 0.0 or not syy > 0.0:
        return None
    t, d = sxx + syy, sxx - syy
    e = math.sqrt(d * d + 4.0 * (sxy * sxy)) / t
    return FWHM_PER_SIGMA * math.sqrt(t / 2.0), e


def lower_median(v):
    v = sorted(v)
    return v[(len(v) - 1) // 2]


def frame_seeing(packed, n_packed, p):
    """step 5: (status, n_used, fwhm_px, scatter, ell)"""
    wd, el = [], []
    for k in range(n_packed):
        se = shape_of(packed[k])
        if se is not None and se[1] <= p["e_max"]:
            wd.append(se[0])
            el.append(se[1])
    fw = sc = ell = float("nan")
    if wd:
        fw = lower_median(wd)
        sc = 1.4826 * lower_median([abs(v - fw) for v in wd])
        ell = lower_median(el)
    return (SEEING_FEW if len(wd) < p["min_stars"] else SEEING_OK), len(wd), fw, sc, ell


def measure_frame(img, recs, n_out, sigma=None, **params):
    """One frame (any float32 byte order), its finder records and n_out -> (STAR_DTYPE [max_used], a FRAME_DTYPE record,
    the status of each of the n_out records)"""
    p = dict(DEFAULTS, **params)
    sg = S.DEFAULT_SIGMA if sigma is None else np.float32(sigma)
    x = np.array(img, dtype=np.float32)
    floor = np.float32(p["k_peak"] * 3.0 * float(sg))
    out = np.zeros(p["max_used"], STAR_DTYPE)
    fr = np.zeros((), FRAME_DTYPE)
    stats = []
    n_ok = 0
    for i in range(int(n_out)):
        st = status_of(x, recs, int(n_out), i, floor, p)
        stats.append(st)
        if st != OK:
            fr[STATUS_FIELDS[st]] += 1
            continue
        if n_ok < p["max_used"]:
            s = sums_of(x, int(recs[i]["x"]), int(recs[i]["y"]), p)
            out[n_ok] = (i, s[0], *s[2:], s[1])
        n_ok += 1
    fr["n_ok"], fr["n_packed"] = n_ok, min(n_ok, p["max_used"])
    fr["n_cand"] = int(n_out) - int(fr["n_not_candidate"])
    fr["status"], fr["n_used"], fr["fwhm_px"], fr["scatter"], fr["ell"] = frame_seeing(out, int(fr["n_packed"]), p)
    return out, fr, stats


def measure_batch(frames, records, frame_records, sigma=None, **params):
    """(packed [n, max_used], frame records [n])"""
    n = len(frames)
    sig = [None] * n if sigma is None else np.broadcast_to(np.asarray(sigma, np.float32), (n,))
    res = [measure_frame(frames[i], records[i], frame_records[i]["n_out"], sig[i], **params) for i in range(n)]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], FRAME_DTYPE)


def measure_seeing(frames, sigma=None, stars_params=None, **params):
    """the finder's restatement, then this one: (packed, frame records, finder records, finder frame records)"""
    rec, frec = S.find_stars_batch(frames, sigma, **(stars_params or {}))
    out, ofr = measure_batch(frames, rec, frec, sigma, **params)
    return out, ofr, rec, frec
