"""numpy restatement of the light curves of include/lfdmi.h ("light curves"): float64 throughout, the header's expressions left to
right (numpy rounds every operation and never contracts), integer sums in int64.  The device reproduces it in every integer and
every bit of every double."""
import numpy as np

SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                          ("half", "<f8"), ("bg_in", "<f8"), ("bg_out", "<f8")])
LC_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_ok", "<i4"), ("first_ok", "<i4"), ("last_ok", "<i4"),
                     ("peak_section", "<i4"), ("dof", "<i4"), ("pad", "<i4"),
                     ("mean_rate", "<f8"), ("mean_rate_err", "<f8"), ("chi2", "<f8"), ("peak_rate", "<f8"), ("length", "<f8"),
                     ("flux", "<f8"), ("flux_err", "<f8")])
SECTION_DTYPE = np.dtype([("status", "<i4"), ("n_geom", "<i4"), ("n_core", "<i4"), ("n_sky", "<i4"),
                          ("q_core", "<i8"), ("q_sky", "<i8"), ("t0", "<f8"), ("t1", "<f8"),
                          ("mean", "<f8"), ("bkg", "<f8"), ("sb", "<f8"), ("flux", "<f8"), ("flux_err", "<f8"),
                          ("rate", "<f8"), ("rate_err", "<f8"), ("coverage", "<f8")])
OK, BAD_SEGMENT, TOO_LONG, EMPTY = 0, 1, 2, 3
SEC_OK, SEC_LOW, SEC_EMPTY = 0, 1, 2
MAX_SECTIONS = 1024
MAX_BG = 64.0
DEFAULTS = {"sec_len": 32.0, "clip": 0.125, "min_core": 32, "min_sky": 32}
LC_DOUBLES = ("mean_rate", "mean_rate_err", "chi2", "peak_rate", "length", "flux", "flux_err")
SEC_DOUBLES = ("mean", "bkg", "sb", "flux", "flux_err", "rate", "rate_err", "coverage")
NAN = np.float64(np.nan)


def segment(frame=0, x1=0.0, y1=0.0, x2=1.0, y2=0.0, half=4.0, bg_in=None, bg_out=None):
    s = np.zeros(1, SEGMENT_DTYPE)[0]
    s["frame"], s["x1"], s["y1"], s["x2"], s["y2"], s["half"] = frame, x1, y1, x2, y2, half
    s["bg_in"] = half + 4.0 if bg_in is None else bg_in
    s["bg_out"] = min(float(s["bg_in"]) + 16.0, MAX_BG) if bg_out is None else bg_out
    return s


def fixed(v):
    """step 1: q of float32 values (the caller masks the invalid ones)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(v.astype(np.float64) * 2.0 ** 30).astype(np.int64)


def valid(frame, clip, mask=None, skip_bits=0):
    """step 1: bool [h, w] of a float32 frame"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(frame) & (frame != 0) & (np.abs(frame) <= np.float32(clip))
    if mask is not None:
        ok &= (mask & np.uint8(skip_bits)) == 0
    return ok


def geometry(s, sec_len, max_sections):
    """step 2 -> (status, (x1, y1, ex, ey, nx, ny, half, bg_in, bg_out, L, inv, n_sec) or None)"""
    x1, y1, x2, y2 = (np.float64(s[k]) for k in ("x1", "y1", "x2", "y2"))
    half, bg_in, bg_out = (np.float64(s[k]) for k in ("half", "bg_in", "bg_out"))
    for v in (x1, y1, x2, y2):
        if not np.isfinite(v) or abs(v) > 1e6:
            return BAD_SEGMENT, None
    if not np.isfinite(half) or not half > 0 or np.isnan(bg_in) or np.isnan(bg_out):
        return BAD_SEGMENT, None
    if bg_in < half or bg_out < bg_in or bg_out > MAX_BG:
        return BAD_SEGMENT, None
    dx = x2 - x1
    dy = y2 - y1
    L = np.sqrt(dx * dx + dy * dy)
    if L == 0:
        return BAD_SEGMENT, None
    inv = np.float64(1.0) / np.float64(sec_len)
    ns = np.ceil(L * inv)
    if ns > max_sections:
        return TOO_LONG, None
    ex, ey = dx / L, dy / L
    return OK, (x1, y1, ex, ey, -ey, ex, half, bg_in, bg_out, L, inv, max(1, int(ns)))


def sums(frame, g, ok, q, full=False):
    """steps 3 and 4 over a whole frame (buffer-row order) -> int64 [n_sec, 5]: n_geom, n_core, n_sky, Q_core, Q_sky.
    full=True evaluates every pixel of the frame."""
    x1, y1, ex, ey, nx, ny, half, bg_in, bg_out, L, inv, n_sec = g
    h, w = frame.shape
    # only the segment's bounding box, grown by bg_out + 2 px, is evaluated: a pixel outside it has t outside [0, L] or |u| above
    # bg_out by more than a pixel, so it belongs to nothing (the sums do not change, only the time)
    x2, y2 = x1 + L * ex, y1 + L * ey
    grow = bg_out + 2.0
    ca, cb = int(max(0, np.floor(min(x1, x2) - grow))), int(min(w, np.ceil(max(x1, x2) + grow) + 1))
    ya, yb = int(max(0, np.floor(min(y1, y2) - grow))), int(min(h, np.ceil(max(y1, y2) + grow) + 1))
    if full:
        ca, cb, ya, yb = 0, w, 0, h
    out = np.zeros((n_sec, 5), np.int64)
    if ca >= cb or ya >= yb:
        return out
    rows = np.arange(h - yb, h - ya)                                  # buffer row r is flipped row h-1-r
    ok, q = ok[rows[0]:rows[-1] + 1, ca:cb], q[rows[0]:rows[-1] + 1, ca:cb]
    x = np.arange(ca, cb, dtype=np.float64)[None, :]
    y = (h - 1 - rows).astype(np.float64)[:, None]
    ax, ay = x - x1, y - y1
    u = ax * nx + ay * ny
    t = ax * ex + ay * ey
    part = (t >= 0) & (t <= L)
    j = np.minimum(np.floor(np.where(part, t, 0.0) * inv).astype(np.int64), n_sec - 1)
    au = np.abs(u)
    core = part & (au <= half)
    sky = part & ~core & (au >= bg_in) & (au <= bg_out)
    np.add.at(out[:, 0], j[core], 1)
    np.add.at(out[:, 1], j[core & ok], 1)
    np.add.at(out[:, 2], j[sky & ok], 1)
    np.add.at(out[:, 3], j[core & ok], q[core & ok])
    np.add.at(out[:, 4], j[sky & ok], q[sky & ok])
    return out


def section(j, s5, g, p, sigma):
    """step 5"""
    x1, y1, ex, ey, nx, ny, half, bg_in, bg_out, L, inv, n_sec = g
    sec_len = np.float64(p["sec_len"])
    o = np.zeros(1, SECTION_DTYPE)[0]
    o["n_geom"], o["n_core"], o["n_sky"], o["q_core"], o["q_sky"] = (int(v) for v in s5)
    o["t0"] = np.float64(j) * sec_len
    o["t1"] = min(np.float64(j + 1) * sec_len, L)
    for k in SEC_DOUBLES:
        o[k] = NAN
    if o["n_geom"] == 0:
        o["status"] = SEC_EMPTY
        return o
    if o["n_core"] < p["min_core"] or o["n_sky"] < p["min_sky"]:
        o["status"] = SEC_LOW
        return o
    o["status"] = SEC_OK
    nc, ns, width, sigma = np.float64(o["n_core"]), np.float64(o["n_sky"]), np.float64(2.0) * half, np.float64(sigma)
    s_core = np.float64(o["q_core"]) * np.float64(2.0 ** -30)
    s_sky = np.float64(o["q_sky"]) * np.float64(2.0 ** -30)
    mean = s_core / nc
    bkg = s_sky / ns
    sb = mean - bkg
    o["mean"], o["bkg"], o["sb"] = mean, bkg, sb
    o["flux"] = sb * nc
    o["flux_err"] = sigma * np.sqrt(nc + nc * nc / ns)
    o["rate"] = sb * width
    o["rate_err"] = sigma * np.sqrt(np.float64(1.0) / nc + np.float64(1.0) / ns) * width
    o["coverage"] = nc / np.float64(o["n_geom"])
    return o


def record(rows, n_sec):
    """step 6"""
    o = np.zeros(1, LC_DTYPE)[0]
    o["n_sec"] = n_sec
    o["first_ok"] = o["last_ok"] = o["peak_section"] = -1
    for k in LC_DOUBLES:
        o[k] = NAN
    okj = [j for j in range(n_sec) if rows[j]["status"] == SEC_OK]
    o["n_ok"], o["dof"] = len(okj), len(okj) - 1
    if not okj:
        o["status"] = EMPTY
        return o
    o["status"], o["first_ok"], o["last_ok"] = OK, okj[0], okj[-1]
    num = den = w = length = np.float64(0.0)
    peak = None
    for j in okj:
        s = rows[j]
        num = num + np.float64(s["n_core"]) * s["rate"]
        den = den + np.float64(s["n_core"])
        w = w + np.float64(1.0) / (s["rate_err"] * s["rate_err"])
        length = length + (s["t1"] - s["t0"])
        if peak is None or s["rate"] > rows[peak]["rate"]:
            peak = j
    mean_rate = num / den
    err = np.float64(1.0) / np.sqrt(w)
    chi2 = np.float64(0.0)
    for j in okj:
        d = (rows[j]["rate"] - mean_rate) / rows[j]["rate_err"]
        chi2 = chi2 + d * d
    o["mean_rate"], o["mean_rate_err"], o["chi2"] = mean_rate, err, chi2
    o["peak_section"], o["peak_rate"] = peak, rows[peak]["rate"]
    o["length"], o["flux"], o["flux_err"] = length, mean_rate * length, err * length
    return o


def light_curves(frames, segs, mask=None, skip_bits=0, sigma=None, max_sections=256, **params):
    """the whole call: frames float32 (or '>f4') [n, h, w] -> (LC_DTYPE records [n_seg], SECTION_DTYPE records [n_seg,
    max_sections])"""
    p = dict(DEFAULTS, **params)
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
        mask = None if mask is None else np.asarray(mask).reshape(1, *frames.shape[1:])
    frames = frames.astype(np.float32)                                  # (a big-endian array: the same values, native)
    n = len(frames)
    sig = np.broadcast_to(np.asarray(0.025 if sigma is None else sigma, np.float32), (n,))
    segs = np.asarray(segs, SEGMENT_DTYPE).reshape(-1)
    out = np.zeros(len(segs), LC_DTYPE)
    sec = np.zeros((len(segs), max_sections), SECTION_DTYPE)
    cache = {}
    for i, s in enumerate(segs):
        f = int(s["frame"])
        assert 0 <= f < n
        status, g = geometry(s, p["sec_len"], max_sections)
        if status != OK:
            out[i]["status"] = status
            for k in LC_DOUBLES:
                out[i][k] = NAN
            continue
        if f not in cache:
            ok = valid(frames[f], p["clip"], None if mask is None else mask[f], skip_bits)
            cache[f] = (ok, np.where(ok, fixed(np.where(ok, frames[f], np.float32(0))), 0))
        s5 = sums(frames[f], g, *cache[f])
        n_sec = g[-1]
        for j in range(n_sec):
            sec[i, j] = section(j, s5[j], g, p, sig[f])
        out[i] = record(sec[i], n_sec)
    return out, sec
