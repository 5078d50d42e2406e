"""Injection and recovery: add model trails of known line and brightness to frames, detect, and count what comes back -- the
detector's efficiency as a function of the trail's peak (include/lfdmi.h: trail injection).

    python -m lfd_amd.recovery --synth K0:N --peaks 0.05,0.1,0.2,5 --out DIR [--detector radon | radon-short | streak] [--length-frac F] [--null K [--null-scheme S]]

The plan (``draw_trails``), the matching (``match``) and the rows use integer RNG draws and IEEE + - * / sqrt only -- cos and sin
come from ``cos_sin`` below, a fixed sequence of multiplications and additions -- so every machine draws the same plan and
judges a detection the same way.
"""
import math

import numpy as np

from . import _native
from . import inject as _inject

PLAN_DTYPE = np.dtype([("frame", "<i4"), ("peak", "<f8"), ("rho", "<f8"), ("theta", "<f8"), ("t0", "<f8"), ("t1", "<f8")])
ROW_DTYPE = np.dtype([("frame", "<i4"), ("peak", "<f8"), ("rho", "<f8"), ("theta", "<f8"), ("length", "<f8"), ("found", "<i4"),
                      ("matched", "<i4"), ("d_rho", "<f8"), ("d_theta", "<f8"), ("fwhm", "<f8")])
ROW_COLUMNS = ROW_DTYPE.names
# The matching tolerance in Hough cells (1 degree, houghMethod px): the smallest of 1, 1.5, 2, 3 with which every trail of the
# calibration set that the oracle detects is matched (injection and recovery).
K_MATCH = 1.0
THETA_STEPS = 4096

_HALF_PI = math.pi / 2
_SIN_C = [(-1.0) ** k / float(math.factorial(2 * k + 1)) for k in range(14)]
_COS_C = [(-1.0) ** k / float(math.factorial(2 * k)) for k in range(14)]


def cos_sin(theta):
    """(cos, sin) of theta in [0, pi] (scalars or arrays) from the Taylor series about pi/2, 14 terms each in Horner form: the
    truncation is below 1e-17, the rounding a few ulp, and the operations are the same on every machine."""
    x = np.asarray(theta, np.float64) - _HALF_PI
    x2 = x * x
    sn = np.zeros_like(x2)
    cs = np.zeros_like(x2)
    for k in range(13, -1, -1):
        sn = sn * x2 + _SIN_C[k]
        cs = cs * x2 + _COS_C[k]
    return -(sn * x), cs              # cos(theta) = -sin(theta - pi/2), sin(theta) = cos(theta - pi/2)


def draw_trails(n_frames, shape, seed, peaks, length=None):
    """One trail per frame through the frame's interior, as PLAN_DTYPE records: a point with integer coordinates in the middle
    half of the frame, theta = j pi / THETA_STEPS (j an integer draw) rounded to float32 and widened, rho = the line through the
    point.  peaks: frame i takes peaks[i % len(peaks)].  length None: the trail crosses the whole frame (t0 / t1 infinite);
    otherwise it extends length / 2 px either side of the point."""
    h, w = shape
    rng = np.random.default_rng(np.random.PCG64(int(seed)))
    x0 = (w // 4 + rng.integers(0, max(1, w // 2), n_frames)).astype(np.float64)
    y0 = (h // 4 + rng.integers(0, max(1, h // 2), n_frames)).astype(np.float64)
    j = rng.integers(0, THETA_STEPS, n_frames)
    theta = (j.astype(np.float64) * (math.pi / THETA_STEPS)).astype(np.float32).astype(np.float64)
    c, s = cos_sin(theta)
    plan = np.zeros(n_frames, PLAN_DTYPE)
    plan["frame"] = np.arange(n_frames)
    plan["peak"] = [float(peaks[i % len(peaks)]) for i in range(n_frames)]
    plan["rho"] = x0 * c + y0 * s
    plan["theta"] = theta
    if length is None:
        plan["t0"], plan["t1"] = -np.inf, np.inf
    else:
        tm = (x0 - plan["rho"] * c) * -s + (y0 - plan["rho"] * s) * c
        plan["t0"], plan["t1"] = tm - 0.5 * float(length), tm + 0.5 * float(length)
    return plan


def shorten(plan, shape, frac, seed):
    """The plan with every trail cut to the fraction ``frac`` of its crossing of the frame, at a random place along it: with
    (ta, tb) the trail's extent inside the frame, t0 = ta + u (1 - frac) (tb - ta) and t1 = t0 + frac (tb - ta), u = an integer draw / 2^20
    from a stream of its own (seeded by (seed, 1)), so ``draw_trails`` draws what it always drew.  frac = 1: the plan
    itself."""
    frac = float(frac)
    if not 0.0 < frac <= 1.0:
        raise ValueError("length_frac must be in (0, 1]")
    if frac == 1.0:
        return plan
    out = np.array(plan, PLAN_DTYPE)
    u = np.random.default_rng(np.random.PCG64([int(seed), 1])).integers(0, 1 << 20, len(out)).astype(np.float64) / float(1 << 20)
    for i in range(len(out)):
        ta, tb = extent(float(out["rho"][i]), float(out["theta"][i]), float(out["t0"][i]), float(out["t1"][i]), shape)
        if ta > tb:
            continue
        out["t0"][i] = ta + u[i] * (1.0 - frac) * (tb - ta)
        out["t1"][i] = out["t0"][i] + frac * (tb - ta)
    return out


def plan_checksum(plan):
    """SHA-256 of the plan's bytes (tests/golden/inject_plan.json)"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(plan, PLAN_DTYPE).tobytes()).hexdigest()


def to_inject(plan, table=0):
    """PLAN_DTYPE -> the INJECT_DTYPE records of ``Context.inject_trails``: amplitude = peak (tables of peak 1)"""
    tr = np.zeros(len(plan), _native.INJECT_DTYPE)
    for k in ("frame", "rho", "theta", "t0", "t1"):
        tr[k] = plan[k]
    tr["table"] = table
    tr["amplitude"] = plan["peak"]
    return tr


def extent(rho, theta, t0, t1, shape):
    """(ta, tb): the part of [t0, t1] on which the line's point f + t d lies inside the frame [0, W-1] x [0, H-1]; ta > tb when
    there is none.  Scalars."""
    h, w = shape
    c, s = (float(v) for v in cos_sin(theta))
    fx, fy, dx, dy = rho * c, rho * s, -s, c
    ta = t0 if np.isfinite(t0) else -np.inf
    tb = t1 if np.isfinite(t1) else np.inf
    for f, d, top in ((fx, dx, w - 1.0), (fy, dy, h - 1.0)):
        if d == 0.0:
            if f < 0.0 or f > top:
                return 1.0, 0.0
            continue
        a, b = (0.0 - f) / d, (top - f) / d
        ta, tb = max(ta, min(a, b)), min(tb, max(a, b))
    return ta, tb


def match(records, trails, params_bright, params_dim, k=K_MATCH, shape=None):
    """Is the detection record of a trail's frame the injected trail?  records: RESULT_DTYPE, one per frame; trails: PLAN_DTYPE
    records with theta in [0, pi] (what ``draw_trails`` gives; ``cos_sin`` covers that range only); shape: the frames' (h, w).
    A record matches when it has found != 0, |d_theta| <= k degrees and |d_rho| <= k * houghMethod of the pass that found it (found 1: params_bright, 2: params_dim): k Hough cells either way.
    d_theta = theta_detected - theta_injected; d_rho = the distance of the injected extent's middle point from the detected
    line, along the detected normal.  A detected line near theta = 0 / pi may carry the other orientation: (rho, theta) and
    (-rho, theta -+ pi) are one line, so |d_theta| > pi/2 is folded by pi and d_rho changes sign with it.
    Returns (matched bool, d_rho, d_theta, length); d_rho / d_theta are NaN where nothing was found."""
    if shape is None:
        raise ValueError("match needs the frames' shape")
    n = len(trails)
    if n and not ((trails["theta"] >= 0) & (trails["theta"] <= math.pi)).all():
        raise ValueError("match needs trails with theta in [0, pi]")
    matched = np.zeros(n, bool)
    d_rho = np.full(n, np.nan)
    d_theta = np.full(n, np.nan)
    length = np.zeros(n)
    for i, tr in enumerate(trails):
        rho, theta = float(tr["rho"]), float(tr["theta"])
        ta, tb = extent(rho, theta, float(tr["t0"]), float(tr["t1"]), shape)
        length[i] = max(0.0, tb - ta)
        rec = records[int(tr["frame"])]
        found = int(rec["found"])
        if found == 0 or not ta <= tb:
            continue
        c, s = (float(v) for v in cos_sin(theta))
        tm = 0.5 * (ta + tb)
        mx, my = rho * c + tm * -s, rho * s + tm * c
        thd = float(rec["theta"])
        cd, sd = (float(v) for v in cos_sin(thd))
        dist = mx * cd + my * sd - float(rec["rho"])
        dth = thd - theta
        if dth > _HALF_PI:
            dth, dist = dth - math.pi, -dist
        elif dth < -_HALF_PI:
            dth, dist = dth + math.pi, -dist
        d_rho[i], d_theta[i] = dist, dth
        cell = float((params_bright if found == 1 else params_dim)["houghMethod"])
        matched[i] = abs(dth) <= k * (math.pi / 180) and abs(dist) <= k * cell
    return matched, d_rho, d_theta, length


def make_rows(records, trails, params_bright, params_dim, shape, k=K_MATCH, measured=None):
    """One ROW_DTYPE row per injected trail from its frame's detection record (and, when given, the TRAIL_DTYPE records of
    ``measure_trails``: fwhm of a measured trail, else NaN)."""
    matched, d_rho, d_theta, length = match(records, trails, params_bright, params_dim, k=k, shape=shape)
    rows = np.zeros(len(trails), ROW_DTYPE)
    for key in ("frame", "peak", "rho", "theta"):
        rows[key] = trails[key]
    rows["length"] = length
    rows["found"] = [int(records[int(t["frame"])]["found"]) for t in trails]
    rows["matched"] = matched
    rows["d_rho"], rows["d_theta"] = d_rho, d_theta
    rows["fwhm"] = np.nan
    if measured is not None:
        for i, t in enumerate(trails):
            m = measured[int(t["frame"])]
            if int(m["status"]) == _native.TRAIL_OK:
                rows["fwhm"][i] = float(m["fwhm"])
    return rows


def match_streaks(records, n_streaks, trails, shape, reach):
    """Is one of the found streaks of a trail's frame the injected trail?  records: STREAK_DTYPE [n, K] and n_streaks [n] of
    ``streaks.search_frames``; trails: PLAN_DTYPE records; reach: L b / 2 px.  A found streak matches when both its ends lie
    within ``reach`` of the injected segment's line and its midpoint lies inside the injected extent (the part of [t0, t1] on
    the frame).  Returns (matched bool, d_rho, d_theta, length, found): of the first matching streak in peel order, otherwise
    of the frame's first found streak; d_rho is the distance of the streak's midpoint from the injected line, d_theta the
    difference of the normals' angles folded into [-pi/2, pi/2]; NaN where nothing was found."""
    n = len(trails)
    matched = np.zeros(n, bool)
    found = np.zeros(n, np.int64)
    d_rho = np.full(n, np.nan)
    d_theta = np.full(n, np.nan)
    length = np.zeros(n)
    for i, tr in enumerate(trails):
        rho, theta = float(tr["rho"]), float(tr["theta"])
        ta, tb = extent(rho, theta, float(tr["t0"]), float(tr["t1"]), shape)
        length[i] = max(0.0, tb - ta)
        f = int(tr["frame"])
        found[i] = int(n_streaks[f])
        c, s = math.cos(theta), math.sin(theta)
        for k in range(found[i]):
            rec = records[f][k]
            ends = [abs(float(x) * c + float(y) * s - rho) for x, y in ((rec["x1"], rec["y1"]), (rec["x2"], rec["y2"]))]
            mx, my = 0.5 * (float(rec["x1"]) + float(rec["x2"])), 0.5 * (float(rec["y1"]) + float(rec["y2"]))
            ok = ta <= tb and max(ends) <= reach and ta <= -mx * s + my * c <= tb
            if ok or k == 0:
                d_rho[i] = mx * c + my * s - rho
                d_theta[i] = (float(rec["theta"]) - theta + _HALF_PI) % math.pi - _HALF_PI
            if ok:
                matched[i] = True
                break
    return matched, d_rho, d_theta, length, found


def streak_rows(records, n_streaks, trails, shape, reach):
    """One ROW_DTYPE row per injected trail from its frame's streak records (``match_streaks``); found: the frame's n_streaks"""
    matched, d_rho, d_theta, length, found = match_streaks(records, n_streaks, trails, shape, reach)
    rows = np.zeros(len(trails), ROW_DTYPE)
    for key in ("frame", "peak", "rho", "theta"):
        rows[key] = trails[key]
    rows["length"], rows["found"], rows["matched"] = length, found, matched
    rows["d_rho"], rows["d_theta"] = d_rho, d_theta
    rows["fwhm"] = np.nan
    return rows


def radon_records(lines):
    """RADON_DTYPE records -> RESULT_DTYPE records ``match`` can judge: found 1 (so that the cell is params_bright's
    houghMethod) where the search found a line, with that line's rho and theta"""
    recs = np.zeros(len(lines), _native.RESULT_DTYPE)
    recs["found"] = lines["found"] != 0
    recs["rho"], recs["theta"] = lines["rho"], lines["theta"]
    return recs


def run(ctx, frames, cats, rs, trails, tables, table_step, params_bright=None, params_dim=None, subsample=4, profiles=False,
        k=K_MATCH, detector="hough", radon_params=None, sigma=None, short_params=None, null=0, null_scheme="scramble",
        streak_params=None):
    """Copy ``frames`` ((n, h, w) float32 numpy or torch CUDA), inject the plan ``trails`` (tables of peak 1: see
    ``inject.normalise_peak``), run ``detect_batch`` and match: ROW_DTYPE rows, one per trail.  cats: the frames' catalogues
    (a list of dicts, a packed dict or None) and rs their remove_stars parameters; profiles=True also runs ``measure_trails``
    and fills fwhm.  detector="radon": the stars are removed (``remove_stars``) and the faint-trail search
    (include/lfdmi.h: faint-trail search; ``radon_params``, ``sigma``) takes the detector's place; its line is matched by the
    same rule, with params_bright's houghMethod as the cell.  detector="radon-short": the short-trail search (steps 10 - 12
    of that definition; ``short_params``) instead, and the parent line of a frame's first record is matched.  null=K > 0 (the
    radon detectors): the frames' null peaks of that search (include/lfdmi.h: null peaks; frame f has seed f) are measured on
    the same frames, and the call returns (rows, fap): float64 [n trails], ``radon.false_alarm`` of each trail's frame's line
    among its frame's K null peaks; ``null_scheme``: how the null frames are made ("scramble", "signflip", "rowshift",
    "colshift": steps 21 - 22 of that definition).  detector="streak": the stars are removed and the short-streak search
    (include/lfdmi.h: short-streak search; ``streak_params``, ``sigma``) runs; a trail is matched by ``match_streaks`` with
    reach L b / 2."""
    if null_scheme not in _native.RADON_NULL_SCHEMES:
        raise ValueError("null_scheme: one of %s" % ", ".join(_native.RADON_NULL_SCHEMES))
    if detector not in ("hough", "radon", "radon-short", "streak"):
        raise ValueError("detector: 'hough', 'radon', 'radon-short' or 'streak'")
    if null and detector in ("hough", "streak"):
        raise ValueError("null: the null peaks belong to the radon detectors")
    from .catalogs import pack_catalogs
    from .detecttrails import default_params
    pb, pd, _ = default_params()
    pb = params_bright or pb
    pd = params_dim or pd
    work = frames.clone() if _native._is_dev(frames) else np.array(frames, np.float32, order="C")
    n, h, w = work.shape
    packed = pack_catalogs(list(cats)) if isinstance(cats, (list, tuple)) else cats
    ctx.inject_trails(work, to_inject(trails), np.asarray(tables, np.float32), table_step, subsample=subsample)
    if detector == "streak":
        from . import streaks as _streaks
        if packed is not None:
            ctx.remove_stars(work, packed, rs)
        sp = _streaks.as_params(streak_params)
        full = dict(_streaks.default_params(), **sp)
        recs, ns = _streaks.search_frames(ctx, work, sigma=sigma, **sp)
        return streak_rows(recs, ns, trails, (h, w), full["length"] * full["bin"] / 2.0)
    if detector in ("radon", "radon-short"):
        from . import radon as _radon
        if packed is not None:
            ctx.remove_stars(work, packed, rs)
        rp = _radon.as_params(radon_params)
        with _native.Radon(ctx, (h, w), max_frames=min(n, 16), **rp) as search:
            if detector == "radon":
                kind, sp = "lines", {}
                lines = search.search(work, sigma=sigma)
            else:
                kind, sp = "short", _radon.as_short_params(short_params, rp.get("bin", _radon.RadonParams.bin))
                lines = search.search_short(work, sigma=sigma, **sp)[0][:, 0]
            peaks = search.null(work, K=int(null), kind=kind, sigma=sigma, scheme=null_scheme, **sp)["snr"] if null else None
        rows = make_rows(radon_records(lines), trails, pb, pd, (h, w), k=k)
        if peaks is None:
            return rows
        return rows, np.array([_radon.false_alarm(lines["snr"][int(t["frame"])], peaks[int(t["frame"])]) for t in trails], np.float64)
    recs = ctx.detect_batch(work, pb, pd, packed, rs if packed is not None else None)
    measured = None
    if profiles:
        measured, _ = ctx.measure_trails(work, recs, packed, rs if packed is not None else None)
    return make_rows(recs, trails, pb, pd, (h, w), k=k, measured=measured)


def wilson(recovered, n, z=1.0):
    """Wilson score interval of recovered / n at z standard deviations: (lo, hi); (nan, nan) for n = 0"""
    if n == 0:
        return float("nan"), float("nan")
    p = recovered / n
    den = 1.0 + z * z / n
    mid = (p + z * z / (2.0 * n)) / den
    half = z * math.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / den
    return mid - half, mid + half


def completeness(rows, edges, z=1.0, fap=None):
    """Per peak bin [edges[i], edges[i+1]): n, recovered (matched rows), efficiency and its Wilson interval at z sigmas; with
    ``fap`` (one false-alarm estimate per row, ``run(..., null=K)``) also median_fap, the median over the bin's recovered
    trails (NaN without one)"""
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (rows["peak"] >= lo) & (rows["peak"] < hi)
        n, r = int(sel.sum()), int(rows["matched"][sel].sum())
        wl, wh = wilson(r, n, z)
        out.append({"lo": float(lo), "hi": float(hi), "n": n, "recovered": r, "efficiency": r / n if n else float("nan"),
                    "wilson_lo": wl, "wilson_hi": wh})
        if fap is not None:
            got = np.asarray(fap, np.float64)[sel & (rows["matched"] != 0)]
            out[-1]["median_fap"] = float(np.median(got)) if got.size else float("nan")
    return out


def write_recovery(path, rows):
    """recovery.txt: a header line, then one row per injected trail (floats with repr, so that read_recovery returns them)"""
    with open(path, "w") as f:
        f.write(" ".join(ROW_COLUMNS) + "\n")
        for r in rows:
            f.write(" ".join(str(int(r[k])) if ROW_DTYPE[k].kind == "i" else repr(float(r[k])) for k in ROW_COLUMNS) + "\n")


def read_recovery(path):
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == ROW_COLUMNS[0]:
                continue
            rows.append(tuple(int(v) if ROW_DTYPE[k].kind == "i" else float(v) for k, v in zip(ROW_COLUMNS, parts)))
    return np.array(rows, ROW_DTYPE)


def peak_edges(peaks):
    """bin edges that put every distinct peak into a bin of its own"""
    p = sorted(set(float(v) for v in peaks))
    mids = [0.5 * (a + b) for a, b in zip(p[:-1], p[1:])]
    return [0.0] + mids + [math.inf]


def format_table(table):
    """the completeness table as text; a table made with ``fap`` has a last column, median_fap"""
    fap = bool(table) and "median_fap" in table[0]
    lines = ["%10s %10s %6s %9s %10s %9s %9s" % ("peak_lo", "peak_hi", "n", "recovered", "efficiency", "wilson_lo", "wilson_hi") +
             (" %10s" % "median_fap" if fap else "")]
    for b in table:
        lines.append("%10.4g %10.4g %6d %9d %10.4f %9.4f %9.4f" % (b["lo"], b["hi"], b["n"], b["recovered"], b["efficiency"],
                                                                  b["wilson_lo"], b["wilson_hi"]) +
                     (" %10.4f" % b["median_fap"] if fap else ""))
    return "\n".join(lines)


def main(argv=None):
    import argparse
    import os
    from . import synth
    from .detecttrails import default_params
    ap = argparse.ArgumentParser(description="inject model trails into synthetic frames, detect, print the completeness table")
    ap.add_argument("--synth", required=True, metavar="K0:N", help="synthetic frames K0 .. K0+N-1 (those without a streak of their own)")
    ap.add_argument("--peaks", required=True, help="comma-separated trail peaks in frame units")
    ap.add_argument("--out", required=True, help="directory for recovery.txt")
    ap.add_argument("--sigma", type=float, default=2.0, help="Gaussian cross-section sigma in px")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--profiles", action="store_true", help="also measure the recovered trails' fwhm")
    ap.add_argument("--detector", choices=("hough", "radon", "radon-short", "streak"), default="hough",
                    help="hough: the detector (default); radon: the faint-trail search in its place; radon-short: its "
                         "short-trail search, matched by the candidate's parent line; streak: the short-streak search, "
                         "matched by both ends within L b / 2 px of the injected line and the midpoint inside its extent")
    ap.add_argument("--streak-length", type=int, default=None, help="--detector streak: lfdmi_streak_params.length")
    ap.add_argument("--bin", type=int, default=None, help="--detector radon / radon-short: lfdmi_radon_params.bin")
    ap.add_argument("--length-frac", type=float, default=1.0,
                    help="inject every trail over this fraction of its crossing, at a random place along it (default 1: the whole crossing)")
    ap.add_argument("--null", type=int, default=0, metavar="K",
                    help="--detector radon / radon-short: also measure K null peaks per frame and add the median false-alarm "
                         "estimate of the recovered trails to the table")
    ap.add_argument("--null-scheme", default="scramble", choices=tuple(_native.RADON_NULL_SCHEMES),
                    help="--null K: how the null frames are made (default scramble; signflip, rowshift and colshift leave every "
                         "pixel in its place, row or column)")
    a = ap.parse_args(argv)
    if a.null and a.detector in ("hough", "streak"):
        ap.error("--null needs --detector radon or radon-short")
    k0, n = (int(v) for v in a.synth.split(":"))
    peaks = [float(v) for v in a.peaks.split(",")]
    frames, cats, truths = synth.make_frames(k0, n, with_truth=True)
    keep = [i for i, t in enumerate(truths) if t["streak"] == "none"]
    if not keep:
        raise SystemExit("no frame without a streak of its own in that range")
    frames, cats = np.ascontiguousarray(frames[keep]), [cats[i] for i in keep]
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    table, step = _inject.gaussian_table(a.sigma)
    plan = shorten(draw_trails(len(keep), frames.shape[1:], a.seed, peaks), frames.shape[1:], a.length_frac, a.seed)
    with _native.Context(0, frames.shape[1], frames.shape[2], 16) as ctx:
        rows = run(ctx, frames, cats, rs, plan, _inject.normalise_peak(table), step, pb, pd, profiles=a.profiles,
                   detector=a.detector, radon_params={"bin": a.bin} if a.bin else None, null=a.null, null_scheme=a.null_scheme,
                   streak_params=dict(({"bin": a.bin} if a.bin else {}), **({"length": a.streak_length} if a.streak_length else {})))
    rows, fap = rows if a.null else (rows, None)
    os.makedirs(a.out, exist_ok=True)
    write_recovery(os.path.join(a.out, "recovery.txt"), rows)
    print(format_table(completeness(rows, peak_edges(peaks), fap=fap)))


if __name__ == "__main__":
    main()
