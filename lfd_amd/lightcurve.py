"""Light curves: how a trail's brightness changes along it, in sections of the segment (include/lfdmi.h: light curves).
``Context.light_curves`` is the device call; this module holds the sky-band rule, the segments of every measurement unit's records
(through ``masks.segments_from_*``, so the half-width rule stays in one place), a one-call helper, magnitudes, the variability
figure and the row formats of lightcurves.txt and lightcurve_summary.txt.
"""
import math

import numpy as np

from . import _native

SEGMENT_DTYPE = _native.LC_SEGMENT_DTYPE
LC_DTYPE = _native.LC_DTYPE
SECTION_DTYPE = _native.LC_SECTION_DTYPE
OK, BAD_SEGMENT, TOO_LONG, EMPTY = _native.LC_OK, _native.LC_BAD_SEGMENT, _native.LC_TOO_LONG, _native.LC_EMPTY
SEC_OK, SEC_LOW, SEC_EMPTY = _native.LC_SEC_OK, _native.LC_SEC_LOW, _native.LC_SEC_EMPTY
MAX_BG = _native.LC_MAX_BG
PARAM_NAMES = tuple(k for k, _ in _native.LcParamsStruct._fields_)
LC_COLUMNS = ("run", "camcol", "filter", "field", "source", "line", "section", "t0", "t1", "n_geom", "n_core", "n_sky", "bkg", "flux",
              "flux_err", "rate", "rate_err", "status")
SUMMARY_COLUMNS = ("run", "camcol", "filter", "field", "source", "line", "status", "n_sec", "n_ok", "mean_rate", "mean_rate_err", "chi2",
                   "dof", "peak_section", "peak_rate", "length", "flux", "flux_err")
_INT_COLUMNS = ("run", "camcol", "field", "line", "section", "n_geom", "n_core", "n_sky", "status", "n_sec", "n_ok", "dof", "peak_section")


def as_params(params):
    """a dict of lfdmi_lc_params fields, checked as the library checks them (unknown names raise TypeError, values ValueError)"""
    p = dict(params or {})
    for k in p:
        if k not in PARAM_NAMES:
            raise TypeError(f"unknown light curve parameter {k!r}")
    if "sec_len" in p and not 8.0 <= float(p["sec_len"]) <= 4096.0:
        raise ValueError("sec_len: 8 .. 4096")
    if "clip" in p and not (math.isfinite(float(p["clip"])) and 0.0 < float(p["clip"]) <= 1024.0):
        raise ValueError("clip: finite, 0 < clip <= 1024")
    for k in ("min_core", "min_sky"):
        if k in p and (int(p[k]) != p[k] or int(p[k]) < 1):
            raise ValueError(f"{k}: an integer >= 1")
    return p


def segments(rows, bg_gap=4.0, bg_width=16.0):
    """(frame, x1, y1, x2, y2, half) rows -> SEGMENT_DTYPE records: bg_in = half + bg_gap, bg_out = min(bg_in + bg_width, 64)"""
    out = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, (f, x1, y1, x2, y2, half) in enumerate(rows):
        out[i]["frame"] = int(f)
        out[i]["x1"], out[i]["y1"], out[i]["x2"], out[i]["y2"], out[i]["half"] = float(x1), float(y1), float(x2), float(y2), float(half)
        out[i]["bg_in"] = float(half) + float(bg_gap)
        out[i]["bg_out"] = min(float(out[i]["bg_in"]) + float(bg_width), MAX_BG)
    return out


def segments_from_mask_segments(mask_segs, bg_gap=4.0, bg_width=16.0):
    """MASK_SEGMENT_DTYPE records (what every ``masks.segments_from_*`` builder returns) -> SEGMENT_DTYPE records on the same
    frames, end points and half-widths"""
    ms = np.asarray(mask_segs, _native.MASK_SEGMENT_DTYPE).reshape(-1)
    return segments([(s["frame"], s["x1"], s["y1"], s["x2"], s["y2"], s["half"]) for s in ms], bg_gap, bg_width)


def light_curves(ctx, frames, segs, **kw):
    """``Context.light_curves`` in one call: (LC_DTYPE records, SECTION_DTYPE records [n_seg, max_sections])."""
    return ctx.light_curves(frames, segs, **kw)


def magnitude(flux):
    """22.5 - 2.5 log10(flux) of a flux in nanomaggies; NaN where flux <= 0 or NaN"""
    f = np.asarray(flux, np.float64)
    out = np.full(f.shape, np.nan)
    pos = f > 0
    out[pos] = 22.5 - 2.5 * np.log10(f[pos])
    return out if out.ndim else float(out)


def variability(records):
    """chi2 / dof of LC_DTYPE records: about 1 for a constant trail, NaN without two OK sections"""
    rec = np.asarray(records, LC_DTYPE)
    dof = rec["dof"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(dof > 0, rec["chi2"] / dof, np.nan)


def format_rows(meta, source, line, rec, sections):
    """The lightcurves.txt rows of one segment: one per section that is not EMPTY (``rec``: its LC_DTYPE record, ``sections``:
    its SECTION_DTYPE row of ``Context.light_curves``, of which the first rec["n_sec"] count).  meta = (run, camcol, filter,
    field), source = ``detect`` or ``radon``, line = the record's place in its frame; floats with repr."""
    out = []
    for j, s in enumerate(sections[:int(rec["n_sec"])]):
        if int(s["status"]) == SEC_EMPTY:
            continue
        vals = [repr(float(s[k])) for k in ("t0", "t1")] + [str(int(s[k])) for k in ("n_geom", "n_core", "n_sky")]
        vals += [repr(float(s[k])) for k in ("bkg", "flux", "flux_err", "rate", "rate_err")]
        out.append(" ".join(str(v) for v in (*meta, source, int(line), j, *vals, int(s["status"]))))
    return out


def format_summary_row(meta, source, line, rec):
    """One lightcurve_summary.txt row: SUMMARY_COLUMNS"""
    vals = [int(rec["status"]), int(rec["n_sec"]), int(rec["n_ok"]), repr(float(rec["mean_rate"])), repr(float(rec["mean_rate_err"])),
            repr(float(rec["chi2"])), int(rec["dof"]), int(rec["peak_section"]), repr(float(rec["peak_rate"])), repr(float(rec["length"])),
            repr(float(rec["flux"])), repr(float(rec["flux_err"]))]
    return " ".join(str(v) for v in (*meta, source, int(line), *vals))


def _read(path, columns):
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            rows.append({k: v if k in ("filter", "source") else int(v) if k in _INT_COLUMNS else float(v) for k, v in zip(columns, parts)})
    return rows


def read_lightcurves(path):
    """lightcurves.txt (rows only, no header line) -> list of dicts keyed by LC_COLUMNS."""
    return _read(path, LC_COLUMNS)


def read_summary(path):
    """lightcurve_summary.txt -> list of dicts keyed by SUMMARY_COLUMNS."""
    return _read(path, SUMMARY_COLUMNS)
