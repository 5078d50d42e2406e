"""Trail strips: the band around a segment straightened into a map of sections along the trail by offsets across it
(include/lfdmi.h: trail strips).  ``Context.trail_strips`` is the device call; this module holds the segments of the other units'
records (through ``masks.segments_from_*``, so the half-width rule stays in one place, widened by the wings), a one-call helper
that also makes the per-cell maps, the 8-bit preview and the row format of strips.txt.
"""
import math

import numpy as np

from . import _native

SEGMENT_DTYPE = _native.STRIP_SEGMENT_DTYPE
STRIP_DTYPE = _native.STRIP_DTYPE
SECTION_DTYPE = _native.STRIP_SECTION_DTYPE
CELL_DTYPE = _native.STRIP_CELL_DTYPE
OK, BAD_SEGMENT, TOO_LONG, EMPTY = _native.STRIP_OK, _native.STRIP_BAD_SEGMENT, _native.STRIP_TOO_LONG, _native.STRIP_EMPTY
SEC_OK, SEC_LOW, SEC_EMPTY = _native.STRIP_SEC_OK, _native.STRIP_SEC_LOW, _native.STRIP_SEC_EMPTY
MAX_SECTIONS, MAX_OFF = _native.STRIP_MAX_SECTIONS, _native.STRIP_MAX_OFF
PARAM_NAMES = tuple(k for k, _ in _native.StripParamsStruct._fields_ if k != "pad")
DEFAULT_WING = 6.0
STRIP_COLUMNS = ("run", "camcol", "filter", "field", "source", "line", "section", "t0", "t1", "n_core", "n_wing", "bkg", "rate",
                 "rate_err", "centre", "width", "status")
_INT_COLUMNS = ("run", "camcol", "field", "line", "section", "n_core", "n_wing", "status")


def as_params(params):
    """a dict of lfdmi_strip_params fields, checked as the library checks them (unknown names raise TypeError, values ValueError)"""
    p = dict(params or {})
    for k in p:
        if k not in PARAM_NAMES:
            raise TypeError(f"unknown strip parameter {k!r}")
    if "sec_len" in p and not 4.0 <= float(p["sec_len"]) <= 4096.0:
        raise ValueError("sec_len: 4 .. 4096")
    if "step" in p and not 0.5 <= float(p["step"]) <= 8.0:
        raise ValueError("step: 0.5 .. 8")
    if "wing" in p and not (math.isfinite(float(p["wing"])) and float(p["wing"]) > 0.0):
        raise ValueError("wing: finite, > 0")
    if "k_mom" in p and not (math.isfinite(float(p["k_mom"])) and float(p["k_mom"]) >= 0.0):
        raise ValueError("k_mom: finite, >= 0")
    if "clip" in p and not (math.isfinite(float(p["clip"])) and 0.0 < float(p["clip"]) <= 1024.0):
        raise ValueError("clip: finite, 0 < clip <= 1024")
    for k in ("min_core", "min_wing"):
        if k in p and (int(p[k]) != p[k] or int(p[k]) < 1):
            raise ValueError(f"{k}: an integer >= 1")
    return p


def segments(rows):
    """(frame, x1, y1, x2, y2, half) rows -> SEGMENT_DTYPE records"""
    out = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, (f, x1, y1, x2, y2, half) in enumerate(rows):
        out[i]["frame"] = int(f)
        out[i]["x1"], out[i]["y1"], out[i]["x2"], out[i]["y2"], out[i]["half"] = float(x1), float(y1), float(x2), float(y2), float(half)
    return out


def segments_from_mask_segments(mask_segs, margin=None):
    """MASK_SEGMENT_DTYPE records (what every ``masks.segments_from_*`` builder returns) -> SEGMENT_DTYPE records on the same
    frames and end points, each half-width widened by ``margin`` (default: the default ``wing``, 6 px) so that the wings are sky"""
    m = DEFAULT_WING if margin is None else float(margin)
    ms = np.asarray(mask_segs, _native.MASK_SEGMENT_DTYPE).reshape(-1)
    return segments([(s["frame"], s["x1"], s["y1"], s["x2"], s["y2"], float(s["half"]) + m) for s in ms])


def mean_map(cells):
    """CELL_DTYPE records -> float32 (float)(q * 2^-30 / n), NaN where n == 0"""
    n, q = cells["n"], cells["q"]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = q.astype(np.float64) * np.float64(2.0 ** -30) / n.astype(np.float64)
    return np.where(n > 0, m, np.nan).astype(np.float32)


def maps(rec, cells):
    """one segment's STRIP_DTYPE record and its row of cells -> {"mean" (float32), "n", "n_geom" (int32)}, each (n_sec, n_off);
    (0, 0) arrays for a segment that was not measured"""
    ok = int(rec["status"]) in (OK, EMPTY)
    ns, no = (int(rec["n_sec"]), int(rec["n_off"])) if ok else (0, 0)
    c = cells[:ns * no].reshape(ns, no)
    return {"mean": mean_map(c), "n": c["n"].copy(), "n_geom": c["n_geom"].copy()}


def trail_strips(ctx, frames, segs, **kw):
    """``Context.trail_strips`` in one call: (STRIP_DTYPE records, SECTION_DTYPE records [n_seg, max_sections], and per segment
    the ``maps`` dictionary of (n_sec, n_off) arrays ``mean``, ``n`` and ``n_geom``)."""
    rec, sec, cells = ctx.trail_strips(frames, segs, **kw)
    return rec, sec, [maps(rec[i], cells[i]) for i in range(len(rec))]


def to_uint8(mean, lo_pct=1.0, hi_pct=99.5):
    """a linear stretch of a map between the ``lo_pct`` and ``hi_pct`` percentiles of its finite cells onto 0 .. 255 (rounded,
    clipped); a NaN cell is 0; a map without a finite cell, or whose two percentiles coincide, is 0 everywhere"""
    m = np.asarray(mean, np.float64)
    out = np.zeros(m.shape, np.uint8)
    fin = np.isfinite(m)
    if not fin.any():
        return out
    lo, hi = np.percentile(m[fin], [float(lo_pct), float(hi_pct)])
    if not hi > lo:
        return out
    out[fin] = np.rint(np.clip((m[fin] - lo) / (hi - lo), 0.0, 1.0) * 255.0).astype(np.uint8)
    return out


def write_png(path, mean, lo_pct=1.0, hi_pct=99.5):
    """the preview of a map: offsets down (positive u at the top), sections across"""
    from .detecttrails.debugio import write_png as _write
    img = to_uint8(mean, lo_pct, hi_pct)
    _write(path, np.ascontiguousarray(img.T[::-1]) if img.size else np.zeros((1, 1), np.uint8))


def format_rows(meta, source, line, rec, sections):
    """The strips.txt rows of one segment: one per section that is not EMPTY (``rec``: its STRIP_DTYPE record, ``sections``: its
    SECTION_DTYPE row, of which the first rec["n_sec"] count).  meta = (run, camcol, filter, field), source = ``detect`` or
    ``radon``, line = the record's place in its frame; floats with repr."""
    out = []
    for j, s in enumerate(sections[:int(rec["n_sec"])]):
        if int(s["status"]) == SEC_EMPTY:
            continue
        vals = [repr(float(s[k])) for k in ("t0", "t1")] + [str(int(s[k])) for k in ("n_core", "n_wing")]
        vals += [repr(float(s[k])) for k in ("bkg", "rate", "rate_err", "centre", "width")]
        out.append(" ".join(str(v) for v in (*meta, source, int(line), j, *vals, int(s["status"]))))
    return out


def read_strips(path):
    """strips.txt (rows only, no header line) -> list of dicts keyed by STRIP_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            rows.append({k: v if k in ("filter", "source") else int(v) if k in _INT_COLUMNS else float(v)
                         for k, v in zip(STRIP_COLUMNS, parts)})
    return rows
