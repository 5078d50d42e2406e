"""Trail subtraction: a smooth, star-robust model of a trail made from its own strip and taken out of the frame
(include/lfdmi.h: trail subtraction).  ``Context.subtract_trails`` is the device call; this module holds the parameter check, the
segments of the other units' records (through ``masks.segments_from_*``, widened by the wings as the strips' builder widens
them), a one-call helper, the per-segment model maps and the row format of subtracted.txt.
"""
import math

import numpy as np

from . import _native, strips

SEGMENT_DTYPE = _native.STRIP_SEGMENT_DTYPE
SUB_DTYPE = _native.SUB_DTYPE
OK, BAD_SEGMENT, TOO_LONG, EMPTY = _native.SUB_OK, _native.SUB_BAD_SEGMENT, _native.SUB_TOO_LONG, _native.SUB_EMPTY
MAX_SMOOTH = _native.SUB_MAX_SMOOTH
PARAM_NAMES = tuple(k for k, _ in _native.SubParamsStruct._fields_)
DEFAULT_WING = strips.DEFAULT_WING
SUB_COLUMNS = ("run", "camcol", "filter", "field", "source", "line", "status", "n_sec", "n_usable", "n_model", "n_pix", "removed", "peak",
               "peak_section")
_INT_COLUMNS = ("run", "camcol", "field", "line", "status", "n_sec", "n_usable", "n_model", "n_pix", "peak_section")
segments = strips.segments


def as_params(params):
    """a dict of lfdmi_sub_params fields, checked as the library checks them (unknown names raise TypeError, values ValueError)"""
    p = dict(params or {})
    for k in p:
        if k not in PARAM_NAMES:
            raise TypeError(f"unknown subtraction parameter {k!r}")
    if "sec_len" in p and not 4.0 <= float(p["sec_len"]) <= 4096.0:
        raise ValueError("sec_len: 4 .. 4096")
    if "step" in p and not 0.5 <= float(p["step"]) <= 8.0:
        raise ValueError("step: 0.5 .. 8")
    if "wing" in p and not (math.isfinite(float(p["wing"])) and float(p["wing"]) > 0.0):
        raise ValueError("wing: finite, > 0")
    if "clip" in p and not (math.isfinite(float(p["clip"])) and 0.0 < float(p["clip"]) <= 1024.0):
        raise ValueError("clip: finite, 0 < clip <= 1024")
    for k in ("smooth", "min_sec", "min_n", "min_wing", "apply"):
        if k in p and int(p[k]) != p[k]:
            raise ValueError(f"{k}: an integer")
    if "smooth" in p and not 0 <= int(p["smooth"]) <= MAX_SMOOTH:
        raise ValueError(f"smooth: 0 .. {MAX_SMOOTH}")
    if not 1 <= int(p.get("min_sec", 3)) <= 2 * int(p.get("smooth", 2)) + 1:   # (the defaults where a name is missing)
        raise ValueError("min_sec: 1 .. 2 * smooth + 1")
    for k in ("min_n", "min_wing"):
        if k in p and int(p[k]) < 1:
            raise ValueError(f"{k}: an integer >= 1")
    if "apply" in p and int(p["apply"]) not in (0, 1):
        raise ValueError("apply: 0 or 1")
    return p


def segments_from_mask_segments(mask_segs, margin=None):
    """MASK_SEGMENT_DTYPE records (what every ``masks.segments_from_*`` builder returns) -> SEGMENT_DTYPE records on the same
    frames and end points, each half-width widened by ``margin`` (default: the default ``wing``, 6 px) so that the wings are
    sky: ``strips.segments_from_mask_segments``' rule"""
    return strips.segments_from_mask_segments(mask_segs, margin)


def subtract_trails(ctx, frames, segs, **kw):
    """``Context.subtract_trails`` in one call, with the tables: (SUB_DTYPE records, and per segment the (n_sec, n_off) float32
    model map of ``model_maps``).  ``frames`` are changed in place unless ``apply=0``."""
    rec, model = ctx.subtract_trails(frames, segs, want_model=True, **kw)
    return rec, [model_maps(rec[i], model[i]) for i in range(len(rec))]


def model_maps(rec, model):
    """one segment's SUB_DTYPE record and its row of the tables -> the float32 (n_sec, n_off) model; a (0, 0) array for a segment
    that was not measured"""
    ok = int(rec["status"]) in (OK, EMPTY)
    ns, no = (int(rec["n_sec"]), int(rec["n_off"])) if ok else (0, 0)
    return np.asarray(model[:ns * no], np.float32).reshape(ns, no).copy()


def format_rows(meta, source, line, rec):
    """The subtracted.txt row of one segment, as a one-element list.  meta = (run, camcol, filter, field), source = ``detect``
    or ``radon``, line = the record's place in its frame; floats with repr."""
    vals = [int(rec[k]) for k in ("status", "n_sec", "n_usable", "n_model", "n_pix")]
    vals += [repr(float(rec["removed"])), repr(float(rec["peak"])), int(rec["peak_section"])]
    return [" ".join(str(v) for v in (*meta, source, int(line), *vals))]


def read_subtracted(path):
    """subtracted.txt (rows only, no header line) -> list of dicts keyed by SUB_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            rows.append({k: v if k in ("filter", "source") else int(v) if k in _INT_COLUMNS else float(v)
                         for k, v in zip(SUB_COLUMNS, parts)})
    return rows
