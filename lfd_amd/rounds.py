"""Detection rounds: several trails per frame from the bright and dim detector (include/lfdmi.h: detection rounds).
``Context.detect_rounds`` is the device call; this module holds its parameters, a one-call helper, the segments of the found
trails for the measurement units and the trails.txt row format.
"""
import numpy as np

from . import _native, masks

MAX_TRAILS = _native.ROUNDS_MAX_TRAILS
TRAIL_COLUMNS = ("run", "camcol", "filter", "field", "round", "found", "rho", "theta", "x1", "y1", "x2", "y2", "dup_of")
_FIELDS = ("max_trails", "half", "dup_dist")


class RoundsParams(dict):
    """the fields of lfdmi_rounds_params that differ from the library's defaults"""


def default_params():
    """the library's defaults as a dict: max_trails 4, half 10.0, dup_dist 20.0"""
    p = _native.make_rounds_params()
    return RoundsParams((k, getattr(p, k)) for k in _FIELDS)


def as_params(params=None, **kw):
    """None, a dict or keywords -> RoundsParams (unknown names raise)"""
    out = RoundsParams(params or {})
    out.update(kw)
    unknown = set(out) - set(_FIELDS)
    if unknown:
        raise TypeError(f"unknown rounds parameter {sorted(unknown)[0]!r}")
    return out


def detect_rounds(ctx, frames, params_bright, params_dim, catalogs=None, rs=None, pinned=False, params=None, **kw):
    """``Context.detect_rounds`` in one call: (records [n, max_trails], n_found [n], dup_of [n, max_trails])."""
    return ctx.detect_rounds(frames, params_bright, params_dim, catalogs, rs, pinned=pinned, **as_params(params, **kw))


def found_rows(records, n_found, dup_of=None, skip_dups=False):
    """[(frame, round)] of every found trail, frames ascending, rounds ascending; skip_dups: without those dup_of labels"""
    rows = []
    for i, nf in enumerate(np.asarray(n_found).reshape(-1)):
        for k in range(int(nf)):
            if skip_dups and dup_of is not None and int(dup_of[i][k]) >= 0:
                continue
            rows.append((i, k))
    return rows


def segments(records, n_found, dup_of=None, skip_dups=False, fwhm=None, bits=1, cap=0.0, fill=0.0, **half_kw):
    """The found trails -> (masks.SEGMENT_DTYPE records, (frame, round) of each), so that masks, light curves, strips and
    subtraction take the extra trails unchanged: x1 .. y2 of every found record, half-width by ``masks.half_width`` and its
    keywords.  fwhm: None, or one value per returned segment in the returned order, which ``found_rows`` with the same
    arguments gives in advance."""
    records = np.asarray(records)
    where = found_rows(records, n_found, dup_of, skip_dups)
    rows = []
    for j, (i, k) in enumerate(where):
        r = records[i][k]
        fw = float("nan") if fwhm is None else fwhm[j]
        rows.append((i, r["x1"], r["y1"], r["x2"], r["y2"], masks.half_width(fw, **half_kw)))
    return masks.segments(rows, bits, cap, fill), where


def format_row(meta, k, rec, dup):
    """One trails.txt row: meta = (run, camcol, filter, field), k = the round; floats with repr."""
    return " ".join(str(v) for v in (*meta, int(k), int(rec["found"]), repr(float(rec["rho"])), repr(float(rec["theta"])),
                                     int(rec["x1"]), int(rec["y1"]), int(rec["x2"]), int(rec["y2"]), int(dup)))


def read_trails(path):
    """trails.txt (rows only, no header line) -> list of dicts keyed by TRAIL_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(TRAIL_COLUMNS, parts):
                r[k] = v if k == "filter" else float(v) if k in ("rho", "theta") else int(v)
            rows.append(r)
    return rows
