"""Short streaks: the oriented segment sums of include/lfdmi.h (short-streak search) on frames, and what follows a found streak.

``search_frames`` runs lfdmi_streak_search; ``segments`` turns its found records into ``masks.SEGMENT_DTYPE``, which the masks,
light curves, strips, stacked cross-sections and the subtraction take.  tests/streak_ref.py restates the search in numpy."""
import math

import numpy as np

from . import _native

STREAK_DTYPE = _native.STREAK_DTYPE
OK, NONE = _native.STREAK_OK, _native.STREAK_NONE
MAX_STREAKS = _native.STREAK_MAX_STREAKS
MAX_CELLS = 4096                     # Hb and Wb at most
PARAM_NAMES = ("bin", "length", "max_streaks", "peel_halfwidth", "clip", "threshold")
STREAK_COLUMNS = ("run", "camcol", "filter", "field", "streak", "q", "s", "r0", "c0", "n_pix", "snr", "x1", "y1", "x2", "y2")
_INT_COLUMNS = ("run", "camcol", "field", "streak", "q", "s", "r0", "c0", "n_pix")


def default_params():
    """lfdmi_default_streak_params as a dict"""
    p = _native.make_streak_params()
    return {k: getattr(p, k) for k in PARAM_NAMES}


def in_range(clip, b, length):
    """step 2's range rule: llrint(clip * 2^20) * b * b * L < 2^31 with the float32 clip"""
    top = float(np.float32(clip)) * 1048576.0
    return top < 2.0 ** 31 and int(np.rint(top)) * b * b * length < 2 ** 31


def as_params(params):
    """None, True or a dict of lfdmi_streak_params fields -> a checked dict of the given fields (unknown names: TypeError, values
    the library refuses: ValueError)"""
    if params is None or params is True:
        return {}
    p = dict(params)
    for k in p:
        if k not in PARAM_NAMES:
            raise TypeError(f"unknown streak parameter {k!r}")
    full = default_params()                                          # (the library's: one place holds them)
    full.update(p)
    for k in ("bin", "length", "max_streaks", "peel_halfwidth"):
        if int(full[k]) != full[k]:
            raise ValueError(f"streak parameter {k} must be an integer")
    if full["bin"] not in (1, 2, 4):
        raise ValueError("streak bin must be 1, 2 or 4")
    if full["length"] not in (8, 16, 32, 64):
        raise ValueError("streak length must be 8, 16, 32 or 64")
    if not 1 <= full["max_streaks"] <= MAX_STREAKS:
        raise ValueError(f"streak max_streaks must be 1 .. {MAX_STREAKS}")
    if not 0 <= full["peel_halfwidth"] <= 65536:
        raise ValueError("streak peel_halfwidth must be 0 .. 65536")
    for k in ("clip", "threshold"):
        if not (math.isfinite(full[k]) and full[k] > 0):
            raise ValueError(f"streak {k} must be finite and positive")
    if not in_range(full["clip"], int(full["bin"]), int(full["length"])):
        raise ValueError("streak clip * bin * bin * length does not fit the int32 sums")
    return p


def tile():
    """(rows, columns) of anchors a workgroup of k_streak_search owns"""
    return _native.streak_tile()


def search_frames(ctx, frames, sigma=None, pinned=False, native_device=False, **params):
    """``Context.streak_search``: (STREAK_DTYPE records [n, max_streaks], int32 n_streaks [n])."""
    return ctx.streak_search(frames, sigma=sigma, pinned=pinned, native_device=native_device, **as_params(params))


def found(records, n_streaks):
    """[(frame, streak, record)] of every found streak: frames ascending, peel order within a frame"""
    rec = np.asarray(records)
    if rec.ndim == 1:
        rec = rec[None]
    ns = np.asarray(n_streaks).reshape(-1)
    return [(f, k, rec[f, k]) for f in range(rec.shape[0]) for k in range(int(ns[f]))]


def segments(records, n_streaks, half=None, bits=1, cap=0.0, fill=0.0):
    """The found streaks of ``search_frames`` -> ``masks.SEGMENT_DTYPE`` records with the end points x1 .. y2, frames ascending,
    peel order within a frame.  half: the band's half-width in px; None: ``masks.half_width(None)``'s default."""
    from . import masks
    if half is None:
        half = masks.half_width(float("nan"))
    rows = [(f, r["x1"], r["y1"], r["x2"], r["y2"], half) for f, _, r in found(records, n_streaks)]
    return masks.segments(rows, bits=bits, cap=cap, fill=fill)


def format_row(meta, streak, rec):
    """One streaks.txt row: meta = (run, camcol, filter, field), streak = the record's place in its frame; floats with repr."""
    ints = [int(rec[k]) for k in ("q", "s", "r0", "c0", "n_pix")]
    vals = [repr(float(rec[k])) for k in ("snr", "x1", "y1", "x2", "y2")]
    return " ".join(str(v) for v in (*meta, int(streak), *ints, *vals))


def read_streaks(path):
    """streaks.txt (rows only, no header line) -> list of dicts keyed by STREAK_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            row = {}
            for k, v in zip(STREAK_COLUMNS, parts):
                row[k] = int(v) if k in _INT_COLUMNS else (v if k == "filter" else float(v))
            rows.append(row)
    return rows
