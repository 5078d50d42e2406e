"""Stacked cross-sections: width, flux and a profile row for trails too faint for ``measure_trails`` -- the frame summed along a
given segment, separately for every perpendicular offset (include/lfdmi.h: stacked cross-sections).  ``Context.stack_profiles``
is the device call; this module holds the parameters, the segments of the faint-trail search's lines or of results rows, a
one-call helper, the mapping onto trail records for the defocus fit and the radon_profiles.txt format of
``DetectTrails(radon_profiles=True)``.
"""
import dataclasses
import math

import numpy as np

from . import _native

STACK_DTYPE = _native.STACK_DTYPE
SEGMENT_DTYPE = _native.STACK_SEGMENT_DTYPE
OK, BAD_SEGMENT, TOO_SHORT, TOO_FAINT = _native.STACK_OK, _native.STACK_BAD_SEGMENT, _native.STACK_TOO_SHORT, _native.STACK_TOO_FAINT
MAX_HALF = _native.STACK_MAX_HALF
PROFILE_COLUMNS = ("run", "camcol", "filter", "field", "line", "status", "x1", "y1", "x2", "y2", "n_col", "background", "noise",
                   "peak", "fwhm", "fwhm_arcsec", "depth", "flux", "flux_err", "snr")


@dataclasses.dataclass
class StackParams:
    """lfdmi_stack_params with its defaults; ``validate`` applies the library's rules without a device."""
    wing: int = 8
    n_iter: int = 2
    min_cols: int = 64
    clip: float = 0.125
    prof_half: float = 24.0
    step: float = 0.5
    box: float = 4.0
    max_shift: float = 8.0
    k_sig: float = 6.0
    k_ref: float = 4.0
    pixscale: float = 0.396

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self):
        for name in ("wing", "n_iter", "min_cols"):
            if int(getattr(self, name)) != getattr(self, name):
                raise ValueError(f"{name} must be an integer")
        if not (math.isfinite(self.step) and self.step > 0 and math.isfinite(self.prof_half) and self.prof_half > 0):
            raise ValueError("step and prof_half must be positive")
        kk = self.prof_half / self.step
        K = int(math.floor(kk + 0.5))
        if K < 1 or K > 512 or abs(kk - K) > 1e-9 * kk:
            raise ValueError("prof_half / step must be an integer, 1 .. 512")
        if not self.prof_half + self.step / 2.0 <= MAX_HALF:
            raise ValueError("prof_half + step / 2 must be at most %g" % MAX_HALF)
        if self.wing < 1 or not self.wing < self.prof_half:
            raise ValueError("wing must be 1 .. below prof_half")
        if not 0 <= self.n_iter <= 16:
            raise ValueError("n_iter must be 0 .. 16")
        if self.min_cols < 2:
            raise ValueError("min_cols must be >= 2")
        if math.isnan(self.clip) or not self.clip > 0:
            raise ValueError("clip must be positive (inf: no clipping)")
        for name in ("box", "max_shift"):
            if not (math.isfinite(getattr(self, name)) and getattr(self, name) >= 0):
                raise ValueError(f"{name} must be >= 0")
        if math.isnan(self.k_sig) or math.isnan(self.k_ref) or not math.isfinite(self.pixscale):
            raise ValueError("k_sig, k_ref and pixscale must be numbers")
        return self


def default_params():
    """lfdmi_default_stack_params as a StackParams (read from the library: no GPU needed)."""
    p = _native.make_stack_params()
    return StackParams(**{k: getattr(p, k) for k, _ in _native.StackParamsStruct._fields_})


def as_params(params):
    """None / dict / StackParams -> validated dict of lfdmi_stack_params fields"""
    if params is None:
        return {}
    if isinstance(params, StackParams):
        return params.validate().as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(StackParams)}
    if unknown:
        raise TypeError(f"unknown stack parameter {sorted(unknown)[0]!r}")
    StackParams(**params).validate()
    return dict(params)


def segments(rows):
    """(frame, x1, y1, x2, y2) rows -> SEGMENT_DTYPE records"""
    out = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, (f, x1, y1, x2, y2) in enumerate(rows):
        out[i] = (int(f), 0, float(x1), float(y1), float(x2), float(y2))
    return out


def segments_from_radon_lines(lines, n_lines):
    """The found lines of ``Radon.search_lines`` (records [n, K], n_lines [n]) -> (SEGMENT_DTYPE records, (frame, line) of each):
    every found line's segment ex1 .. ey2, frames ascending, peel order within a frame."""
    lines = np.asarray(lines)
    if lines.ndim == 1:
        lines = lines[None]
    rows, where = [], []
    for i, nl in enumerate(np.asarray(n_lines).reshape(-1)):
        for k in range(int(nl)):
            r = lines[i, k]
            rows.append((i, r["ex1"], r["ey1"], r["ex2"], r["ey2"]))
            where.append((i, k))
    return segments(rows), where


def segments_from_radon_wide(lines, n_lines):
    """The found bands of ``Radon.search_wide`` (records [n, K], n_lines [n]) -> (SEGMENT_DTYPE records, (frame, line) of each):
    the records carry ``segments_from_radon_lines``' fields, and ex1 .. ey2 lie on the band's centre line."""
    return segments_from_radon_lines(lines, n_lines)


def segments_from_results(records):
    """Detection records (RESULT_DTYPE, one per frame) -> (SEGMENT_DTYPE records, frame of each): the x1 .. y2 of a results row for
    every frame with found != 0."""
    rec = np.asarray(records).reshape(-1)
    rows = [(i, r["x1"], r["y1"], r["x2"], r["y2"]) for i, r in enumerate(rec) if int(r["found"]) and not int(r["status"])]
    return segments(rows), [r[0] for r in rows]


def stack_profiles(ctx, frames, segs, sigma=None, raw=False, **params):
    """``Context.stack_profiles`` with validated parameters: (STACK_DTYPE records, float32 rows [n_seg, 2K+1])."""
    return ctx.stack_profiles(frames, segs, sigma=sigma, raw=raw, **as_params(params))


_TRAIL_STATUS = {OK: _native.TRAIL_OK, BAD_SEGMENT: _native.TRAIL_NOT_FOUND, TOO_SHORT: _native.TRAIL_TOO_SHORT,
                 TOO_FAINT: _native.TRAIL_TOO_FAINT}


def to_trails(records):
    """STACK_DTYPE records -> TRAIL_DTYPE records, so that ``Context.fit_defocus`` runs on the rows unchanged with a bank built
    for the same prof_half / prof_step (= step) / wing: n_pos = n_col, n_seg = 2 (the halves)."""
    rec = np.asarray(records, STACK_DTYPE).reshape(-1)
    out = np.zeros(len(rec), _native.TRAIL_DTYPE)
    out["status"] = [_TRAIL_STATUS[int(s)] for s in rec["status"]]
    out["n_pos"], out["n_seg"], out["min_valid"] = rec["n_col"], 2, rec["min_valid"]
    for k in ("rho", "theta", "x1", "y1", "x2", "y2", "background", "noise", "peak", "fwhm", "fwhm_arcsec", "depth"):
        out[k] = rec[k]
    return out


def format_row(meta, line, rec):
    """One radon_profiles.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with
    repr."""
    vals = [repr(float(rec[k])) for k in ("x1", "y1", "x2", "y2")] + [int(rec["n_col"])]
    vals += [repr(float(rec[k])) for k in PROFILE_COLUMNS[11:]]
    return " ".join(str(v) for v in (*meta, int(line), int(rec["status"]), *vals))


def read_profiles(path):
    """radon_profiles.txt (rows only, no header line) -> list of dicts keyed by PROFILE_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(PROFILE_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ("run", "camcol", "field", "line", "status", "n_col") else float(v)
            rows.append(r)
    return rows
