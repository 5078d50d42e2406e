"""Source finder: the compact sources of a frame as a remove_stars catalogue, for frames that have no photoObj table
(include/lfdmi.h: source finder).  ``Context.find_stars`` and ``Context.stars_catalog`` are the device calls; this module holds
the parameters, a one-call helper, the catalogue of step 8 on the host and the stars.txt format of
``DetectTrails(find_stars=True)``.
"""
import dataclasses
import math

import numpy as np

from . import _native
from .catalogs import empty_packed

STAR_DTYPE = _native.STAR_DTYPE
FRAME_DTYPE = _native.STARS_FRAME_DTYPE
OK, TRUNCATED = _native.STARS_OK, _native.STARS_TRUNCATED
EXTENDED, EDGE = _native.STAR_EXTENDED, _native.STAR_EDGE
MAX_OBJ = _native.STARS_MAX_OBJ
STARS_COLUMNS = ("run", "camcol", "filter", "field", "status", "n_found", "n_out", "n_extended")


@dataclasses.dataclass
class StarsParams:
    """lfdmi_stars_params with its defaults; ``validate`` applies the library's rules without a device."""
    k_det: float = 5.0
    k_edge: float = 3.0
    edge_frac: float = 0.02
    sep: int = 3
    r_max: int = 32
    max_obj: int = 4096

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self):
        for name in ("sep", "r_max", "max_obj"):
            if int(getattr(self, name)) != getattr(self, name):
                raise ValueError(f"{name} must be an integer")
        for name in ("k_det", "k_edge"):
            if not (math.isfinite(getattr(self, name)) and getattr(self, name) > 0):
                raise ValueError(f"{name} must be positive")
        if not 0.0 <= self.edge_frac <= 1.0:
            raise ValueError("edge_frac must be 0 .. 1")
        if not 1 <= self.sep <= 8:
            raise ValueError("sep must be 1 .. 8")
        if not 1 <= self.r_max <= 32:
            raise ValueError("r_max must be 1 .. 32")
        if not 1 <= self.max_obj <= MAX_OBJ:
            raise ValueError("max_obj must be 1 .. %d" % MAX_OBJ)
        return self


def default_params():
    """lfdmi_default_stars_params as a StarsParams (read from the library: no GPU needed)."""
    p = _native.make_stars_params()
    return StarsParams(**{k: getattr(p, k) for k, _ in _native.StarsParamsStruct._fields_})


def as_params(params):
    """None / dict / StarsParams -> validated dict of lfdmi_stars_params fields"""
    if params is None:
        return {}
    if isinstance(params, StarsParams):
        return params.validate().as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(StarsParams)}
    if unknown:
        raise TypeError(f"unknown stars parameter {sorted(unknown)[0]!r}")
    StarsParams(**params).validate()
    return dict(params)


def find_stars(ctx, frames, sigma=None, **params):
    """``Context.find_stars`` with validated parameters: (STAR_DTYPE records [n, max_obj], FRAME_DTYPE records [n])."""
    return ctx.find_stars(frames, sigma=sigma, **as_params(params))


def to_catalog(records, frame_records, pixscale=0.396):
    """Step 8 on the host: records [n, max_obj] and frame records [n] -> the dict ``pack_catalogs`` returns.  The same values
    ``Context.stars_catalog`` computes on the device, the padding of ``empty_packed`` past ``count`` included."""
    frec = np.asarray(frame_records, FRAME_DTYPE).reshape(-1)
    rec = np.asarray(records, STAR_DTYPE).reshape(len(frec), -1)
    out = empty_packed(len(frec), rec.shape[1])
    for i, fr in enumerate(frec):
        k = int(fr["n_out"])
        r = rec[i, :k]
        out["count"][i] = k
        out["ROWC"][i, :k] = r["x"].astype(np.float32)[:, None]
        out["COLC"][i, :k] = r["y"].astype(np.float32)[:, None]
        out["PETROTH90"][i, :k] = (r["rad"].astype(np.float64) * float(pixscale)).astype(np.float32)[:, None]
        out["NOBSERVE"][i, :k] = np.where(r["flags"] & EXTENDED, 0, 1)
        out["NDETECT"][i, :k] = 1
    return out


def n_extended(records, frame_records):
    """extended candidates among each frame's reported records"""
    frec = np.asarray(frame_records, FRAME_DTYPE).reshape(-1)
    rec = np.asarray(records, STAR_DTYPE).reshape(len(frec), -1)
    return np.array([int(np.count_nonzero(rec[i, :int(fr["n_out"])]["flags"] & EXTENDED)) for i, fr in enumerate(frec)], np.int64)


def format_row(meta, frec, n_ext):
    """One stars.txt row: meta = (run, camcol, filter, field)."""
    return " ".join(str(v) for v in (*meta, int(frec["status"]), int(frec["n_found"]), int(frec["n_out"]), int(n_ext)))


def read_stars(path):
    """stars.txt -> list of dicts keyed by STARS_COLUMNS (a header line is skipped)."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == STARS_COLUMNS[0]:
                continue
            rows.append({k: (v if k == "filter" else int(v)) for k, v in zip(STARS_COLUMNS, parts)})
    return rows
