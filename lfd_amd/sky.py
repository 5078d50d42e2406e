"""Sky normalisation: make a frame that still carries its sky look like the sky-subtracted nanomaggie frames the detector was
tuned on (include/lfdmi.h: sky normalisation).  ``_native.Sky`` is the device handle; this module holds the parameters, a
one-call helper and the sky.txt format of ``DetectTrails(normalize=True)``.
"""
import dataclasses

import numpy as np

from . import _native

SKY_DTYPE = _native.SKY_DTYPE
SUBTRACT, NORMALISE = _native.SKY_SUBTRACT, _native.SKY_NORMALISE
OK, NO_SKY, NO_NOISE = _native.SKY_OK, _native.SKY_NO_SKY, _native.SKY_NO_NOISE
SKY_COLUMNS = ("run", "camcol", "filter", "field", "status", "sky", "sigma", "gain", "n_empty")


@dataclasses.dataclass
class SkyParams:
    """lfdmi_sky_params with its defaults.  target_sigma = 0.025 is the sky sigma of ``synth.make_frame``, the recipe the
    detection thresholds and the benchmark are quoted on."""
    cell: int = 64
    k_clip: float = 3.0
    n_clip: int = 3
    filter: int = 3
    mode: int = NORMALISE
    target_sigma: float = 0.025

    def as_dict(self):
        return dataclasses.asdict(self)


def default_params():
    """lfdmi_default_sky_params as a SkyParams (read from the library: no GPU needed)."""
    p = _native.make_sky_params()
    return SkyParams(**{k: getattr(p, k) for k, _ in _native.SkyParamsStruct._fields_})


def as_params(params):
    """None / dict / SkyParams -> dict of lfdmi_sky_params fields"""
    if params is None:
        return {}
    if isinstance(params, SkyParams):
        return params.as_dict()
    return dict(params)


def normalize_frames(ctx, frames, meshes=False, **params):
    """Normalise (n, h, w) frames on ``ctx``: returns (float32 numpy frames, SKY_DTYPE records[, sky mesh, sigma mesh]).  For
    repeated calls keep a ``_native.Sky`` handle instead: this one is created and destroyed per call."""
    arr = frames if _native._is_dev(frames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Sky(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **params) as sky:
        out = np.empty((n, h, w), np.float32)
        res = sky.normalize(arr, out=out, meshes=meshes)
    out = out.reshape(shp)
    return (out, *res) if meshes else (out, res)


def format_row(meta, rec):
    """One sky.txt row: meta = (run, camcol, filter, field); floats with repr."""
    return " ".join(str(v) for v in (*meta, int(rec["status"]), repr(float(rec["sky"])), repr(float(rec["sigma"])),
                                      repr(float(rec["gain"])), int(rec["n_empty"])))


def read_sky(path):
    """sky.txt -> list of dicts keyed by SKY_COLUMNS (the header line is skipped)."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == SKY_COLUMNS[0]:
                continue
            r = {}
            for k, v in zip(SKY_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ("run", "camcol", "field", "status", "n_empty") else float(v)
            rows.append(r)
    return rows
