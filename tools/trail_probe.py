"""Cost of lfdmi_measure_trails: a 256-frame SDSS batch in which every frame has a trail, and a batch of 4096 x 4096 frames,
both device-resident (what DetectTrails' device path measures on; distinct frames tiled on the device).  Prints one JSON line: ms per batch (median of the timed
repetitions) and the frames measured.

    python tools/trail_probe.py [--reps 5] [--lsst 256] [--lsst-unique 16]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trail_frames(n_unique, shape, seed=0):
    from lfd_amd import synth
    rng = np.random.default_rng(seed)
    h, w = shape
    out = []
    for k in range(n_unique):
        img = rng.normal(0.0, 0.025, shape).astype(np.float32)
        ang = rng.uniform(5, 85) + (90 if k % 2 else 0)
        synth._add_streak(img, rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w, ang, 1.0 if k % 3 else 0.08, 2.0)
        out.append(img)
    return np.stack(out)


def time_batch(ctx, frames, recs, reps, repeat=1):
    """frames (n_unique) go to the device once and are tiled there `repeat` times (an LSST-size batch of 256 frames is 17 GB)"""
    import torch
    dev = torch.from_numpy(frames).to("cuda:0").repeat(repeat, 1, 1)
    recs = np.concatenate([recs] * repeat)
    ctx.measure_trails(dev, recs)          # first call: the workspace
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, prof = ctx.measure_trails(dev, recs)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), int((recs["found"] != 0).sum()), int((out["status"] == 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lsst", type=int, default=256)          # LSST-size frames in the batch (a multiple of --lsst-unique)
    ap.add_argument("--lsst-unique", type=int, default=16)
    a = ap.parse_args()
    import torch
    torch.cuda.init()                      # (the HIP runtime through torch first, as bench.py does)
    from lfd_amd import _native, synth
    from lfd_amd.detecttrails import default_params
    pb, pd, _ = default_params()
    res = {}
    base = trail_frames(32, synth.SDSS_SHAPE)
    with _native.Context(0, *synth.SDSS_SHAPE, 64) as ctx:
        rec = ctx.detect_batch(base.copy(), pb, pd)
        ms, found, ok = time_batch(ctx, base, rec, a.reps, repeat=8)
        res["sdss_256"] = {"frames": 256, "ms": round(ms, 3), "found": found, "measured_ok": ok}
    big = trail_frames(a.lsst_unique, synth.LSST_SHAPE, seed=1)
    with _native.Context(0, *synth.LSST_SHAPE, 16) as ctx:
        rec = ctx.detect_batch(big.copy(), pb, pd)
        ms, found, ok = time_batch(ctx, big, rec, a.reps, repeat=a.lsst // a.lsst_unique)
        res["lsst_%d" % a.lsst] = {"frames": a.lsst, "ms": round(ms, 3), "found": found, "measured_ok": ok}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
