"""Device time of the frame seeing (lfdmi_measure_seeing) on device-resident frames and device-resident finder records, against
the source finder on the same frames and a device-to-device copy of them, all from the same run.

    python tools/psf_probe.py [--frames 256] [--distinct 16] [--calls 20] [--shape 1489 2048] [--out profiles/psf_probe.txt]

Frames are ``synth.make_frame`` (400 stars per SDSS frame), ``--distinct`` of them repeated to ``--frames``.  A call is timed on
the host around the whole entry point (measure_seeing waits for its stream once, find_stars twice).  The figure to read is the
ratio to find_stars.  Per-kernel times are not measured here: that takes a rocprofv3 --kernel-trace --stats pass.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=2, default=(1489, 2048))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psf_probe.txt"))
    a = ap.parse_args()
    import torch
    from lfd_amd import _native, synth
    h, w = a.shape
    base = np.stack([synth.make_frame(k, shape=(h, w))[0] for k in range(a.distinct)])
    dev = torch.from_numpy(base).cuda().repeat((a.frames + a.distinct - 1) // a.distinct, 1, 1)[:a.frames].contiguous()
    other = torch.empty_like(dev)
    with _native.Context(0, h, w, 8) as ctx:
        rec, frec = ctx.find_stars(dev, device_out=True)          # warm-up (and the pool's first allocations)
        out, fr = ctx.measure_seeing(dev, rec, frec)
        torch.cuda.synchronize()
        t_find, t_psf, t_copy = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            rec, frec = ctx.find_stars(dev, device_out=True)
            t_find.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            out, fr = ctx.measure_seeing(dev, rec, frec)
            t_psf.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other.copy_(dev)
            torch.cuda.synchronize()
            t_copy.append((time.perf_counter() - t0) * 1e3)

    def line(name, t):
        return "%-30s median %8.3f ms  range %8.3f .. %8.3f ms" % (name, statistics.median(t), min(t), max(t))
    text = [
        "frames %d x %d x %d (%d distinct), %d calls; records per frame %d .. %d, candidates %d .. %d, OK %d .. %d, used %d .. %d"
        % (a.frames, h, w, a.distinct, a.calls, frec["n_out"].min(), frec["n_out"].max(), fr["n_cand"].min(), fr["n_cand"].max(),
           fr["n_ok"].min(), fr["n_ok"].max(), fr["n_used"].min(), fr["n_used"].max()),
        "fwhm_px %.4f .. %.4f, frames with too few stars: %d" % (np.nanmin(fr["fwhm_px"]), np.nanmax(fr["fwhm_px"]),
                                                                  int((fr["status"] != 0).sum())),
        line("measure_seeing (whole call)", t_psf),
        line("find_stars (whole call)", t_find),
        line("device-to-device copy", t_copy),
        "measure_seeing / find_stars %.3f, measure_seeing / copy %.2f; per-kernel times: unmeasured (no kernel trace was taken)"
        % (statistics.median(t_psf) / statistics.median(t_find), statistics.median(t_psf) / statistics.median(t_copy)),
    ]
    print("\n".join(text))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
