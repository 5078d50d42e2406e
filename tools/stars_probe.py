"""Device time of the source finder (lfdmi_find_stars) on device-resident frames, against a device-to-device copy of the same
frames from the same run and against the 4 H W byte floor.

    python tools/stars_probe.py [--frames 256] [--distinct 16] [--calls 20] [--shape 1489 2048]

Frames are ``synth.make_frame`` (400 stars per SDSS frame), ``--distinct`` of them repeated to ``--frames``.  A call is timed on
the host around the whole entry point (it waits for its stream twice), records left on the device.  Per-kernel times are not
measured here: that takes a rocprofv3 --kernel-trace --stats pass.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=2, default=(1489, 2048))
    a = ap.parse_args()
    import torch
    from lfd_amd import _native, synth
    h, w = a.shape
    base = np.stack([synth.make_frame(k, shape=(h, w))[0] for k in range(a.distinct)])
    dev = torch.from_numpy(base).cuda().repeat((a.frames + a.distinct - 1) // a.distinct, 1, 1)[:a.frames].contiguous()
    other = torch.empty_like(dev)
    nbytes = dev.numel() * 4
    with _native.Context(0, h, w, 8) as ctx:
        rec, frec = ctx.find_stars(dev, device_out=True)          # warm-up (and the pool's first allocations)
        torch.cuda.synchronize()
        t_find, t_copy, t_cat = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            rec, frec = ctx.find_stars(dev, device_out=True)
            t_find.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ctx.stars_catalog(rec, frec, 0.396, device=True)
            torch.cuda.synchronize()
            t_cat.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other.copy_(dev)
            torch.cuda.synchronize()
            t_copy.append((time.perf_counter() - t0) * 1e3)
    floor = nbytes / 8e12 * 1e3

    def line(name, t):
        return "%-28s median %8.3f ms  range %8.3f .. %8.3f ms" % (name, statistics.median(t), min(t), max(t))
    print("frames %d x %d x %d (%d distinct), %d calls; sources per frame: n_found %d .. %d, n_out %d .. %d"
          % (a.frames, h, w, a.distinct, a.calls, frec["n_found"].min(), frec["n_found"].max(), frec["n_out"].min(), frec["n_out"].max()))
    print(line("find_stars (whole call)", t_find))
    print(line("stars_catalog (whole call)", t_cat))
    print(line("device-to-device copy", t_copy))
    print("byte floor 4 H W at 8 TB/s     %8.3f ms (%.1f MB)" % (floor, nbytes / 1e6))
    print("find_stars / copy %.2f, find_stars / floor %.1f; per-kernel times: unmeasured (no kernel trace was taken)"
          % (statistics.median(t_find) / statistics.median(t_copy), statistics.median(t_find) / floor))


if __name__ == "__main__":
    main()
