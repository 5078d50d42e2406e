"""Device time of the frame previews (lfdmi_frame_previews) on device-resident frames, images left on the device, against a
device-to-device copy of the same frames in the same run.

    python tools/preview_probe.py [--frames 256] [--distinct 16] [--calls 20] [--shape 1489 2048] [--bin 4] [--out profiles/preview_probe.txt]

Frames are ``synth.make_frame``, ``--distinct`` of them repeated to ``--frames``.  A call is timed on the host around the whole
entry point, which waits for its stream once at its end; RANK mode at the default ranks.  The figures to read are the ratio to the
copy (which moves 8 H W bytes a frame: 4 in, 4 out) and to the floor of 4 H W bytes a frame the binning kernel must read, at the
copy's own measured rate.  Per-kernel times, and so what bounds the selection, are not measured here: that takes a
rocprofv3 --kernel-trace --stats pass.
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
    ap.add_argument("--bin", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preview_probe.txt"))
    a = ap.parse_args()
    import torch
    from lfd_amd import _native, synth
    h, w = a.shape
    base = np.stack([synth.make_frame(k, shape=(h, w))[0] for k in range(a.distinct)])
    dev = torch.from_numpy(base).cuda().repeat((a.frames + a.distinct - 1) // a.distinct, 1, 1)[:a.frames].contiguous()
    other = torch.empty_like(dev)
    with _native.Context(0, h, w, 8) as ctx:
        out, rec = ctx.frame_previews(dev, bin=a.bin, out_device=True)          # warm-up (and the pool's first allocations)
        torch.cuda.synchronize()
        t_prev, t_copy = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            out, rec = ctx.frame_previews(dev, bin=a.bin, out_device=True)
            t_prev.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other.copy_(dev)
            torch.cuda.synchronize()
            t_copy.append((time.perf_counter() - t0) * 1e3)
        chunks = ctx.debug_unit_split()["chunks"]

    def line(name, t):
        return "%-30s median %8.3f ms  range %8.3f .. %8.3f ms" % (name, statistics.median(t), min(t), max(t))
    mp, mc = statistics.median(t_prev), statistics.median(t_copy)
    gb = a.frames * h * w * 4 / 1e9
    text = [
        "frames %d x %d x %d (%d distinct), bin %d, RANK mode, images left on the device, %d calls; statuses OK %d, FLAT %d, EMPTY %d"
        % (a.frames, h, w, a.distinct, a.bin, a.calls, int((rec["status"] == 0).sum()), int((rec["status"] == 1).sum()),
           int((rec["status"] == 2).sum())),
        "cells per frame %d, lo %.5f .. %.5f, hi %.5f .. %.5f; chunks of the last call (0: not recorded) %d"
        % (int(rec["n_cells"][0] + rec["n_empty"][0]), rec["lo_f"].min(), rec["lo_f"].max(), rec["hi_f"].min(), rec["hi_f"].max(), chunks),
        line("frame_previews (whole call)", t_prev),
        line("device-to-device copy", t_copy),
        "frame_previews / copy %.2f; the copy moves %.2f GB at %.0f GB/s, so reading the frames once (%.2f GB, the 4 H W floor) "
        "would take %.3f ms at that rate: frame_previews / floor %.2f"
        % (mp / mc, 2 * gb, 2 * gb / (mc * 1e-3), gb, mc / 2, mp / (mc / 2)),
        "per-kernel times (binning, limits, render) and what bounds the selection: unmeasured (no kernel trace was taken)",
    ]
    print("\n".join(text))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
