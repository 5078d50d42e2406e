"""Device time of the short-streak search (lfdmi_streak_search) on device-resident noise frames at the defaults, against the
faint-trail search (``Radon.search``) and a device-to-device copy of the same frames in the same run, and the largest noise
peak over the full frames beside the 372 x 512 crops' ceiling the default threshold rests on.

    python tools/streak_probe.py [--frames 256] [--calls 20] [--shape 1489 2048] [--out profiles/streak_probe.txt]

A call is timed on the host around the whole entry point (it waits for its stream once per round; noise frames stop after round
0).  The three timings alternate inside one loop, so they see the same clocks.  There is no earlier code that does this job and
no speed gate: the ratios are recorded.  What bounds k_streak_search (LDS reads, integer adds or the score) is not measured
here: that takes a rocprofv3 --kernel-trace --stats pass and counters in a run of their own.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CROP_CEILING = 5.41          # the largest noise-only peak of the sixteen 372 x 512 crops (include/lfdmi.h: short-streak search, step 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=2, default=(1489, 2048))
    ap.add_argument("--radon-frames", type=int, default=32, help="max_frames of the faint-trail handle (it searches in chunks of them)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "streak_probe.txt"))
    a = ap.parse_args()
    import torch
    from lfd_amd import _native, streaks
    h, w = a.shape
    gen = torch.Generator(device="cuda").manual_seed(20)
    dev = torch.empty((a.frames, h, w), dtype=torch.float32, device="cuda").normal_(0.0, 0.025, generator=gen)
    other = torch.empty_like(dev)
    torch.cuda.synchronize()                                       # the fill ran on torch's stream, the calls run on the context's
    nbytes = dev.numel() * 4
    with _native.Context(0, h, w, 8) as ctx, _native.Radon(ctx, (h, w), max_frames=a.radon_frames) as radon:
        rec, ns = streaks.search_frames(ctx, dev)                  # warm-up (and the pool's first allocations)
        radon.search(dev)
        torch.cuda.synchronize()
        t_streak, t_radon, t_copy = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            rec, ns = streaks.search_frames(ctx, dev)
            t_streak.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            radon.search(dev)
            t_radon.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other.copy_(dev)
            torch.cuda.synchronize()
            t_copy.append((time.perf_counter() - t0) * 1e3)

    def line(name, t):
        return "%-32s median %9.3f ms  range %9.3f .. %9.3f ms" % (name, statistics.median(t), min(t), max(t))
    peak = float(rec["snr"][:, 0].max())
    ms, mr, mc = statistics.median(t_streak), statistics.median(t_radon), statistics.median(t_copy)
    out = ["frames %d x %d x %d of sigma-0.025 noise on the device, %d calls, defaults (bin 2, L 32, threshold 8)" % (a.frames, h, w, a.calls),
           line("streak_search (whole call)", t_streak),
           line("Radon.search (whole call)", t_radon),
           line("device-to-device copy", t_copy),
           "per frame: streak_search %.3f ms, Radon.search %.3f ms, copy %.3f ms (%.1f MB)" % (ms / a.frames, mr / a.frames, mc / a.frames,
                                                                                               nbytes / a.frames / 1e6),
           "streak_search / Radon.search %.2f, streak_search / copy %.1f" % (ms / mr, ms / mc),
           "largest noise peak over the %d full frames %.2f (found: %d frames); the crops' ceiling is %.2f" % (a.frames, peak, int((ns > 0).sum()),
                                                                                                              CROP_CEILING),
           "what bounds k_streak_search: unmeasured (no kernel trace was taken)"]
    print("\n".join(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
