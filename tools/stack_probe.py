"""Device time of lfdmi_stack_profiles: 256 device-resident SDSS frames (1489 x 2048) with 1 and with 4 full-length segments
each, per call between HIP events (the median of several calls), and the bytes the kernel must move -- every pixel of every
band once per pass -- with the time that floor takes at the memory bandwidth given.

    python tools/stack_probe.py [--frames 256] [--calls 5] [--n-iter 2] [--bandwidth-tbs 8.0]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def band_bytes(segs, shape, prof_half=24.0, step=0.5):
    """bytes of the pixels within the band of every segment, once: 4 * columns * 2 (P + step / 2) / cosphi"""
    h, w = shape
    total = 0.0
    for s in segs:
        dx, dy = s["x2"] - s["x1"], s["y2"] - s["y1"]
        xmajor = abs(dx) >= abs(dy)
        g = (dy / dx) if xmajor else (dx / dy)
        a = sorted((s["x1"], s["x2"]) if xmajor else (s["y1"], s["y2"]))
        cols = max(0, min(math.floor(a[1]), (w if xmajor else h) - 1) - max(math.ceil(a[0]), 0) + 1)
        total += 4.0 * cols * 2.0 * (prof_half + step / 2.0) * math.sqrt(1.0 + g * g)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--n-iter", type=int, default=2)
    ap.add_argument("--bandwidth-tbs", type=float, default=8.0)
    args = ap.parse_args()
    import torch
    from lfd_amd import _native, stack
    shape = (1489, 2048)
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randn((n, *shape), generator=gen, device="cuda", dtype=torch.float32) * 0.025
    rng = np.random.default_rng(2)
    out = {"frames": n, "n_iter": args.n_iter, "passes": args.n_iter + 1}
    with _native.Context(0, *shape, 1) as ctx:
        for per in (1, 4):
            rows = []
            for f in range(n):
                for k in range(per):                       # full crossings, shallow and steep alternating
                    if k % 2 == 0:
                        y = rng.uniform(100, shape[0] - 100, 2)
                        rows.append((f, -1.0, y[0], shape[1] + 1.0, y[1]))
                    else:
                        x = rng.uniform(100, shape[1] - 100, 2)
                        rows.append((f, x[0], -1.0, x[1], shape[0] + 1.0))
            segs = stack.segments(rows)
            ctx.stack_profiles(frames, segs, n_iter=args.n_iter)          # (warm-up: the stream pool grows here)
            ms = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.stack_profiles(frames, segs, n_iter=args.n_iter)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            b = band_bytes(segs, shape)
            floor_ms = b / (args.bandwidth_tbs * 1e12) * 1e3
            med = float(np.median(ms))
            # noise frames stop after their first pass (no half reaches k_ref sigma): the floor is one pass
            out[f"segments_per_frame_{per}"] = {"segments": len(segs), "ms_per_call": round(med, 3), "ms_per_frame": round(med / n, 4),
                                                "band_bytes_per_pass": int(b), "floor_ms_per_pass": round(floor_ms, 3),
                                                "ratio_to_floor": round(med / floor_ms, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
