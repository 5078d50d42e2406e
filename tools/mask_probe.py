"""Times lfdmi_mask_trails on 256 device-resident SDSS frames: one full-length segment of half-width 8 px per frame, a device
mask plane per frame and a zero fill, and in the same run a device-to-device copy of the same 256 frames -- the yardstick for
touching every pixel -- and tools/inject_probe.py's call (one full-length Gaussian trail per frame, subsample 4) on the same
lines.  HIP events on the context's stream (and a host clock around the call, which waits for the stream); two warm-ups, then
--reps repetitions; median, minimum and maximum of each.  Writes profiles/mask_probe.txt.

    python tools/mask_probe.py [--reps 20] [--frames 256]

The GPU step is a child process under its own `timeout`.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch
    from lfd_amd import _native, inject, masks, recovery, synth
    n, shape = a.frames, synth.SDSS_SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((n, *shape), generator=g, device="cuda", dtype=torch.float32) * 0.025
    work = base.clone()
    plane = torch.empty((n, *shape), dtype=torch.uint8, device="cuda")
    table, step = inject.gaussian_table(2.0)
    table = inject.normalise_peak(table).astype(np.float32)
    tr = recovery.to_inject(recovery.draw_trails(n, shape, 1, [0.1]))
    rows = []
    for t in tr:                                           # the trail's line as a segment: foot point -+ 100 px, the whole line
        c, s = math.cos(t["theta"]), math.sin(t["theta"])
        fx, fy = t["rho"] * c, t["rho"] * s
        rows.append((t["frame"], fx + 100.0 * s, fy - 100.0 * c, fx - 100.0 * s, fy + 100.0 * c, a.half))
    segs = masks.segments(rows, bits=1, cap=np.inf)
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_ev = {"mask": [], "inject": [], "copy": []}
    t_host = {"mask": [], "inject": []}

    def timed(name, fn, rep):
        torch.cuda.synchronize()
        ev[0].record(stream)
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        ev[1].record(stream)
        torch.cuda.synchronize()
        if rep >= 2:
            t_ev[name].append(ev[0].elapsed_time(ev[1]))
            if name in t_host:
                t_host[name].append(1e3 * (t1 - t0))
        return out

    with _native.Context(0, *shape, 2) as ctx:
        ctx.set_stream(stream.cuda_stream)
        for rep in range(a.reps + 2):                      # two warm-ups: module load, the stream pool's first allocations
            work.copy_(base)
            _, stats, counts = timed("mask", lambda: ctx.mask_trails(work, segs, mask=plane, fill="zero"), rep)
            work.copy_(base)
            timed("inject", lambda: ctx.inject_trails(work, tr, table, step, subsample=4), rep)
            timed("copy", lambda: work.copy_(base), rep)
        work.copy_(base)
        torch.cuda.synchronize()                           # (the call runs on the context's stream: the copy must have landed)
        _, stats, counts = ctx.mask_trails(work, segs, mask=plane, fill="zero")
        flagged = int((plane != 0).sum().item())
        zeroed = int(((work == 0) & (plane != 0)).sum().item())
        outside = int(((plane == 0) & (work.view(torch.int32) != base.view(torch.int32))).sum().item())
    assert flagged == zeroed == int(counts.sum()) == int(stats["n_pix"].sum()) and outside == 0, (
        flagged, zeroed, int(counts.sum()), int(stats["n_pix"].sum()), outside)
    print("RESULT " + json.dumps({"frames": n, "shape": list(shape), "reps": a.reps, "half": a.half, "pixels_flagged": flagged,
                                  "pixels_zeroed": zeroed, "mask_event_ms": t_ev["mask"], "mask_host_ms": t_host["mask"],
                                  "inject_event_ms": t_ev["inject"], "copy_event_ms": t_ev["copy"]}), flush=True)


def stats(v):
    import numpy as np
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--half", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_probe.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames),
           "--half", str(a.half)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("mask_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    px = r["frames"] * r["shape"][0] * r["shape"][1]
    lines = ["# tools/mask_probe.py: %d device-resident frames of %d x %d, one full-length segment of half-width %g px per frame,"
             % (r["frames"], r["shape"][0], r["shape"][1], r["half"]),
             "# device mask planes (cleared by the call) and a zero fill; %d repetitions after 2 warm-ups; times in ms" % r["reps"],
             "pixels_flagged %d of %d (%.2f %%), pixels_zeroed %d" % (r["pixels_flagged"], px, 100.0 * r["pixels_flagged"] / px, r["pixels_zeroed"]),
             "mask_trails, HIP events on the context's stream:    " + stats(r["mask_event_ms"]),
             "mask_trails, host clock around the call:            " + stats(r["mask_host_ms"]),
             "device-to-device copy of the same frames (events):  " + stats(r["copy_event_ms"]),
             "inject_trails on the same lines (events):           " + stats(r["inject_event_ms"]),
             "mask_event_ms " + " ".join("%.3f" % v for v in r["mask_event_ms"]),
             "copy_event_ms " + " ".join("%.3f" % v for v in r["copy_event_ms"]),
             "inject_event_ms " + " ".join("%.3f" % v for v in r["inject_event_ms"])]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
