"""Times lfdmi_trail_strips on 256 device-resident SDSS frames of noise: one full-length segment per frame (half 14 px: the masks'
default 8 plus the wing of 6; the default parameters), no mask plane; and in the same run lfdmi_light_curves on the same segments
(half 14, the default sky bands: the nearest existing kernel, with the same cull, loads and membership arithmetic and a smaller
table) and a device-to-device copy of the same frames.  HIP events on the context's stream (and a host clock around the call,
which waits for the stream and, for the strips, copies the cells back); two warm-ups, then --reps repetitions; median, minimum and
maximum of each.  Writes profiles/strip_probe.txt.

    python tools/strip_probe.py [--reps 20] [--frames 256]

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
    from lfd_amd import _native, lightcurve, recovery, strips, synth
    n, shape = a.frames, synth.SDSS_SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((n, *shape), generator=g, device="cuda", dtype=torch.float32) * 0.025
    other = torch.empty_like(base)
    rows = []
    for t in recovery.to_inject(recovery.draw_trails(n, shape, 1, [0.1])):   # each line's crossing of the frame as a segment
        th = float(t["theta"])
        c, s = math.cos(th), math.sin(th)
        ta, tb = recovery.extent(float(t["rho"]), th, -np.inf, np.inf, shape)
        rows.append((t["frame"], t["rho"] * c - ta * s, t["rho"] * s + ta * c, t["rho"] * c - tb * s, t["rho"] * s + tb * c, a.half))
    segs = strips.segments(rows)
    lsegs = lightcurve.segments(rows)
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_ev = {"strip": [], "lc": [], "copy": []}
    t_host = {"strip": [], "lc": []}

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
        mc = _native.strip_cells_needed(segs, _native.make_strip_params(), 512)
        for rep in range(a.reps + 2):                      # two warm-ups: module load, the stream pool's first allocations
            rec, sec, cells = timed("strip", lambda: ctx.trail_strips(base, segs, max_sections=512, max_cells=mc), rep)
            lrec, lsec = timed("lc", lambda: ctx.light_curves(base, lsegs, max_sections=512, sec_len=8.0), rep)
            timed("copy", lambda: other.copy_(base), rep)
    ok = rec["status"] == _native.STRIP_OK
    ncell = (rec["n_sec"].astype(np.int64) * rec["n_off"]).sum()
    same = all(np.array_equal(cells[i][:int(r["n_sec"]) * int(r["n_off"])]["n_geom"].reshape(int(r["n_sec"]), -1).sum(1),
                              lsec[i, :int(r["n_sec"])]["n_geom"]) for i, r in enumerate(rec) if ok[i])
    print("RESULT " + json.dumps({"frames": n, "shape": list(shape), "reps": a.reps, "half": a.half, "segments_ok": int(ok.sum()),
                                  "sections": int(rec["n_sec"].sum()), "sections_ok": int(rec["n_ok"].sum()), "cells": int(ncell),
                                  "band_pixels": int(cells["n_geom"].sum()), "n_off": int(rec["n_off"].max()),
                                  "sums_equal_light_curves": bool(same),
                                  "strip_event_ms": t_ev["strip"], "strip_host_ms": t_host["strip"], "lc_event_ms": t_ev["lc"],
                                  "lc_host_ms": t_host["lc"], "copy_event_ms": t_ev["copy"]}), flush=True)


def stats(v):
    import numpy as np
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--half", type=float, default=14.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_probe.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames),
           "--half", str(a.half)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("strip_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    px = r["frames"] * r["shape"][0] * r["shape"][1]
    sp, lc, cp = (float(np.median(r[k])) for k in ("strip_event_ms", "lc_event_ms", "copy_event_ms"))
    lines = ["# tools/strip_probe.py: %d device-resident frames of %d x %d of noise, one full-length segment per frame (half %g px, default"
             % (r["frames"], r["shape"][0], r["shape"][1], r["half"]),
             "# parameters: sections of 8 px by %d bins of 1 px), no mask plane; %d repetitions after 2 warm-ups; times in ms" % (r["n_off"], r["reps"]),
             "segments OK %d of %d, sections %d (OK %d), cells %d" % (r["segments_ok"], r["frames"], r["sections"], r["sections_ok"], r["cells"]),
             "band pixels (|u| <= half, t in [0, L]) %d of %d (%.2f %%); summed over the bins the cells equal light_curves' n_geom: %s" % (
                 r["band_pixels"], px, 100.0 * r["band_pixels"] / px, r["sums_equal_light_curves"]),
             "trail_strips, HIP events on the context's stream:        " + stats(r["strip_event_ms"]),
             "trail_strips, host clock around the call:                " + stats(r["strip_host_ms"]),
             "light_curves on the same segments (sec_len 8), events:   " + stats(r["lc_event_ms"]),
             "light_curves, host clock around the call:                " + stats(r["lc_host_ms"]),
             "device-to-device copy of the same frames (events):       " + stats(r["copy_event_ms"]),
             "trail_strips / light_curves %.2f; trail_strips / copy %.3f" % (sp / lc, sp / cp),
             "strip_event_ms " + " ".join("%.3f" % v for v in r["strip_event_ms"]),
             "lc_event_ms " + " ".join("%.3f" % v for v in r["lc_event_ms"]),
             "copy_event_ms " + " ".join("%.3f" % v for v in r["copy_event_ms"])]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
