"""Times lfdmi_subtract_trails on 256 device-resident SDSS frames of noise: one full-length segment per frame (half 14 px: the
masks' default 8 plus the wing of 6; the default parameters, sections of 32 px), no mask plane; and in the same run
lfdmi_trail_strips on the same segments at the same sec_len (the same cells, copied back to the host), lfdmi_mask_trails with a
zero fill at the same half-width on a copy of the frames, and a device-to-device copy of the frames.  HIP events on the context's
stream (and a host clock around each call, which waits for the stream); two warm-ups, then --reps repetitions; median, minimum
and maximum of each, and the ratios of the subtraction to the other three.  The subtraction changes the frames in place, so every
repetition subtracts the model of what the one before left: the work per call is the same.  Writes profiles/sub_probe.txt.

    python tools/sub_probe.py [--reps 20] [--frames 256]

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
    from lfd_amd import _native, recovery, strips, synth
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
    msegs = np.zeros(len(segs), _native.MASK_SEGMENT_DTYPE)
    for k in ("frame", "x1", "y1", "x2", "y2", "half"):
        msegs[k] = segs[k]
    msegs["bits"] = 1
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    names = ("sub", "strip", "mask", "copy")
    t_ev = {k: [] for k in names}
    t_host = {k: [] for k in names}

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
            t_host[name].append(1e3 * (t1 - t0))
        return out

    sec_len = float(_native.make_sub_params().sec_len)
    with _native.Context(0, *shape, 2) as ctx:
        ctx.set_stream(stream.cuda_stream)
        mc = _native.strip_cells_needed(segs, _native.make_sub_params(), 512)
        for rep in range(a.reps + 2):                      # two warm-ups: module load, the stream pool's first allocations
            timed("copy", lambda: other.copy_(base), rep)
            timed("mask", lambda: ctx.mask_trails(other, msegs, mask=False, fill="zero"), rep)
            srec, ssec, cells = timed("strip", lambda: ctx.trail_strips(base, segs, max_sections=512, max_cells=mc, sec_len=sec_len), rep)
            rec, _ = timed("sub", lambda: ctx.subtract_trails(base, segs, max_sections=512, max_cells=mc), rep)
    ok = rec["status"] == _native.SUB_OK
    print("RESULT " + json.dumps({"frames": n, "shape": list(shape), "reps": a.reps, "half": a.half, "sec_len": sec_len,
                                  "segments_ok": int(ok.sum()), "sections": int(rec["n_sec"].sum()), "usable": int(rec["n_usable"].sum()),
                                  "cells": int((rec["n_sec"].astype(np.int64) * rec["n_off"]).sum()), "model_cells": int(rec["n_model"].sum()),
                                  "pixels": int(rec["n_pix"].sum()), "band_pixels": int(cells["n_geom"].sum()),
                                  "cell_bytes": int(cells.nbytes), "n_off": int(rec["n_off"].max()),
                                  "event_ms": t_ev, "host_ms": t_host}), flush=True)


def stats(v):
    import numpy as np
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--half", type=float, default=14.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sub_probe.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames),
           "--half", str(a.half)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("sub_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    px = r["frames"] * r["shape"][0] * r["shape"][1]
    e, hst = r["event_ms"], r["host_ms"]
    su, sp, mk, cp = (float(np.median(e[k])) for k in ("sub", "strip", "mask", "copy"))
    hsu, hsp = float(np.median(hst["sub"])), float(np.median(hst["strip"]))
    lines = ["# tools/sub_probe.py: %d device-resident frames of %d x %d of noise, one full-length segment per frame (half %g px, default"
             % (r["frames"], r["shape"][0], r["shape"][1], r["half"]),
             "# parameters: sections of %g px by %d bins of 1 px, smooth 2), no mask plane; %d repetitions after 2 warm-ups; times in ms"
             % (r["sec_len"], r["n_off"], r["reps"]),
             "segments OK %d of %d, sections %d (usable %d), cells %d (with a model %d), pixels changed in the last call %d" % (
                 r["segments_ok"], r["frames"], r["sections"], r["usable"], r["cells"], r["model_cells"], r["pixels"]),
             "band pixels (|u| <= half, t in [0, L]) %d of %d (%.2f %%); trail_strips copies %.1f MB of cells to the host, subtract_trails none"
             % (r["band_pixels"], px, 100.0 * r["band_pixels"] / px, r["cell_bytes"] / 1e6),
             "subtract_trails, HIP events on the context's stream:        " + stats(e["sub"]),
             "subtract_trails, host clock around the call:                " + stats(hst["sub"]),
             "trail_strips on the same segments (sec_len %g), events:     %s" % (r["sec_len"], stats(e["strip"])),
             "trail_strips, host clock around the call:                   " + stats(hst["strip"]),
             "mask_trails(fill=zero) at the same half-width, events:      " + stats(e["mask"]),
             "device-to-device copy of the same frames (events):          " + stats(e["copy"]),
             "events: subtract_trails / trail_strips %.2f; / mask_trails(fill=zero) %.2f; / copy %.3f" % (su / sp, su / mk, su / cp),
             "host clock: subtract_trails / trail_strips %.2f" % (hsu / hsp)]
    lines += ["%s_event_ms " % k + " ".join("%.3f" % v for v in e[k]) for k in ("sub", "strip", "mask", "copy")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
