"""Times lfdmi_light_curves on 256 device-resident SDSS frames of noise: one full-length segment per frame (half 8 px, the default
sky bands and parameters), no mask plane; and in the same run lfdmi_mask_trails on the same segments (the nearest existing
kernel: the same membership arithmetic on a band of half-width 8, which reads no pixel) and a device-to-device copy of the same
frames.  HIP events on the context's stream (and a host clock around the call, which waits for the stream); two warm-ups, then
--reps repetitions; median, minimum and maximum of each.  Also the ratio to the band's byte floor: 4 bytes for every pixel within
bg_out of a segment, at 8 TB/s.  Writes profiles/lc_probe.txt.

    python tools/lc_probe.py [--reps 20] [--frames 256]

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

HBM_BYTES_PER_S = 8e12


def child(a):
    import numpy as np
    import torch
    from lfd_amd import _native, lightcurve, masks, recovery, synth
    n, shape = a.frames, synth.SDSS_SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((n, *shape), generator=g, device="cuda", dtype=torch.float32) * 0.025
    other = torch.empty_like(base)
    plane = torch.empty((n, *shape), dtype=torch.uint8, device="cuda")
    rows = []
    for t in recovery.to_inject(recovery.draw_trails(n, shape, 1, [0.1])):   # each line's crossing of the frame as a segment
        th = float(t["theta"])
        c, s = math.cos(th), math.sin(th)
        ta, tb = recovery.extent(float(t["rho"]), th, -np.inf, np.inf, shape)
        rows.append((t["frame"], t["rho"] * c - ta * s, t["rho"] * s + ta * c, t["rho"] * c - tb * s, t["rho"] * s + tb * c, a.half))
    segs = lightcurve.segments(rows)
    msegs = masks.segments(rows, bits=1, cap=0.0)
    band = masks.segments([(*r[:5], float(segs[i]["bg_out"])) for i, r in enumerate(rows)], bits=1, cap=0.0)
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_ev = {"lc": [], "mask": [], "copy": []}
    t_host = {"lc": [], "mask": []}

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
            rec, sec = timed("lc", lambda: ctx.light_curves(base, segs, max_sections=128), rep)
            timed("mask", lambda: ctx.mask_trails(None, msegs, mask=plane), rep)
            timed("copy", lambda: other.copy_(base), rep)
        _, bstats, _ = ctx.mask_trails(None, band, mask=plane)
    ok = rec["status"] == _native.LC_OK
    print("RESULT " + json.dumps({"frames": n, "shape": list(shape), "reps": a.reps, "half": a.half, "segments_ok": int(ok.sum()),
                                  "sections": int(rec["n_sec"].sum()), "sections_ok": int(rec["n_ok"].sum()),
                                  "core_pixels": int(sec["n_geom"].sum()), "sky_pixels": int(sec["n_sky"].sum()),
                                  "band_pixels": int(bstats["n_pix"].sum()), "bg_out": float(segs[0]["bg_out"]),
                                  "chi2_dof_median": float(np.median(lightcurve.variability(rec[ok]))),
                                  "lc_event_ms": t_ev["lc"], "lc_host_ms": t_host["lc"], "mask_event_ms": t_ev["mask"],
                                  "copy_event_ms": t_ev["copy"]}), flush=True)


def stats(v):
    import numpy as np
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--half", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lc_probe.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames),
           "--half", str(a.half)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("lc_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    px = r["frames"] * r["shape"][0] * r["shape"][1]
    lc, mk, cp = (float(np.median(r[k])) for k in ("lc_event_ms", "mask_event_ms", "copy_event_ms"))
    floor_ms = 1e3 * 4.0 * r["band_pixels"] / HBM_BYTES_PER_S
    lines = ["# tools/lc_probe.py: %d device-resident frames of %d x %d of noise, one full-length segment per frame (half %g px, sky bands"
             % (r["frames"], r["shape"][0], r["shape"][1], r["half"]),
             "# out to %g px, default parameters), no mask plane; %d repetitions after 2 warm-ups; times in ms" % (r["bg_out"], r["reps"]),
             "segments OK %d of %d, sections %d (OK %d), median chi2 / dof %.3f" % (r["segments_ok"], r["frames"], r["sections"], r["sections_ok"],
                                                                                  r["chi2_dof_median"]),
             "band pixels (|u| <= bg_out, t in [0, L]) %d of %d (%.2f %%); core %d, valid sky %d" % (
                 r["band_pixels"], px, 100.0 * r["band_pixels"] / px, r["core_pixels"], r["sky_pixels"]),
             "light_curves, HIP events on the context's stream:   " + stats(r["lc_event_ms"]),
             "light_curves, host clock around the call:           " + stats(r["lc_host_ms"]),
             "mask_trails on the same segments, mask only:        " + stats(r["mask_event_ms"]),
             "device-to-device copy of the same frames (events):  " + stats(r["copy_event_ms"]),
             "light_curves / mask_trails %.2f; light_curves / copy %.3f" % (lc / mk, lc / cp),
             "byte floor of the band (4 bytes a pixel at 8 TB/s) %.4f ms; light_curves / floor %.1f" % (floor_ms, lc / floor_ms),
             "lc_event_ms " + " ".join("%.3f" % v for v in r["lc_event_ms"]),
             "mask_event_ms " + " ".join("%.3f" % v for v in r["mask_event_ms"]),
             "copy_event_ms " + " ".join("%.3f" % v for v in r["copy_event_ms"])]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
