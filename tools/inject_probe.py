"""Times lfdmi_inject_trails on 256 device-resident SDSS frames: one full-length Gaussian trail (sigma 2 px) per frame,
subsample 4, and in the same run a device-to-device copy of the same 256 frames -- the yardstick for touching every pixel.
HIP events on the context's stream (and a host clock around the call, which waits for the stream); a warm-up, then --reps
repetitions; median, minimum and maximum of each.  Writes profiles/inject_probe.txt.

    python tools/inject_probe.py [--reps 20] [--frames 256]

The GPU step is a child process under its own `timeout`.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch
    from lfd_amd import _native, inject, recovery, synth
    n, shape = a.frames, synth.SDSS_SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((n, *shape), generator=g, device="cuda", dtype=torch.float32) * 0.025
    work = base.clone()
    table, step = inject.gaussian_table(2.0)
    table = inject.normalise_peak(table).astype(np.float32)
    tr = recovery.to_inject(recovery.draw_trails(n, shape, 1, [0.1]))
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    inj_ev, inj_host, cp_ev = [], [], []
    with _native.Context(0, *shape, 2) as ctx:
        ctx.set_stream(stream.cuda_stream)
        for rep in range(a.reps + 2):                      # two warm-ups: module load, the stream pool's first allocations
            work.copy_(base)
            torch.cuda.synchronize()
            ev[0].record(stream)
            t0 = time.perf_counter()
            ctx.inject_trails(work, tr, table, step, subsample=4)
            t1 = time.perf_counter()
            ev[1].record(stream)
            torch.cuda.synchronize()
            if rep >= 2:
                inj_ev.append(ev[0].elapsed_time(ev[1]))
                inj_host.append(1e3 * (t1 - t0))
            ev[0].record(stream)
            work.copy_(base)
            ev[1].record(stream)
            torch.cuda.synchronize()
            if rep >= 2:
                cp_ev.append(ev[0].elapsed_time(ev[1]))
        ctx.inject_trails(work, tr, table, step, subsample=4)
        changed = int((work != base).sum().item())
    print("RESULT " + json.dumps({"frames": n, "shape": list(shape), "reps": a.reps, "table_len": len(table), "table_step": step,
                                  "pixels_changed": changed, "inject_event_ms": inj_ev, "inject_host_ms": inj_host,
                                  "copy_event_ms": cp_ev}), flush=True)


def stats(v):
    import numpy as np
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inject_probe.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("inject_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    r = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    px = r["frames"] * r["shape"][0] * r["shape"][1]
    lines = ["# tools/inject_probe.py: %d device-resident frames of %d x %d, one full-length Gaussian trail (sigma 2 px, table of %d nodes"
             % (r["frames"], r["shape"][0], r["shape"][1], r["table_len"]),
             "# at %.3f px) per frame, subsample 4; %d repetitions after 2 warm-ups; times in ms" % (r["table_step"], r["reps"]),
             "pixels_changed %d of %d (%.2f %%)" % (r["pixels_changed"], px, 100.0 * r["pixels_changed"] / px),
             "inject_trails, HIP events on the context's stream:  " + stats(r["inject_event_ms"]),
             "inject_trails, host clock around the call:          " + stats(r["inject_host_ms"]),
             "device-to-device copy of the same frames (events):  " + stats(r["copy_event_ms"]),
             "inject_event_ms " + " ".join("%.3f" % v for v in r["inject_event_ms"]),
             "copy_event_ms " + " ".join("%.3f" % v for v in r["copy_event_ms"])]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
