"""Calls in flight, measured in one process: blocks of synchronous ``detect`` / ``multiscale``, the two-context stand-in
(``BatchDetector(calls_in_flight=2).detect_async``) and ``BatchDetector.submit`` (two calls in flight on one workspace),
alternated, after warm-up, ``--repeats`` times.  Prints one JSON line per block and a summary (ms/step, frames/s, spread,
workspace bytes of each).

  python tools/submit_probe.py --workload sdss --frames 256 --steps 20 --warmup 3 --repeats 5
  python tools/submit_probe.py --workload lsst ...                       # the 4096 x 4096 multi-scale dim pass
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/submit_probe.py --only submit --repeats 1
  python tools/submit_probe.py --gaps DIR/.../kernel_trace.csv --marker k_rs_boxes   # idle time before each call's first kernel
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gaps(path, marker):
    """Idle time (ms) between the end of the kernel before each call's first kernel (a launch whose name contains `marker`,
    not preceded by another such launch) and that kernel's start."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    out = []
    for i in range(1, len(rows)):
        if marker in rows[i][2] and marker not in rows[i - 1][2]:
            out.append((rows[i][0] - max(r[1] for r in rows[max(0, i - 64):i])) / 1e6)
    g = np.array(out) if out else np.zeros(1)
    return {"marker": marker, "calls": len(out), "gap_ms_median": float(np.median(g)), "gap_ms_p90": float(np.percentile(g, 90)),
            "gap_ms_max": float(g.max()), "gap_ms_min": float(g.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sdss", choices=("sdss", "lsst"))
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated subset of sync,standin,submit")
    ap.add_argument("--gaps", default="", help="a rocprofv3 kernel_trace.csv: print the inter-call gaps and exit")
    ap.add_argument("--marker", default="k_rs_boxes")
    args = ap.parse_args()
    if args.gaps:
        print(json.dumps(gaps(args.gaps, args.marker)))
        return
    import torch
    from lfd_amd import _native, synth
    from lfd_amd.batch import BatchDetector
    from lfd_amd.detecttrails import default_params

    lsst = args.workload == "lsst"
    shape = synth.LSST_SHAPE if lsst else synth.SDSS_SHAPE
    n, nd = args.frames, min(args.frames, args.distinct)
    host, cats = synth.make_frames(0, nd, shape, 8, with_catalog=not lsst)[:2]
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    rhos = [20.0, 10.0, 5.0]
    if lsst:
        pd = dict(pd, erodeKernel=np.ones((9, 9), np.uint8))
    dev = torch.device("cuda", 0)
    idx = torch.arange(n, device=dev) % nd
    base = torch.from_numpy(host).to(dev)[idx].contiguous()
    frames = [base, base.clone()]                  # two buffers: frames of two calls in flight must not overlap
    cat = None
    if not lsst:
        packed = synth.pack_catalogs([cats[i % nd] for i in range(n)])
        cat = {k: torch.from_numpy(v).to(dev) for k, v in packed.items()}
    stream = torch.cuda.current_stream().cuda_stream
    only = set(filter(None, args.only.split(","))) or {"sync", "standin", "submit"}
    det = BatchDetector(0, shape, n, stream=stream)
    std = BatchDetector(0, shape, n, stream=stream, calls_in_flight=2) if "standin" in only else None

    def call(mode, k):
        f = frames[k & 1]
        if mode == "sync":
            return det.multiscale(f, pd, rhos) if lsst else det.detect(f, pb, pd, cat, rs)
        if mode == "standin":
            return std.multiscale_async(f, pd, rhos) if lsst else std.detect_async(f, pb, pd, cat, rs)
        return det.submit_multiscale(f, pd, rhos) if lsst else det.submit(f, pb, pd, cat, rs)

    def block(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prev = None
        for k in range(steps):
            cur = call(mode, k)
            if mode != "sync":                     # two in flight: the next call is queued before the previous one is read
                if prev is not None:
                    prev.result()
                prev = cur
        if prev is not None:
            prev.result()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    modes = [m for m in ("sync", "standin", "submit") if m in only]
    for m in modes:
        block(m, args.warmup)
    ws = {"sync": det.workspace_bytes(), "submit": det.workspace_bytes()}
    if std is not None:
        ws["standin"] = std.workspace_bytes()
    ms = {m: [] for m in modes}
    for r in range(args.repeats):
        for m in modes:
            t = block(m, args.steps)
            ms[m].append(t)
            print(json.dumps({"workload": args.workload, "repeat": r, "mode": m, "ms_per_step": round(t, 4),
                              "frames_per_s": round(n / t * 1e3, 1)}), flush=True)
    summary = {"workload": args.workload, "frames_per_step": n, "distinct": nd, "steps": args.steps, "repeats": args.repeats}
    for m in modes:
        a = np.array(ms[m])
        summary[m] = {"ms_per_step_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4),
                      "ms_max": round(float(a.max()), 4), "frames_per_s_median": round(n / float(np.median(a)) * 1e3, 1),
                      "workspace_bytes": ws[m], "spilled": det.spill_count() if m != "standin" else std.spill_count()}
    print(json.dumps({"summary": summary}), flush=True)
    det.close()
    if std is not None:
        std.close()


if __name__ == "__main__":
    main()
