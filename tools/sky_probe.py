"""Times lfdmi_sky_normalize on device-resident frames: 256 SDSS frames, and as many 4096 x 4096 frames as fit --budget-gb of
device memory beside the handle's buffer (input + output buffer: two copies), at cell 64 and 128, against the 12 B/px floor
(two reads, one write).  Writes profiles/sky_probe.json.

    python tools/sky_probe.py [--reps 5] [--budget-gb 40] [--trace] [--counters]

--trace     one more run per cell under `rocprofv3 --kernel-trace --stats` -> profiles/sky_probe_kernel_stats.csv (cell 64) and
            profiles/sky_probe_kernel_stats_cell128.csv
--counters  two counter passes (runs of their own: --pmc with --kernel-trace only) at cell 64 -> profiles/sky_probe_counters.txt
Every GPU step is a child process under its own `timeout` (which signals the child's whole process group).
"""
import argparse
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PMC = (("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS"),
       ("SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_WAIT_ANY", "SQ_LDS_BANK_CONFLICT"))


def one(name, shape, n, cell, reps):
    import numpy as np
    import torch
    from lfd_amd import _native
    h, w = shape
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randn((n, h, w), generator=g, device="cuda", dtype=torch.float32) * 30 + 1000
    with _native.Context(0, h, w, 2) as ctx, _native.Sky(ctx, shape, max_frames=n, cell=cell) as sky:
        sky.normalize(frames)                                  # warm-up: module load, first touch
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = sky.normalize(frames)
            ts.append(time.perf_counter() - t0)
    ms = 1e3 * float(np.median(ts))
    floor_bytes = 12.0 * n * h * w
    return {"frames": name, "n": n, "shape": list(shape), "cell": cell, "ms_per_call": ms, "ms_all": [1e3 * t for t in ts],
            "bytes_floor": floor_bytes, "achieved_TBps_of_floor_bytes": floor_bytes / (ms * 1e-3) / 1e12,
            "ms_floor_at_4.8_TBps": floor_bytes / 4.8e12 * 1e3, "status_ok": int((rec["status"] == 0).sum()),
            "sigma_median": float(np.median(rec["sigma"]))}


def child(a):
    """the measuring process: one JSON line per configuration on stdout"""
    n_lsst = max(1, int(a.budget_gb * 1e9 // (2 * 4096 * 4096 * 4)))
    legs = [("sdss", (1489, 2048), a.frames or 256), ("lsst", (4096, 4096), n_lsst)]
    for name, shape, n in legs:
        if a.leg and name != a.leg:
            continue
        for cell in ((a.cell,) if a.cell else (64, 128)):
            print("RESULT " + json.dumps(one(name, shape, n, cell, a.reps)), flush=True)


def run_child(extra, timeout_s, prefix=()):
    cmd = ["timeout", "-k", "10", str(timeout_s), *prefix, sys.executable, os.path.abspath(__file__), "--child", *extra]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("sky_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    return [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget-gb", type=float, default=40.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", default="")
    ap.add_argument("--cell", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)
    doc = {"tool": "tools/sky_probe.py", "copy_rate_yardstick_TBps": [4.8, 5.7],
           "runs": run_child(["--reps", str(a.reps), "--budget-gb", str(a.budget_gb)], 600)}
    for r in doc["runs"]:
        print(r, flush=True)
    with open(os.path.join(prof, "sky_probe.json"), "w") as f:
        json.dump(doc, f, indent=1)
    small = ["--leg", "sdss", "--reps", "1"]
    if a.trace:
        for cell, name in ((64, "sky_probe_kernel_stats.csv"), (128, "sky_probe_kernel_stats_cell128.csv")):
            tmp = tempfile.mkdtemp(prefix="sky_probe_")
            try:
                run_child(small + ["--cell", str(cell)], 300,
                          ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "sky", "--output-format", "csv", "--"])
                found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                if not found:
                    raise SystemExit("sky_probe: rocprofv3 wrote no kernel_stats.csv")
                shutil.copy(found[0], os.path.join(prof, name))
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    if a.counters:
        acc = collections.defaultdict(lambda: collections.defaultdict(float))
        cnt = collections.defaultdict(lambda: collections.defaultdict(int))
        for pmc in PMC:
            tmp = tempfile.mkdtemp(prefix="sky_probe_")
            try:
                run_child(small + ["--cell", "64", "--frames", "64"], 300,
                          ["rocprofv3", "--kernel-trace", "--pmc", *pmc, "-d", tmp, "--output-format", "csv", "--"])
                for fn in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                    with open(fn) as f:
                        for r in csv.DictReader(f):
                            k = r["Kernel_Name"].split("(")[0]
                            acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
                            cnt[k][r["Counter_Name"]] += 1
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        with open(os.path.join(prof, "sky_probe_counters.txt"), "w") as f:
            f.write("# 64 SDSS frames, cell 64, two launches per kernel (warm-up + 1); counter sums per launch\n")
            for k in sorted(acc):
                if "sky" in k:
                    f.write(k[:60] + " " + " ".join("%s=%.4g" % (c, acc[k][c] / cnt[k][c]) for c in sorted(acc[k])) + "\n")


if __name__ == "__main__":
    main()
