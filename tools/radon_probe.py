"""Times lfdmi_radon_search on 256 device-resident SDSS frames at bin 1, 2 and 4: ms per call as the median of repeated calls
between HIP events, beside the bytes each kernel has to move (the rows a level stores, read once and written once, sums and
16-bit counts) and the floor those bytes give at the copy rate the project quotes (4.8 TB/s, DESIGN.md: sky normalisation).
Writes profiles/radon_probe.json.

    python tools/radon_probe.py [--reps 5] [--frames 256] [--max-frames 16] [--out FILE] [--trace] [--lines K] [--short] [--wide]

--lines K  also times lfdmi_radon_search_lines(max_lines=K) on the same frames with one faint streak added to every second
           frame: ms per call and per round (a frame runs one round more than it has found lines, K at the most), beside the
           plain search's time

--short    also times lfdmi_radon_search_short(max_lines=K) in the same run on the same frames and settings (K of --lines,
           4 without it): ms per call and per frame-round, and the ratio of its frame-round to search_lines' frame-round,
           which is the yardstick: the scoring levels move the same bytes, so the ratio shows what the scores cost

--wide     also times lfdmi_radon_search_wide(max_lines=K, max_width 8) in the same run on the same frames (K of --lines, 4
           without it): ms per call and per frame-round, and the ratio of its frame-round to search_lines' frame-round: the wide
           call stores the last level and reads it back, which search_lines never does, and scores four widths

--trace  one more run per bin (32 frames, one timed call of each search asked for) under `rocprofv3 --kernel-trace --stats`
         -> <--out without .json>_kernel_stats_bin<b>.csv beside --out (default: profiles/radon_probe_kernel_stats_bin<b>.csv)
Every GPU step is a child process under its own `timeout`.
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 4.8e12
SHAPE = (1489, 2048)


def kernel_bytes(shape, b):
    """bytes per frame each kernel must move: {kernel: bytes}; a stored value is 6 bytes (float32 sum + 16-bit count)"""
    from lfd_amd import radon
    hb, wb, p01, p23 = radon.working_dims(shape, b)
    out = {"k_radon_prep": 4 * shape[0] * shape[1] + 6 * hb * wb, "k_radon_first": 0, "k_radon_level": 0, "k_radon_level_last": 0,
           "k_radon_finish": 0}
    for R, P in ((hb, p01), (hb, p01), (wb, p23), (wb, p23)):
        G = min(32, P // 2)
        out["k_radon_first"] += 6 * hb * wb + 6 * (R + G - 1) * P
        n = G
        while 2 * n < P:
            out["k_radon_level"] += 6 * (R + n - 1) * P + 6 * (R + 2 * n - 1) * P
            n *= 2
        out["k_radon_level_last"] += 6 * (R + n - 1) * P
    return out


def timed(call, reps):
    """(what the last call returned, the ms of each of ``reps`` calls between HIP events), after one warm-up call: module load,
    first touch, the buffers a search allocates on its first call"""
    import torch
    out, ms = call(), []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def peel_mode(name, r, call, a, lines_round=None):
    """a peeling search's records and its keys of the result; lines_round: search_lines' ms per frame-round, the yardstick"""
    import numpy as np
    (recs, nl), ms = timed(call, a.reps)
    rounds = int(np.minimum(nl + 1, a.lines).sum())               # frame-rounds the call ran
    med = float(np.median(ms))
    out = {"ms_per_call": med, "ms_all": ms, "found": int(nl.sum()), "frame_rounds": rounds, "ms_per_frame_round": med / rounds}
    if lines_round is not None:
        out["over_lines_per_frame_round"] = med / rounds / lines_round
    return recs, {**{"%s_%s" % (name, k): v for k, v in out.items()}, "bytes_with_" + name: r.dims()[2]}


def child(a):
    import numpy as np
    import torch
    from lfd_amd import _native
    h, w = SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randn((a.frames, h, w), generator=g, device="cuda", dtype=torch.float32) * 0.025
    if a.lines:
        frames[::2, h // 3, :] += 0.02                       # a faint row: every second frame peels at least once
    for b in ((a.bin,) if a.bin else (1, 2, 4)):
        with _native.Context(0, h, w, 2) as ctx, _native.Radon(ctx, SHAPE, max_frames=a.max_frames, bin=b) as r:
            rec, ms = timed(lambda: r.search(frames), a.reps)
            med = float(np.median(ms))
            lines = {}
            if a.lines:
                _, lines = peel_mode("lines", r, lambda: r.search_lines(frames, max_lines=a.lines), a)
                lines.update({"lines_max": a.lines, "plain_ms_per_call": med})
            if a.short:
                srecs, more = peel_mode("short", r, lambda: r.search_short(frames, max_lines=a.lines), a, lines["lines_ms_per_frame_round"])
                lines.update(more, short_levels=sorted({int(v) for v in srecs["level"][srecs["status"] == 0]}))
            if a.wide:
                wrecs, more = peel_mode("wide", r, lambda: r.search_wide(frames, max_lines=a.lines), a, lines["lines_ms_per_frame_round"])
                lines.update(more, wide_widths=sorted({int(v) for v in wrecs["width"][wrecs["status"] == 0]}))
            kb = kernel_bytes(SHAPE, b)
            total = float(sum(kb.values())) * a.frames
            print("RESULT " + json.dumps({
                "bin": b, "frames": a.frames, "max_frames": a.max_frames, "shape": list(SHAPE), "P": [r.p01, r.p23],
                "device_bytes_per_inflight_frame": r.bytes // a.max_frames, "ms_per_call": med, "ms_all": ms,
                "ms_per_frame": med / a.frames, "bytes_per_frame_by_kernel": kb, "bytes_per_call": total,
                "ms_floor_at_4.8_TBps": total / COPY_RATE * 1e3, "x_the_floor": med / (total / COPY_RATE * 1e3),
                "snr_max": float(rec["snr"].max()), "found": int(rec["found"].sum()), **lines}), flush=True)


def run_child(extra, timeout_s, prefix=()):
    cmd = ["timeout", "-k", "10", str(timeout_s), *prefix, sys.executable, os.path.abspath(__file__), "--child", *extra]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("radon_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    return [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--max-frames", type=int, default=16)
    ap.add_argument("--bin", type=int, default=0)
    ap.add_argument("--lines", type=int, default=0)
    ap.add_argument("--short", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radon_probe.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if (a.short or a.wide) and not a.lines:
        a.lines = 4
    if a.child:
        child(a)
        return
    common = ["--frames", str(a.frames), "--max-frames", str(a.max_frames), "--lines", str(a.lines)] + (["--short"] if a.short else []) + \
        (["--wide"] if a.wide else [])
    doc = {"tool": "tools/radon_probe.py", "copy_rate_TBps": COPY_RATE / 1e12,
           "runs": run_child(common + ["--reps", str(a.reps)], 500)}
    for r in doc["runs"]:
        print({k: r[k] for k in ("bin", "ms_per_call", "ms_floor_at_4.8_TBps", "x_the_floor", "lines_ms_per_call",
                                 "lines_ms_per_frame_round", "lines_found", "short_ms_per_call",
                                 "short_ms_per_frame_round", "short_found", "short_over_lines_per_frame_round", "wide_ms_per_call",
                                 "wide_ms_per_frame_round", "wide_found", "wide_over_lines_per_frame_round") if k in r}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.trace:
        # the traced child runs the same searches as the timed one; the files are named after --out, so a --wide run written
        # to radon_probe_wide.json leaves the plain search's radon_probe_kernel_stats_bin<b>.csv alone
        stem = os.path.splitext(os.path.basename(a.out))[0]
        modes = ["--lines", str(a.lines)] + (["--short"] if a.short else []) + (["--wide"] if a.wide else [])
        for b in (1, 2, 4):
            tmp = tempfile.mkdtemp(prefix="radon_probe_")
            try:
                run_child(["--frames", "32", "--max-frames", str(a.max_frames), "--reps", "1", "--bin", str(b)] + modes, 300,
                          ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "radon", "--output-format", "csv", "--"])
                found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                if not found:
                    raise SystemExit("radon_probe: rocprofv3 wrote no kernel_stats.csv")
                shutil.copy(found[0], os.path.join(os.path.dirname(os.path.abspath(a.out)), "%s_kernel_stats_bin%d.csv" % (stem, b)))
            finally:
                shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
