"""What detect_rounds costs beside plain detect: 256 device-resident synthetic SDSS frames, a second streak injected into every
eighth, the median, min and max of 20 calls of each in one run.  Writes profiles/rounds_probe.txt.

    python tools/rounds_probe.py [--frames 256] [--calls 20] [--out profiles/rounds_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rounds_probe.txt"))
    a = ap.parse_args()
    import torch
    from lfd_amd import _native, recovery, synth
    from lfd_amd.detecttrails import default_params
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    n, (h, w) = a.frames, synth.SDSS_SHAPE
    host, cats = synth.make_frames(0, n)
    cat = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in synth.pack_catalogs(cats).items()}
    base = torch.from_numpy(host).cuda()
    with _native.Context(0, h, w, n) as ctx:
        # a second streak in every eighth frame: a bright Gaussian trail across the frame, 60 degrees from the horizontal
        second = list(range(0, n, 8))
        tr = np.zeros(len(second), _native.INJECT_DTYPE)
        tr["frame"], tr["rho"], tr["theta"], tr["t0"], tr["t1"], tr["amplitude"] = second, 900.0, np.deg2rad(30.0), -np.inf, np.inf, 5.0
        table = np.exp(-0.5 * (np.arange(-32, 33) * 0.25 / 2.0) ** 2).astype(np.float32)
        ctx.inject_trails(base, tr, table, 0.25)
        work = torch.empty_like(base)

        def timed(call):
            out = []
            for _ in range(a.calls + 2):
                work.copy_(base)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = call()
                out.append(1e3 * (time.perf_counter() - t0))
            return np.array(out[2:]), res
        t_plain, rec = timed(lambda: ctx.detect_batch(work, pb, pd, cat, rs))
        t_rounds, (recs, nf, dup) = timed(lambda: ctx.detect_rounds(work, pb, pd, cat, rs, max_trails=4))
    assert recs[:, 0].tobytes() == rec.tobytes()
    per_round = [int((nf > k).sum()) for k in range(4)]
    lines = [
        "detect_rounds(max_trails=4, half=10, dup_dist=20) beside detect: %d device-resident synthetic SDSS frames (%d x %d)," % (n, h, w),
        "a second streak injected into every eighth; %d calls each after 2 warm-up calls, wall time of the call in ms" % a.calls,
        "",
        "call            median      min      max",
        "detect        %8.2f %8.2f %8.2f" % (np.median(t_plain), t_plain.min(), t_plain.max()),
        "detect_rounds %8.2f %8.2f %8.2f" % (np.median(t_rounds), t_rounds.min(), t_rounds.max()),
        "",
        "frames found by round 0: %d; frames that found a line in rounds 0..3: %s" % (int((rec["found"] != 0).sum()), per_round),
        "frames with a second streak: %d; of those with n_found >= 2: %d; records labelled dup_of >= 0: %d" % (
            len(second), int((nf[second] >= 2).sum()), int((dup >= 0).sum())),
        "",
        "Not measured: the gather kernel's own time (no kernel trace was taken), the pool allocations' and the catalogue",
        "compaction's share of a round, host or pinned frames, other max_trails or half, more than one run of this probe.",
    ]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
