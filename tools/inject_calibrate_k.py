"""Sets recovery.K_MATCH on the CPU, where the chain runs exactly: frames of synth.make_frame without a streak of their own, one
full-length Gaussian trail (sigma 2 px) of peak synth.BRIGHT_PEAK per frame from recovery.draw_trails, injected with the numpy
restatement (tests/inject_ref.py), detected with the oracle.  Prints, for k = 1, 1.5, 2, 3, how many of the detected trails
match, and every detected trail's d_rho / d_theta.

    python tools/inject_calibrate_k.py [--frames 32] [--first 0] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import inject_ref
    from lfd_amd import inject, recovery, synth, _native
    from lfd_amd.detecttrails import default_params
    from oracle import lfd_oracle as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    pb, pd, prs = default_params()
    rs = O.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    table, step = inject.gaussian_table(2.0)
    table = inject.normalise_peak(table).astype(np.float32)
    plan = recovery.draw_trails(a.frames, synth.SDSS_SHAPE, a.seed, [synth.BRIGHT_PEAK])
    recs = np.zeros(a.frames, _native.RESULT_DTYPE)
    k, used = a.first, []
    while len(used) < a.frames:
        img, cat, truth = synth.make_frame(k)
        k += 1
        if truth["streak"] != "none":
            continue
        i = len(used)
        used.append(k - 1)
        tr = recovery.to_inject(plan[i:i + 1])
        tr["frame"] = 0
        inject_ref.inject(img[None], tr, table, step, 4)
        res = O.detect_frame(img, pb, pd, cat, rs)
        for key, v in res.items():
            recs[i][key] = v
    matched, d_rho, d_theta, length = recovery.match(recs, plan, pb, pd, k=1.0, shape=synth.SDSS_SHAPE)
    found = recs["found"] != 0
    print("frames", used)
    for i in range(a.frames):
        print("frame %4d theta %.4f rho %9.2f length %7.1f found %d d_rho %8.3f d_theta %9.5f" % (
            used[i], plan["theta"][i], plan["rho"][i], length[i], recs["found"][i], d_rho[i], d_theta[i]))
    print("detected %d of %d" % (found.sum(), a.frames))
    for kk in (1.0, 1.5, 2.0, 3.0):
        m = recovery.match(recs, plan, pb, pd, k=kk, shape=synth.SDSS_SHAPE)[0]
        print("k = %.1f: matched %d of the %d detected" % (kk, int(m[found].sum()), int(found.sum())))


if __name__ == "__main__":
    main()
