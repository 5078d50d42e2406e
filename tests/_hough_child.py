"""Child of tests/test_gpu_hough_shapes.py: LFDMI_VOTE_THREADS, LFDMI_VOTE_WGS and LFDMI_PEAK_ROWS are read once per process, so
they are set by the parent for a fresh interpreter.  argv[1]: an .npz with, per case name, the oracle's accumulator
("acc_<name>") and line list ("lines_<name>", "n_<name>").  Exit status 0: every case equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import hough_cases as H
    from lfd_amd import _native
    assert os.environ["LFDMI_VOTE_THREADS"] == "64" and os.environ["LFDMI_VOTE_WGS"] == "1" and os.environ["LFDMI_PEAK_ROWS"] == "8"
    ref = np.load(sys.argv[1])
    names = sorted(k[4:] for k in ref.files if k.startswith("acc_"))
    bad = []
    for name in names:
        c = H.BY_NAME[name]
        img = H.frame(c)
        h, w = H.ctx_dims(c)
        with _native.Context(0, h, w, 1, caps="worst") as ctx:
            acc = ctx.hough_accum(img, c["rho"], c["theta"])
            lines, n = ctx.hough_lines(img, c["rho"], c["theta"], threshold=1)
        ok = np.array_equal(acc, ref["acc_" + name]) and n == int(ref["n_" + name]) and np.array_equal(lines, ref["lines_" + name])
        print(name, "ok" if ok else "DIFFERS", flush=True)
        if not ok:
            bad.append(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
