"""Cost of the defocus bank and fit (include/lfdmi.h: defocus fit) with the default grid.  Prints one JSON line: the bank build
in ms, the whole lfdmi_fit_defocus call in ms for n = 256, 1024 and 4096 trails with its end-to-end rate (n x columns x
(2K+1) x 2 / t, in TFLOP/s and as a fraction of the 155 TF/s measured FP32 matrix peak; the call includes the host's
centring, the copies, k_def_pick and the read-back), and for the record the numpy restatement's scoring of a few trails
against the same columns.  The scoring kernel alone: run this under rocprofv3 --kernel-trace --stats (k_def_gemm's
average per call; profiles/defocus_probe_kernel_stats.csv).

    python tools/defocus_probe.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP32_MATRIX_PEAK_TF = 155.0


def profiles(n, seed=0):
    """n noisy model profiles (heights 70 .. 250 km, seeing 1.0 .. 1.8) as measure_trails records + rows"""
    import defocus_ref as R
    from lfd_amd import _native
    g = R.Grid()
    rng = np.random.default_rng(seed)
    base = []
    for k in range(16):
        m = R.model(g, float(rng.uniform(70, 250)), 0.0, float(rng.uniform(1.0, 1.8)))
        base.append(m["samp"][g.S:g.S + 2 * g.K + 1] / m["samp"].max())
    base = np.array(base)
    rows = base[rng.integers(0, len(base), n)] * 2.0 + rng.normal(0, 0.05, (n, base.shape[1]))
    tr = np.zeros(n, _native.TRAIL_DTYPE)
    tr["status"] = _native.TRAIL_OK
    tr["noise"] = 0.05
    return tr, rows.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from lfd_amd import _native, defocus
    out = {}
    with _native.Context(0, 64, 64, 1) as ctx:
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            b = defocus.DefocusBank(ctx)
            ts.append((time.perf_counter() - t0) * 1e3)
            if _ < 1:
                b.close()
        out["bank_build_ms"] = round(min(ts), 2)
        out["columns"] = int(b.n_columns)
        out["valid_models"] = int(b.grid["valid"].sum())
        out["models"] = int(b.n_models)
        out["bins"] = int(b.n_bins)
        fits = {}
        for n in (256, 1024, 4096):
            tr, rows = profiles(n)
            ctx.fit_defocus(b, tr[:8], rows[:8])         # the workspace
            tt = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.fit_defocus(b, tr, rows)
                tt.append(time.perf_counter() - t0)
            t = float(np.median(tt))
            tf = n * b.n_columns * b.n_bins * 2 / t / 1e12
            fits[str(n)] = {"call_ms": round(t * 1e3, 2), "end_to_end_tflops": round(tf, 2),
                            "end_to_end_of_fp32_peak": round(tf / FP32_MATRIX_PEAK_TF, 3)}
        out["fit"] = fits
        # the numpy restatement's scoring of a few trails against the same columns (double, in chunks)
        tr, rows = profiles(4, seed=1)
        cols = b.columns()
        t0 = time.perf_counter()
        vt = rows.astype(np.float64) - rows.astype(np.float64).mean(axis=1, keepdims=True)
        best = np.full(len(vt), -np.inf)
        for c0 in range(0, len(cols), 65536):
            c = cols[c0:c0 + 65536].astype(np.float64) @ vt.T
            best = np.maximum(best, c.max(axis=0))
        out["numpy_4_trails_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
