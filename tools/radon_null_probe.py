"""Times lfdmi_radon_null on 256 device-resident SDSS-size noise frames (bin 2, kind "lines", K = 8) beside K times one
lfdmi_radon_search of the same frames in the same run: the null should cost about K searches, and what it costs beyond them is
k_radon_prep_null's gather against k_radon_prep's streaming read.  ms per call as the median and range of repeated calls between
HIP events.  Also records the first full-frame figures of the false-alarm ceiling: the largest unscrambled peak and the largest
null peak over those frames for every kind, and the same for ``synth.make_frame`` frames after remove_stars (each of which
carries its recipe's streak, so their unscrambled peak is a trail's, not a ceiling).  Writes profiles/radon_null_probe.txt.

``--scheme a,b,..`` (or ``all``): the same for lfdmi_radon_null_scheme under each named scheme in one run -- ms per call against K
searches and against the scramble, and both sets of ceilings per scheme; ``--rounds R``: also the sign-flip call with R peel
records per frame (what a round R of ``radon.null_rounds`` costs).  Then the default output is
profiles/radon_null_schemes_probe.txt.

    python tools/radon_null_probe.py [--reps 20] [--frames 256] [--max-frames 16] [--K 8] [--synth 16] [--out FILE]
                                     [--scheme all] [--rounds R]

The GPU step is a child process under its own `timeout`.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (1489, 2048)
KINDS = ("lines", "short", "wide")


def timed(call, reps):
    """the ms of each of ``reps`` calls between HIP events, after one warm-up call"""
    import torch
    call()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    import numpy as np
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def ceilings(r, frames, K, scheme="scramble"):
    """per kind: the largest unscrambled peak and the largest null peak over ``frames``"""
    out = {}
    for kind in KINDS:
        if kind == "lines":
            peak = r.search(frames)["snr"]
        else:
            peak = getattr(r, "search_" + kind)(frames, max_lines=1)[0][:, 0]["snr"]
        null = r.null(frames, K=K, kind=kind, scheme=scheme)["snr"]
        out[kind] = {"unscrambled_max": float(peak.max()), "null_max": float(null.max()), "null_min": float(null.min()),
                     "frames_above_own_null_max": int((peak > null.max(axis=1)).sum()), "frames": int(len(peak)), "K": K}
    return out


def child(a):
    import numpy as np
    import torch
    from lfd_amd import _native, synth
    from lfd_amd.detecttrails import default_params
    h, w = SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randn((a.frames, h, w), generator=g, device="cuda", dtype=torch.float32) * 0.025
    with _native.Context(0, h, w, 2) as ctx, _native.Radon(ctx, SHAPE, max_frames=a.max_frames, bin=2) as r:
        search = stats(timed(lambda: r.search(frames), a.reps))
        null = stats(timed(lambda: r.null(frames, K=a.K), a.reps))
        doc = {"frames": a.frames, "max_frames": a.max_frames, "K": a.K, "reps": a.reps, "bin": 2, "search_ms": search, "null_ms": null,
               "ratio_null_over_K_searches": null["median"] / (a.K * search["median"]),
               "extra_ms_per_call": null["median"] - a.K * search["median"],
               "extra_us_per_realisation": 1e3 * (null["median"] - a.K * search["median"]) / (a.K * a.frames),
               "noise": ceilings(r, frames, a.K)}
        schemes = list(_native.RADON_NULL_SCHEMES) if a.scheme == "all" else [s for s in a.scheme.split(",") if s]
        if schemes:
            doc["schemes"] = {}
            for sch in schemes:
                ms = stats(timed(lambda: r.null(frames, K=a.K, scheme=sch), a.reps))
                doc["schemes"][sch] = {"ms": ms, "ratio_over_K_searches": ms["median"] / (a.K * search["median"]),
                                       "ratio_over_scramble": ms["median"] / null["median"], "noise": ceilings(r, frames, a.K, sch)}
        if a.rounds:
            peel = np.zeros((a.frames, a.rounds), _native.RADON_PEEL_DTYPE)
            for k in range(a.rounds):                     # lines of orientation 0 spread over the frame, one cell wide
                peel[:, k] = (0, 50 + 90 * k, 100 + 37 * k, 1)
            ms = stats(timed(lambda: r.null(frames, K=a.K, scheme="signflip", peel=peel), a.reps))
            doc["rounds"] = {"n_peel": a.rounds, "ms": ms, "ratio_over_K_searches": ms["median"] / (a.K * search["median"])}
        if a.synth:
            _, _, prs = default_params()
            imgs, cats = zip(*(synth.make_frame(k)[:2] for k in range(a.synth)))
            sf = np.ascontiguousarray(np.stack(imgs), np.float32)
            rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
            ctx.remove_stars(sf, synth.pack_catalogs(list(cats)), rs)
            dev = torch.from_numpy(sf).cuda()
            doc["synth_after_remove_stars"] = ceilings(r, dev, a.K)
            for sch in schemes:
                doc["schemes"][sch]["synth_after_remove_stars"] = ceilings(r, dev, a.K, sch)
    print("RESULT " + json.dumps(doc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--max-frames", type=int, default=16)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--synth", type=int, default=16)
    ap.add_argument("--scheme", default="", help="schemes to time and measure beside the scramble, comma separated, or 'all'")
    ap.add_argument("--rounds", type=int, default=0, metavar="R", help="also time the sign-flip call with R peel records per frame")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "radon_null_schemes_probe.txt" if a.scheme or a.rounds else "radon_null_probe.txt")
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames",
           str(a.frames), "--max-frames", str(a.max_frames), "--K", str(a.K), "--synth", str(a.synth), "--scheme", a.scheme, "--rounds", str(a.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("radon_null_probe: %s ended with status %d" % (" ".join(cmd), p.returncode))
    doc = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0]
    lines = ["tools/radon_null_probe.py: %d device-resident %d x %d noise frames, bin 2, kind lines, K = %d, %d calls, max_frames %d"
             % (doc["frames"], *SHAPE, doc["K"], doc["reps"], doc["max_frames"]),
             "Radon.search   ms per call: median %.2f (range %.2f .. %.2f)" % tuple(doc["search_ms"][k] for k in ("median", "min", "max")),
             "Radon.null     ms per call: median %.2f (range %.2f .. %.2f)" % tuple(doc["null_ms"][k] for k in ("median", "min", "max")),
             "null / (K searches): %.3f; beyond K searches: %.2f ms per call, %.2f us per realisation (k_radon_prep_null's gather "
             "against k_radon_prep's read; what bounds it: unmeasured)" % (doc["ratio_null_over_K_searches"], doc["extra_ms_per_call"],
                                                                        doc["extra_us_per_realisation"])]
    for name in ("noise", "synth_after_remove_stars"):
        for kind, c in doc.get(name, {}).items():
            lines.append("%s, %s: %d frames, K = %d: largest unscrambled peak %.3f, null peaks %.3f .. %.3f, frames above their own "
                         "null maximum: %d" % (name, kind, c["frames"], c["K"], c["unscrambled_max"], c["null_min"], c["null_max"],
                                               c["frames_above_own_null_max"]))
    for sch, d in doc.get("schemes", {}).items():
        lines.append("scheme %s: ms per call: median %.2f (range %.2f .. %.2f); / (K searches): %.3f; / scramble in this run: %.3f "
                     "(what bounds its prep kernel: unmeasured)" % (sch, d["ms"]["median"], d["ms"]["min"], d["ms"]["max"],
                                                                    d["ratio_over_K_searches"], d["ratio_over_scramble"]))
        for name in ("noise", "synth_after_remove_stars"):
            for kind, c in d.get(name, {}).items():
                lines.append("scheme %s: %s, %s: %d frames, K = %d: largest unscrambled peak %.3f, null peaks %.3f .. %.3f, frames above "
                             "their own null maximum: %d" % (sch, name, kind, c["frames"], c["K"], c["unscrambled_max"], c["null_min"],
                                                             c["null_max"], c["frames_above_own_null_max"]))
    if "rounds" in doc:
        d = doc["rounds"]
        lines.append("signflip with %d peel records per frame: ms per call: median %.2f (range %.2f .. %.2f); / (K searches): %.3f"
                     % (d["n_peel"], d["ms"]["median"], d["ms"]["min"], d["ms"]["max"], d["ratio_over_K_searches"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
