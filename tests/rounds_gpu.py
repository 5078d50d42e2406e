"""What the detection rounds' GPU tests share: the composition of existing public calls that defines a later round
(``detect_batch``, ``mask_trails(fill="zero")`` with cap = +inf on a copy, ``detect_batch`` again), and the default parameters."""
import numpy as np

from lfd_amd import _native, masks, synth
from lfd_amd.detecttrails import default_params


def params():
    pb, pd, prs = default_params()
    return pb, pd, _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"}), prs


def found(r):
    return int(r["status"]) == 0 and int(r["found"]) != 0


def dup_of(recs, k, dup_dist):
    import rounds_ref as RR
    return RR.dup_of(recs, k, dup_dist)


def composed(ctx, frames, cats, max_trails=4, half=10.0, dup_dist=20.0):
    """native float32 host frames [n, h, w] (not modified) -> (records, n_found, dup_of) by the loop of public calls"""
    pb, pd, rs, _ = params()
    n = len(frames)
    rec = np.zeros((n, max_trails), _native.RESULT_DTYPE)
    nf = np.zeros(n, np.int32)
    dup = np.full((n, max_trails), -1, np.int32)
    alive = list(range(n))
    for k in range(max_trails):
        if not alive:
            break
        work = np.ascontiguousarray(frames[alive]).copy()
        rows = [(s, rec[i, j]["x1"], rec[i, j]["y1"], rec[i, j]["x2"], rec[i, j]["y2"], half) for s, i in enumerate(alive) for j in range(k)]
        if rows:
            ctx.mask_trails(work, masks.segments(rows, cap=np.inf), mask=False, fill="zero")
        cat = synth.pack_catalogs([cats[i] for i in alive]) if cats is not None else None
        out = ctx.detect_batch(work, pb, pd, cat, rs if cat is not None else None)
        nxt = []
        for s, i in enumerate(alive):
            rec[i, k] = out[s]
            dup[i, k] = dup_of(rec[i], k, dup_dist)
            if found(out[s]):
                nf[i] = k + 1
                nxt.append(i)
        alive = nxt
    return rec, nf, dup


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
