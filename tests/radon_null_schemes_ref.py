"""numpy restatement of the null schemes and the peel rounds (include/lfdmi.h: faint-trail search, null peaks, steps 21 - 22) on
top of radon_null_ref: the null frame X' of each scheme with numpy integers, the peel through radon_lines_ref's and
radon_wide_ref's own blotting, and the null records as the existing restatements of the searches on the result.  Nothing here is
new floating-point arithmetic, so the device has to reproduce these records bit for bit."""
import numpy as np

import radon_lines_ref as L
import radon_null_ref as NR
import radon_ref as R
import radon_short_ref as S
import radon_wide_ref as W

SCHEMES = ("scramble", "signflip", "rowshift", "colshift")
MAX_LINES = 8


def u_of(i, k):
    """step 18's u for the indices ``i`` (uint32 array) and key k"""
    i = np.asarray(i, np.uint32)
    return NR.fmix32(NR.fmix32(i * np.uint32(0x9E3779B1) + np.uint32(k & 0xFFFFFFFF)) ^ np.uint32(k >> 32))


def offsets(count, k, size):
    """step 21: o(0 .. count-1) = (u * size) >> 32, each below ``size``"""
    u = u_of(np.arange(count, dtype=np.uint32), k)
    return ((u.astype(np.uint64) * np.uint64(size)) >> np.uint64(32)).astype(np.int64)


def null_frame(frame, seed, r, scheme):
    """step 21: X' of one (h, w) frame of a 4-byte dtype of either byte order, in that dtype"""
    if scheme == "scramble":
        return NR.scramble(frame, seed, r)
    x = np.ascontiguousarray(frame)
    h, w = x.shape
    k = NR.key(seed, r)
    if scheme == "signflip":
        # the value's bits, whatever the storage order; the result goes back into that order
        bits = x.astype(x.dtype.newbyteorder("<")).view(np.uint32).reshape(-1)
        flip = u_of(np.arange(bits.size, dtype=np.uint32), k) & np.uint32(0x80000000)
        return (bits ^ flip).view("<f4").reshape(h, w).astype(x.dtype)
    bits = x.view(np.uint32)
    if scheme == "rowshift":
        o = offsets(h, k, w)
        assert o.size == h and int(o.max()) < w
        cols = (np.arange(w)[None, :] + o[:, None]) % w
        return np.take_along_axis(bits, cols, axis=1).view(x.dtype)
    if scheme == "colshift":
        o = offsets(w, k, h)
        assert o.size == w and int(o.max()) < h
        rows = (np.arange(h)[:, None] + o[None, :]) % h
        return np.take_along_axis(bits, rows, axis=0).view(x.dtype)
    raise ValueError("scheme: one of %s" % (SCHEMES,))


def check_peel(peel, scheme, shape, b):
    """step 22's rules for one frame's peel records (dicts or records with q, y0, s, width)"""
    if len(peel) > MAX_LINES:
        raise ValueError("n_peel: 0 .. %d" % MAX_LINES)
    if len(peel) and scheme != "signflip":
        raise ValueError("peel records need the signflip scheme")
    hb, wb = -(-shape[0] // b), -(-shape[1] // b)
    for rec in peel:
        k = int(rec["width"])
        if k == 0:
            continue
        if k < 1 or k > 16 or k & (k - 1) or not 0 <= int(rec["q"]) <= 3:
            raise ValueError("width: 0 or a power of two up to 16; q: 0 .. 3")
        C, Rr = (wb, hb) if int(rec["q"]) < 2 else (hb, wb)
        P = R.pow2_at_least(C)
        if not 0 <= int(rec["s"]) <= P - 1 or not -(P - 1) <= int(rec["y0"]) <= Rr - 1:
            raise ValueError("s: 0 .. P-1; y0: -(P-1) .. R-1")


def peeled(V, M, peel, hw):
    """step 22: (V', M') without the bands of the records with width >= 1, through the searches' own blotting"""
    for rec in peel:
        k = int(rec["width"])
        line = {"q": int(rec["q"]), "y0": int(rec["y0"]), "s": int(rec["s"]), "width": k}
        if k == 1:
            V, M = L.peel(V, M, line, hw)
        elif k > 1:
            V, M = W.peel(V, M, line, hw)
    return V, M


def record_vm(V, M, sigma, shape, kind, p, kp):
    """step 20 on a prepared (V, M): record 0 of the kind's search, a found short or wide record with its segment"""
    b = int(p["bin"])
    if kind == "lines":
        rec = L.search_vm(V, M, sigma, shape, p)
        return {k: rec[k] for k in NR.PLAIN_FIELDS}
    if kind == "short":
        q = dict(S.SHORT_DEFAULTS, **kp)
        rec = S.search_short_vm(V, M, sigma, shape, b, int(q["min_strip"]), q["short_threshold"])
        if rec["status"] == R.OK and rec["found"]:
            rec.update(L.extent(V, M, rec, sigma, q["min_seg"], shape, b))
        return rec
    if kind == "wide":
        q = dict(W.WIDE_DEFAULTS, **kp)
        rec = W.search_wide_vm(V, M, sigma, shape, b, p["min_len"], int(q["max_width"]), q["wide_threshold"])
        if rec["status"] == R.OK and rec["found"]:
            rec.update(W.extent(V, M, rec, sigma, q["min_seg"], shape, b))
        return rec
    raise ValueError("kind: 'lines', 'short' or 'wide'")


def null_record(frame, seed, r, kind="lines", sigma=R.DEFAULT_SIGMA, scheme="scramble", peel=(), **params):
    """steps 20 - 22: the null record (a dict) of realisation r of one frame; ``params``: the handle's and the kind's
    (``peel_halfwidth`` among them: the lines kind takes the fields of the several-lines search)"""
    p = dict(R.DEFAULTS)
    kp = {k: params[k] for k in params if k not in p}
    p.update({k: params[k] for k in params if k in p})
    b = int(p["bin"])
    shape = np.asarray(frame).shape
    check_peel(peel, scheme, shape, b)
    x = null_frame(frame, seed, r, scheme).astype(np.float32)          # (a '>f4' frame: the values, which is step 1's swap)
    V, M = R.prepare(x, b, p["clip"])
    hw = -(-int(kp.get("peel_halfwidth", 8)) // b)
    V, M = peeled(V, M, peel, hw)
    return record_vm(V, M, np.float32(sigma), shape, kind, p, kp)


def null_records(frames, K, kind="lines", sigma=None, seeds=None, scheme="scramble", peel=None, **params):
    """[n][K] null records of (n, h, w) frames; peel: None or [n][n_peel] records"""
    n = len(frames)
    sg = np.broadcast_to(np.asarray(R.DEFAULT_SIGMA if sigma is None else sigma, np.float32), (n,))
    sd = range(n) if seeds is None else [int(v) for v in seeds]
    return [[null_record(frames[f], sd[f], r, kind, sg[f], scheme, () if peel is None else peel[f], **params) for r in range(K)]
            for f in range(n)]


def null_snr(frames, K, kind="lines", sigma=None, seeds=None, scheme="scramble", peel=None, **params):
    """float32 [n, K]: the null peaks"""
    return np.array([[rec["snr"] for rec in row] for row in null_records(frames, K, kind, sigma, seeds, scheme, peel, **params)],
                    np.float32)


def peel_of(lines, n_lines, upto):
    """[n][upto] peel records (dicts) from the records of a search: the frame's first min(n_lines, upto) lines, width 1 where the
    record has none, and width 0 in the places after them"""
    out = []
    for f in range(len(lines)):
        row = []
        for k in range(upto):
            rec = lines[f][k] if k < len(lines[f]) else None
            if rec is not None and k < int(n_lines[f]):
                names = rec.dtype.names if hasattr(rec, "dtype") else rec
                row.append({"q": int(rec["q"]), "y0": int(rec["y0"]), "s": int(rec["s"]), "width": int(rec["width"]) if "width" in names else 1})
            else:
                row.append({"q": 0, "y0": 0, "s": 0, "width": 0})
        out.append(row)
    return out


def null_rounds(frames, lines, n_lines, K, kind="lines", sigma=None, seeds=None, **params):
    """float32 [n, max_lines, K]: round k is the signflip null with the frame's lines 0 .. k-1 peeled; NaN where the frame never
    ran round k (round k ran iff k <= n_lines)"""
    n, max_lines = len(frames), len(lines[0])
    out = np.full((n, max_lines, K), np.nan, np.float32)
    for k in range(max_lines):
        ran = [f for f in range(n) if k <= int(n_lines[f])]
        if not ran:
            break
        pl = peel_of([lines[f] for f in ran], [n_lines[f] for f in ran], k)
        sd = None if seeds is None else [seeds[f] for f in ran]
        sg = None if sigma is None else np.broadcast_to(np.asarray(sigma, np.float32), (n,))[ran]
        if seeds is None:
            sd = ran                                                    # seeds = None: frame f has seed f, wherever it sits in the call
        out[ran, k] = null_snr([frames[f] for f in ran], K, kind, sg, sd, "signflip", pl if k else None, **params)
    return out
