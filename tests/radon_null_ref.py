"""numpy restatement of the null peaks (include/lfdmi.h: faint-trail search, null peaks, steps 17 - 20): the key and the source
pixel in numpy integers, the scrambled frame as a gather of 32-bit patterns, and the null records as record 0 of the existing
restatements (tests/radon_ref.py, radon_short_ref.py, radon_wide_ref.py) of that frame.  Nothing here is new floating-point
arithmetic, so the device has to reproduce these records bit for bit."""
import numpy as np

import radon_ref as R
import radon_short_ref as S
import radon_wide_ref as W

GOLD64 = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
KINDS = ("lines", "short", "wide")
NULL_MAX = 64
PLAIN_FIELDS = ("status", "found", "q", "y0", "s", "n_pix", "sum", "snr", "x1", "y1", "x2", "y2", "rho", "theta")


def splitmix64(x):
    """the usual finaliser on a Python integer, modulo 2^64"""
    x = (x + GOLD64) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def key(seed, r):
    """step 17: the key of realisation r of a frame with ``seed``"""
    return splitmix64((int(seed) + GOLD64 * (int(r) + 1)) & MASK64)


def fmix32(h):
    """murmur3's finaliser on a uint32 array (wrapping arithmetic)"""
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def source(i, k, n):
    """step 18: j for the buffer indices ``i`` (uint32 array), key k and N = n pixels"""
    if not 0 < n < 1 << 32:
        raise ValueError("N = H W must be below 2^32")
    i = np.asarray(i, np.uint32)
    a = fmix32(i * np.uint32(0x9E3779B1) + np.uint32(k & 0xFFFFFFFF))
    u = fmix32(a ^ np.uint32(k >> 32))
    return ((u.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.uint32)


def scramble(frame, seed, r):
    """step 19: X' of one frame (any 4-byte dtype, either byte order: the patterns move as they are stored)"""
    x = np.ascontiguousarray(frame)
    bits = x.view(np.uint32).reshape(-1)
    j = source(np.arange(bits.size, dtype=np.uint32), key(seed, r), bits.size)
    assert int(j.max()) < bits.size
    return bits[j].view(x.dtype).reshape(x.shape)


def null_record(frame, seed, r, kind="lines", sigma=R.DEFAULT_SIGMA, **params):
    """step 20: the null record (as a dict) of realisation r; ``params``: the handle's and the kind's"""
    x = scramble(frame, seed, r).astype(np.float32)                    # (a '>f4' frame: the values, which is step 1's swap)
    if kind == "lines":
        return R.search(x, sigma, **params)
    params = dict(params, max_lines=1)
    if kind == "short":
        return S.search_short(x, sigma, **params)[0][0]
    if kind == "wide":
        return W.search_wide(x, sigma, **params)[0][0]
    raise ValueError("kind: 'lines', 'short' or 'wide'")


def null_records(frames, K, kind="lines", sigma=None, seeds=None, **params):
    """[n][K] null records of (n, h, w) frames; sigma: None, a number or n values; seeds: None (frame f has seed f) or n"""
    n = len(frames)
    sg = np.broadcast_to(np.asarray(R.DEFAULT_SIGMA if sigma is None else sigma, np.float32), (n,))
    sd = range(n) if seeds is None else [int(v) for v in seeds]
    return [[null_record(frames[f], sd[f], r, kind, sg[f], **params) for r in range(K)] for f in range(n)]


def null_snr(frames, K, kind="lines", sigma=None, seeds=None, **params):
    """float32 [n, K]: the null peaks"""
    return np.array([[rec["snr"] for rec in row] for row in null_records(frames, K, kind, sigma, seeds, **params)], np.float32)
