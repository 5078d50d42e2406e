"""Named frames for the sky normalisation (lfd_amd/csrc/sky/k_sky.h, sky.hip) and a plain restatement of the index arithmetic
of its kernels.

Noise frames reach whatever branch of the kernels they reach.  The cases here choose it: the number of bits the radix
selection still has to decide (``rem``) and the width of its last pass, the live count of a cell against area / 8, pixels on
the closed clip boundary, meshes of 1 to 289 cells, empty cells by their neighbours, and the column spans, row intervals and
16-byte / scalar paths of the apply kernel.  A case is ``Case(name, frames [n, h, w] float32, params, note)``; the name's
prefix is its family (``sel_``, ``cell_``, ``empty_``, ``clip_``, ``mesh_``, ``apply_``) and the seed of every random draw is
derived from the name.  ``BIG_ENDIAN`` names the cases that are also given to the device as '>f4'; ``MAX_FRAMES`` the ones
that need a handle of fewer slots than frames.

The second half restates what the kernels compute with their constants -- ``sky_key``, the kmin / rem / pass-width schedule
of ``sky_select``, the rounds of ``k_sky_cells``, the host's ``use_lds`` / ``vec_in`` / ``v4`` choices and the grid of
``k_sky_apply`` -- so that tests/test_sky_cases_model.py can prove on the CPU that every case sits on the seam it names;
tests/test_gpu_sky_seams.py runs them on the device against tests/sky_ref.py.
"""
import zlib
from typing import NamedTuple

import numpy as np

import sky_ref as S

F32 = np.float32
# constants of k_sky.h that the cases sit on
SKY_THREADS = 256
SKY_LDS_MAX = 16384
SKY_ROW_SPLIT = 4
FAMILIES = ("sel", "cell", "empty", "clip", "mesh", "apply")
REMS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32)
MAD_REMS = (0, 1, 9, 24, 30, 31)
LIVE_COUNTS = (1, 2, 3, 255, 256, 257)
CELLS = (17, 18, 50, 100, 127, 128, 129, 255, 256)


class Case(NamedTuple):
    name: str
    frames: np.ndarray
    params: dict
    note: str

    @property
    def family(self):
        return self.name.split("_")[0]


BIG_ENDIAN = set()
MAX_FRAMES = {}


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the kernels' index arithmetic ------------------------------------------------------------------------------------------

def f2k(v):
    """sky_key: float32 (not NaN) -> uint32, ascending keys = ascending values"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_of(x):
    return int(f2k(F32(x)).ravel()[0])


def k2f(k):
    """sky_unkey"""
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def valid_key(k):
    """keys of finite floats as the statistics see them (-0 never appears: it counts as +0)"""
    k = np.asarray(k, np.int64)
    return ((k >= 0x00800000) & (k <= 0x7FFFFFFE)) | ((k >= 0x80000000) & (k <= 0xFF7FFFFF))


def select_trace(keys):
    """sky_select on the live keys: the range reduction, then passes of min(8, rem) bits from the top.  -> dict with m, kmin,
    rem, widths, cands (keys still matching the prefix at each pass), distinct (occupied bins of each pass), key (the lower
    median), ties (keys equal to it)"""
    keys = np.asarray(keys, np.uint32).ravel()
    m = int(keys.size)
    if m == 0:
        return dict(m=0, rem=0, widths=[], cands=[], distinct=[], key=None, ties=0)
    kmin = int(keys.min())
    rem = rem0 = (int(keys.max()) - kmin).bit_length()
    d = keys.astype(np.int64) - kmin
    prefix, r = 0, (m - 1) >> 1
    widths, cands, distinct = [], [], []
    while rem > 0:
        wd = min(8, rem)
        shift = rem - wd
        live = d[(d >> rem) == (prefix >> rem)]
        hist = np.bincount((live >> shift) & ((1 << wd) - 1), minlength=256)
        cum = np.cumsum(hist)
        digit = int(np.searchsorted(cum, r, side="right"))
        r -= int(cum[digit] - hist[digit])
        widths.append(wd); cands.append(int(live.size)); distinct.append(int((hist > 0).sum()))
        prefix |= digit << shift
        rem = shift
    key = kmin + prefix
    return dict(m=m, kmin=kmin, rem=rem0, widths=widths, cands=cands, distinct=distinct, key=key, ties=int((keys == key).sum()))


def cell_trace(pix, k_clip=3.0, n_clip=3, closed=True):
    """k_sky_cells on one cell's pixels: per round the two selections' traces, the clip interval and the pixels on its ends.
    closed=False: the interval open, what a `>` / `<` in SkyCellSrc::value would compute.  -> dict(n0, b, s, rounds)"""
    pix = np.asarray(pix, F32).ravel()
    fin = pix[np.isfinite(pix)] + F32(0)
    fd = fin.astype(np.float64)
    lo, hi = -np.inf, np.inf
    rounds, med, mad = [], F32(0), F32(0)
    for t in range(n_clip + 1):
        keep = (fd >= lo) & (fd <= hi) if closed else (fd > lo) & (fd < hi)
        live = fin[keep]
        if live.size == 0:
            break
        t1 = select_trace(f2k(live))
        med = k2f(np.uint32(t1["key"]))[()]
        with np.errstate(over="ignore"):
            dev = np.abs(live - med)
        t2 = select_trace(dev.view(np.uint32))
        mad = np.uint32(t2["key"]).view(F32)[()]
        r = dict(med=med, mad=mad, sel_med=t1, sel_mad=t2, overflow=not np.isfinite(dev).all())
        if t < n_clip:
            d = float(k_clip) * 1.4826 * float(mad)
            lo, hi = max(lo, float(med) - d), min(hi, float(med) + d)
            r.update(lo=lo, hi=hi, on_edge=int(((fd == lo) | (fd == hi))[keep].sum()))
        rounds.append(r)
    return dict(n0=int(fin.size), b=F32(med), s=F32(1.4826 * float(mad)), rounds=rounds)


def host_paths(h, w, cell, src_off=0, dst_off=0):
    """lfdmi_sky_create / lfdmi_sky_normalize: where the cell copy lives and which loads are 16 bytes wide.  src_off / dst_off:
    floats between a 16-byte boundary and the first frame.  -> dict(use_lds, lds_px, vec_in, v4, span, spans)"""
    px = min(cell, h) * min(cell, w)
    use_lds = px <= SKY_LDS_MAX
    vec_in = w % 4 == 0 and cell % 4 == 0 and src_off % 4 == 0
    v4 = w % 4 == 0 and src_off % 4 == 0 and dst_off % 4 == 0
    span = SKY_THREADS * (4 if v4 else 1)
    return dict(use_lds=use_lds, lds_px=px if use_lds else 0, vec_in=vec_in, v4=v4, span=span, spans=-(-w // span))


def apply_grid(h, w, cell, v4=True):
    """k_sky_apply's grid: (column spans, columns of the last span, rstart, rows of every (interval, part))"""
    span = SKY_THREADS * (4 if v4 else 1)
    spans = -(-w // span)
    j, _, _, ny = S.axis_table(h, cell)
    rstart = [int(np.flatnonzero(j == k)[0]) for k in range(ny)] + [h]
    rows = [[len(range(rstart[k] + part, rstart[k + 1], SKY_ROW_SPLIT)) for part in range(SKY_ROW_SPLIT)] for k in range(ny)]
    return spans, w - (spans - 1) * span, rstart, rows


# ---- pixels -----------------------------------------------------------------------------------------------------------------

def rem_offsets(rem, rng, n=256, below=53, top=None):
    """n key offsets from a common minimum whose range has exactly `rem` significant bits and whose lower median is decided in
    the last radix pass: offset 0, the top offset, `below` - 1 decoys under and the rest over a cluster of 150 offsets that share
    every digit but the last and tie heavily on that one.  Some decoys differ from the cluster only in the lowest bit of the
    digit before."""
    if rem == 0:
        return np.zeros(n, np.int64)
    top = (1 << rem) - 1 if top is None else top
    assert top.bit_length() == rem
    lastw = rem - 8 * ((rem - 1) // 8)
    if rem <= 8:   # one pass: every offset is in the cluster
        digits = np.sort(rng.choice(1 << rem, size=min(1 << rem, 6), replace=False))
        digits[0], digits[-1] = 0, top
        out = np.concatenate([digits, rng.choice(digits, size=n - len(digits))])
        return rng.permutation(out).astype(np.int64)
    hi_bits = rem - lastw
    P = int(0.7 * (top >> lastw)) | 1
    digits = np.array([0, 1]) if lastw == 1 else rng.choice(1 << lastw, size=4, replace=False)
    cluster = (P << lastw) | np.concatenate([digits, rng.choice(digits, size=150 - len(digits))])
    n_above = n - 150 - below - 1
    lo_dec = rng.integers(1, P << lastw, size=below - 1)
    hi_dec = rng.integers((P + 1) << lastw, top, size=n_above)
    lo_dec[:8] = ((P ^ 1) << lastw) | rng.integers(0, 1 << lastw, size=8)            # P is odd: P ^ 1 is under it
    if hi_bits > 8:
        hi_dec[:8] = ((P + (1 << 8)) << lastw) | rng.integers(0, 1 << lastw, size=8)  # same but one digit higher up
        hi_dec[:8] = np.minimum(hi_dec[:8], top - 1)
    out = np.concatenate([[0], lo_dec, cluster, hi_dec, [top]])
    assert out.size == n
    return rng.permutation(out).astype(np.int64)


def keys_to_cell(keys, shape=(16, 16)):
    keys = np.asarray(keys, np.int64)
    assert valid_key(keys).all()
    return k2f(keys.astype(np.uint32)).reshape(1, *shape).copy()


def sky_frame(rng, h, w, cell, sigma=1.0, nan_frac=0.0):
    """noise on a strong plane with a pedestal of its own in every cell: tx, ty and all four corners matter at every pixel"""
    ny, nx = -(-h // cell), -(-w // cell)
    ped = rng.integers(0, 40, size=(ny, nx)).astype(F32)
    x = rng.normal(0.0, sigma, (h, w)).astype(F32) + F32(100)
    x += np.arange(w, dtype=F32)[None, :] * F32(0.5) + np.arange(h, dtype=F32)[:, None] * F32(0.25)
    x += np.repeat(np.repeat(ped, cell, 0), cell, 1)[:h, :w]
    if nan_frac:
        bad = rng.random((h, w)) < nan_frac
        x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), size=int(bad.sum()))
    return x.astype(F32)


def blank(x, cell, cells, keep=0, rng=None):
    """sets the listed (j, i) cells to NaN / +-Inf, leaving `keep` finite pixels in each"""
    for j, i in cells:
        v = x[j * cell:(j + 1) * cell, i * cell:(i + 1) * cell]
        flat = np.arange(v.size)
        if rng is not None:
            flat = rng.permutation(flat)
        kill = flat[keep:]
        fill = np.array([np.nan, np.inf, -np.inf], F32)[np.arange(kill.size) % 3]
        r, c = np.unravel_index(kill, v.shape)
        v[r, c] = fill
    return x


ONE_CELL = dict(cell=16, filter=1, mode=S.SUBTRACT, k_clip=3.0)
MODES = ((3, S.NORMALISE), (1, S.SUBTRACT), (3, S.SUBTRACT), (1, S.NORMALISE))


def find_k_clip():
    """(k_clip, K): the smallest integer K >= 2 with a double k_clip for which k_clip * 1.4826 == K exactly"""
    for K in range(2, 64):
        k = K / 1.4826
        for c in (k, np.nextafter(k, 0.0), np.nextafter(k, 100.0)):
            if float(c) * 1.4826 == float(K):
                return float(c), K
    raise AssertionError("no exact k_clip")


def _sel_cases():
    out = []
    for nc in (0, 1):
        p = dict(ONE_CELL, n_clip=nc)
        for rem in REMS:
            name = f"sel_rem_{rem}_c{nc}"
            rng = rng_of(f"sel_rem_{rem}")
            if rem == 32:      # -1e30 .. +1e30: the range of the keys fills all 32 bits
                kbase = key_of(-1e30)
                off = rem_offsets(32, rng, top=key_of(1e30) - kbase)
            elif rem == 31:    # -2 .. 2
                kbase, off = 0x40000000, rem_offsets(31, rng)
            else:              # upwards from 100.0
                kbase, off = key_of(100.0), rem_offsets(rem, rng)
            out.append(Case(name, keys_to_cell(kbase + off), p, f"first select: rem {rem}, the median decided in the last pass"))
        for rem in MAD_REMS:
            name = f"sel_mad_{rem}_c{nc}"
            rng = rng_of(f"sel_mad_{rem}")
            if rem == 0:
                x = np.full((1, 16, 16), 3.25, F32)
            else:              # 120 values under 0, 16 zeros, 120 over: med = +0 and |v - med| has the bits of |v|
                top = 0x7E000000 if rem == 31 else None      # 4e37: finite, bit 30 set
                a = rem_offsets(rem, rng, n=240, below=38, top=top)
                a = a[a != 0]
                a = np.concatenate([a, rng.choice(a, size=240 - a.size)])
                v = a.astype(np.uint32).view(F32).copy()
                v[:120] = -v[:120]
                x = rng.permutation(np.concatenate([v, np.zeros(16, F32)])).reshape(1, 16, 16)
            out.append(Case(name, x.astype(F32), p, f"second select: the bits of |v - med| have rem {rem}"))
        for m in LIVE_COUNTS:
            name = f"sel_m_{m}_c{nc}"
            rng = rng_of(f"sel_m_{m}")
            shape = {1: (2, 4), 2: (4, 4), 3: (4, 6), 255: (16, 16), 256: (16, 16), 257: (17, 17)}[m]
            x = np.full(shape[0] * shape[1], np.nan, F32)
            x[:m] = rng.normal(50.0, 2.0, m).astype(F32)
            x = rng.permutation(x).reshape(1, *shape)
            out.append(Case(name, x, dict(p, cell=17 if m == 257 else 16), f"{m} live keys: rank {(m - 1) // 2}"))
        for name, make in (
                ("sel_negative", lambda r: r.normal(-1000.0, 3.0, 256)),
                ("sel_signed_zeros", lambda r: np.concatenate([r.normal(-1.0, 0.1, 60), np.tile([-0.0, 0.0], 70), r.normal(1.0, 0.1, 56)])),
                ("sel_zeros_only", lambda r: np.tile([-0.0, 0.0, -0.0, -0.0], 64)),
                ("sel_subnormal", lambda r: r.normal(1e-40, 2e-41, 256)),
                ("sel_all_equal", lambda r: np.full(256, -7.5)),
        ):
            rng = rng_of(name)
            x = rng.permutation(np.asarray(make(rng), np.float64).astype(F32)).reshape(1, 16, 16)
            out.append(Case(f"{name}_c{nc}", x, p, name[4:].replace("_", " ")))
    return out


CELL_SHAPES = {   # cell: (a frame with w % 4 == 0, one with w % 4 != 0)
    17: ((40, 52), (18, 35)), 18: ((40, 56), (19, 37)), 50: ((120, 104), (51, 101)), 100: ((130, 204), (101, 201)),
    127: ((130, 256), (128, 255)), 128: ((130, 260), (129, 257)), 129: ((140, 260), (130, 259)),
    255: ((260, 264), (256, 257)), 256: ((257, 300), (100, 257)),
}
LDS_FLIPS = (   # (cell, frame in LDS, frame through global memory)
    (256, (60, 256), (100, 256)), (256, (64, 256), (65, 256)), (200, (64, 256), (90, 254)),
)
SMALL_FRAMES = ((5, 7), (1, 1), (1, 64), (64, 1), (9, 1), (9, 2), (9, 3))


def _cell_cases():
    out = []
    for cell in CELLS:
        for tag, (h, w) in zip(("w4", "wodd"), CELL_SHAPES[cell]):
            name = f"cell_{cell}_{tag}_{h}x{w}"
            x = sky_frame(rng_of(name), h, w, cell, nan_frac=0.02)
            out.append(Case(name, x[None], dict(cell=cell, n_clip=2, filter=1, mode=S.SUBTRACT),
                            f"cell {cell} on {h} x {w}" + ("; last cell 1 px wide and high" if tag == "wodd" and cell < 255 else "")))
    for cell, a, b in LDS_FLIPS:
        for tag, (h, w) in (("lds", a), ("global", b)):
            name = f"cell_{cell}_flip_{tag}_{h}x{w}"
            x = sky_frame(rng_of(name), h, w, cell, nan_frac=0.02)
            out.append(Case(name, x[None], dict(cell=cell, n_clip=1, filter=3, mode=S.NORMALISE), f"cell {cell} on {h} x {w}: {tag}"))
    for h, w in SMALL_FRAMES:
        for cell in (16, 256):
            name = f"cell_{cell}_small_{h}x{w}"
            x = sky_frame(rng_of(name), h, w, cell)
            out.append(Case(name, x[None], dict(cell=cell, n_clip=1, filter=3, mode=S.NORMALISE), f"frame {h} x {w} under one cell of {cell}"
                            if max(h, w) <= cell else f"frame {h} x {w}, cell {cell}"))
    return out


def _empty_cases():
    out = []
    for tag, (h, w), (j, i), keep in (("full_32_kept", (32, 32), (1, 1), 32), ("full_31_empty", (32, 32), (1, 1), 31),
                                       ("part_9_kept", (29, 21), (1, 1), 9), ("part_8_empty", (29, 21), (1, 1), 8)):
        name = f"empty_edge_{tag}"
        rng = rng_of(name)
        x = rng.normal(100.0, 1.0, (h, w)).astype(F32)
        x[16 * j:, 16 * i:] += F32(400)          # the cell in question has a pedestal of its own: the mesh shows whether it was used
        blank(x, 16, [(j, i)], keep=keep, rng=rng)
        for filt in (1, 3):
            out.append(Case(f"{name}_f{filt}", x[None].copy(), dict(cell=16, n_clip=1, filter=filt, mode=S.SUBTRACT),
                            f"{keep} finite pixels in a cell of {min(16, h - 16 * j) * min(16, w - 16 * i)}"))
    return out


def clip_boundary_cell(rng, M, K):
    """med M, mad 1: 116 pixels on M - K and M + K, four far outside"""
    v = np.repeat(np.array([-K, -1, 0, 1, K, 40], np.float64), [58, 8, 70, 58, 58, 4]) + M
    return rng.permutation(v.astype(F32)).reshape(1, 16, 16)


def _clip_cases():
    out = []
    name = "clip_mad0"
    rng = rng_of(name)
    x = rng.normal(20.0, 1.0, (32, 32)).astype(F32)
    x[rng.random((32, 32)) < 0.6] = F32(20.25)
    out.append(Case(name, x[None], dict(cell=16, n_clip=3, filter=1, mode=S.NORMALISE), "more than half of every cell identical: mad 0, lo == hi == med"))
    name = "clip_n8"
    rng = rng_of(name)
    x = sky_frame(rng, 48, 80, 16, sigma=2.0)
    x[rng.random(x.shape) < 0.15] += F32(30)
    out.append(Case(name, x[None], dict(cell=16, n_clip=8, filter=3, mode=S.NORMALISE, k_clip=2.0), "eight rounds on a skewed cell"))
    for M in (0.0, 1000.0):
        for nc in (1, 2):
            name = f"clip_edge_M{int(M)}_c{nc}"
            k, K = find_k_clip()
            out.append(Case(name, clip_boundary_cell(rng_of(name), M, K), dict(ONE_CELL, n_clip=nc, k_clip=k),
                            "116 pixels exactly on lo and hi of round 0; an open interval turns s to 0"))
    return out


def mesh_frame(rng, ny, nx, tied, cell=16):
    tile = rng.normal(0.0, 1.0, (cell, cell)).astype(F32)
    k = np.arange(ny * nx).reshape(ny, nx)
    g = k % (2 if ny * nx <= 4 else 3) if tied else rng.permutation(ny * nx).reshape(ny, nx)   # tied: cells of a group are equal
    ped = (g * 3).astype(F32) + F32(64)
    scale = (1 + g).astype(F32)
    x = np.tile(tile, (ny, nx)) * np.repeat(np.repeat(scale, cell, 0), cell, 1) + np.repeat(np.repeat(ped, cell, 0), cell, 1)
    return x.astype(F32)


def _mesh_cases():
    out = []
    for ny, nx in ((1, 1), (1, 5), (5, 1), (2, 2), (2, 3)):
        rng = rng_of(f"mesh_{ny}x{nx}")
        x = np.stack([mesh_frame(rng, ny, nx, False), mesh_frame(rng, ny, nx, True)])
        for filt, mode in MODES:
            out.append(Case(f"mesh_{ny}x{nx}_f{filt}_m{mode}", x, dict(cell=16, n_clip=1, filter=filt, mode=mode),
                            f"mesh {ny} x {nx}: distinct cell values, then tied ones"))
    rng = rng_of("mesh_17x17")
    x = sky_frame(rng, 272, 272, 16)
    blank(x, 16, [(0, 0), (16, 16), (5, 5), (5, 6), (9, 0)])
    for filt, mode in MODES[:2]:
        out.append(Case(f"mesh_17x17_f{filt}_m{mode}", x[None], dict(cell=16, n_clip=1, filter=filt, mode=mode), "289 cells: k_sky_mesh loops"))
    layouts = {
        "mesh_corner_one_neighbour": ((48, 48), [(0, 0), (0, 1), (1, 0)], "empty corner, of its three neighbours one is not empty"),
        "mesh_ring_of_empties": ((80, 80), [(j, i) for j in (1, 2, 3) for i in (1, 2, 3)], "the centre of a 3 x 3 empty block takes the frame value"),
        "mesh_block_in_corner": ((96, 96), [(j, i) for j in (0, 1, 2) for i in (0, 1, 2)], "3 x 3 empty block in the corner: (0, 0), (0, 1), (1, 0), (1, 1) take the frame value"),
    }
    for name, (shape, cells, note) in layouts.items():
        x = blank(sky_frame(rng_of(name), *shape, 16), 16, cells)
        for filt, mode in MODES[:2]:
            out.append(Case(f"{name}_f{filt}_m{mode}", x[None], dict(cell=16, n_clip=1, filter=filt, mode=mode), note))
    name = "mesh_status_mix"
    rng = rng_of(name)
    good = [sky_frame(rng, 40, 56, 16) for _ in range(2)]
    f = np.stack([good[0], np.full((40, 56), np.nan, F32), np.full((40, 56), 7.0, F32), good[1], np.full((40, 56), -np.inf, F32)])
    for filt, mode in MODES:
        MAX_FRAMES[f"{name}_f{filt}_m{mode}"] = 2
        out.append(Case(f"{name}_f{filt}_m{mode}", f, dict(cell=16, n_clip=1, filter=filt, mode=mode),
                        "good, NO_SKY, NO_NOISE, good, NO_SKY through a handle of two slots"))
    return out


def _apply_cases():
    out = []
    for h, w, cell, be, note in (
            (20, 1028, 16, True, "two spans of the 16-byte path, the second of 4 columns; second row interval of 2 rows"),
            (20, 2052, 16, True, "three spans of the 16-byte path, the last of 4 columns; 258 cells"),
            (20, 1024, 18, False, "one full span; cell % 4 != 0: scalar cell loads, 16-byte apply"),
            (20, 257, 100, True, "one column into the second scalar span"),
            (1, 40, 16, False, "one row"), (2, 40, 16, True, "two rows"), (3, 41, 16, False, "three rows, scalar"),
            (70, 88, 24, False, "plane and pedestals, 3 x 4 mesh"),
    ):
        name = f"apply_{h}x{w}_c{cell}"
        rng = rng_of(name)
        x = np.stack([sky_frame(rng, h, w, cell, nan_frac=0.01), sky_frame(rng, h, w, cell, sigma=3.0)])
        if be:
            BIG_ENDIAN.add(name)
        out.append(Case(name, x, dict(cell=cell, n_clip=1, filter=1, mode=S.NORMALISE), note))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        BIG_ENDIAN.clear(); MAX_FRAMES.clear()
        _CASES = _sel_cases() + _cell_cases() + _empty_cases() + _clip_cases() + _mesh_cases() + _apply_cases()
        for c in _CASES:
            assert c.frames.dtype == F32 and c.frames.ndim == 3 and c.frames.flags.c_contiguous, c.name
            c.frames.setflags(write=False)
    return _CASES
