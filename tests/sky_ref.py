"""numpy restatement of the sky normalisation (include/lfdmi.h: sky normalisation, steps 1 - 7).  No device; every statistic
is a selection (np.partition / np.sort), every float32 operation is one numpy float32 operation, so the device can match it
bit for bit."""
import numpy as np

SUBTRACT, NORMALISE = 0, 1
OK, NO_SKY, NO_NOISE = 0, 1, 2
DEFAULTS = dict(cell=64, k_clip=3.0, n_clip=3, filter=3, mode=NORMALISE, target_sigma=0.025)
F32 = np.float32


def lowmed(v):
    """rank floor((m-1)/2) in ascending order"""
    v = np.asarray(v).ravel()
    return np.partition(v, (v.size - 1) // 2)[(v.size - 1) // 2]


def cell_stat(pix, k_clip, n_clip):
    """step 2 for one cell's pixels -> (b, s, |S_0|)"""
    s0 = pix[np.isfinite(pix)].astype(F32) + F32(0)        # (-0 counts as +0)
    n0 = s0.size
    if n0 == 0:
        return F32(0), F32(0), 0
    s = s0
    for t in range(n_clip + 1):
        med = lowmed(s)
        mad = lowmed(np.abs(s - med))                      # float32 subtraction
        if t < n_clip:
            d = float(k_clip) * 1.4826 * float(mad)
            lo, hi = float(med) - d, float(med) + d
            sd = s.astype(np.float64)
            s = s[(sd >= lo) & (sd <= hi)]
    return F32(med), F32(1.4826 * float(mad)), n0


def axis_table(length, cell):
    """step 6 along one axis: (index j per position, float32 weight per position, number of cells)"""
    nc = -(-length // cell)
    r0 = np.arange(nc) * cell
    r1 = np.minimum(r0 + cell, length)
    centre = (r0 + r1 - 1) * 0.5
    y = np.arange(length, dtype=np.float64)
    j = np.maximum(np.searchsorted(centre, y, side="right") - 1, 0)
    j2 = np.minimum(j + 1, nc - 1)
    t = np.zeros(length, F32)
    ok = (j2 != j) & (y >= centre[j])
    t[ok] = ((y[ok] - centre[j[ok]]) / (centre[j2[ok]] - centre[j[ok]])).astype(F32)
    return j, j2, t, nc


def _neigh(mesh, j, i, ny, nx, centre):
    out = []
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if (dj or di or centre) and 0 <= j + dj < ny and 0 <= i + di < nx:
                out.append((j + dj, i + di))
    return out


def meshes(x, cell=64, k_clip=3.0, n_clip=3, filter=3, mode=NORMALISE, target_sigma=0.025):
    """steps 1 - 5 -> (record dict, filtered b mesh, filtered s mesh, step-2 b, step-2 s, non-empty mask)"""
    H, W = x.shape
    ny, nx = -(-H // cell), -(-W // cell)
    b = np.zeros((ny, nx), F32)
    s = np.zeros((ny, nx), F32)
    ne = np.zeros((ny, nx), bool)
    for j in range(ny):
        for i in range(nx):
            pix = x[j * cell:min((j + 1) * cell, H), i * cell:min((i + 1) * cell, W)]
            b[j, i], s[j, i], n0 = cell_stat(pix, k_clip, n_clip)
            ne[j, i] = 8 * n0 >= pix.size
    rec = dict(status=OK, ny=ny, nx=nx, n_empty=int((~ne).sum()), sky=np.nan, sigma=np.nan, gain=1.0)
    if not ne.any():
        rec["status"] = NO_SKY
        nan = np.full((ny, nx), np.nan, F32)
        return rec, nan, nan.copy(), b, s, ne
    sky, sigma = lowmed(b[ne]), lowmed(s[ne])
    fb, fs = b.copy(), s.copy()
    for j, i in zip(*np.nonzero(~ne)):
        nb = [q for q in _neigh(b, j, i, ny, nx, False) if ne[q]]
        fb[j, i] = lowmed([b[q] for q in nb]) if nb else sky
        fs[j, i] = lowmed([s[q] for q in nb]) if nb else sigma
    if filter == 3:
        mb, ms = np.empty_like(fb), np.empty_like(fs)
        for j in range(ny):
            for i in range(nx):
                nb = _neigh(fb, j, i, ny, nx, True)
                mb[j, i] = lowmed([fb[q] for q in nb])
                ms[j, i] = lowmed([fs[q] for q in nb])
    else:
        mb, ms = fb, fs
    gain = F32(1)
    if mode == NORMALISE:
        if sigma == 0:
            rec["status"] = NO_NOISE
        else:
            gain = F32(float(target_sigma) / float(sigma))
    rec.update(sky=float(sky), sigma=float(sigma), gain=float(gain))
    return rec, mb, ms, b, s, ne


def background(mb, shape, cell):
    """step 6: the float32 background image of a filtered mesh"""
    H, W = shape
    j, j2, ty, _ = axis_table(H, cell)
    i, i2, tx, _ = axis_table(W, cell)
    tx = tx[None, :]
    ty = ty[:, None]
    a, b_ = mb[j][:, i], mb[j][:, i2]
    c, d = mb[j2][:, i], mb[j2][:, i2]
    top = a + tx * (b_ - a)
    bot = c + tx * (d - c)
    return top + ty * (bot - top)


def normalize(x, **params):
    """one frame -> (out float32, record dict, filtered b mesh, filtered s mesh)"""
    p = dict(DEFAULTS, **params)
    x = np.asarray(x)
    if x.dtype.byteorder == ">":
        x = x.astype("<f4")
    x = np.ascontiguousarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        rec, mb, ms, _, _, _ = meshes(x, **p)
        fin = np.isfinite(x)
        if rec["status"] == NO_SKY:
            out = np.where(fin, x, F32(0)).astype(F32)
        else:
            bkg = background(mb, x.shape, p["cell"])
            out = np.where(fin, (x - bkg) * F32(rec["gain"]), F32(0)).astype(F32)
    return out, rec, mb, ms


def normalize_batch(frames, **params):
    outs, recs, mbs, mss = [], [], [], []
    for f in frames:
        o, r, mb, ms = normalize(f, **params)
        outs.append(o); recs.append(r); mbs.append(mb); mss.append(ms)
    return np.stack(outs), recs, np.stack(mbs), np.stack(mss)
