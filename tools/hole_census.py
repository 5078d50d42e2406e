"""Developer tool (CPU only): how many hole borders of the bench frames the certain-reject test of lfd_amd/csrc/hole_prune.h
removes, and what share of the hole-slot updates of k_frame_contours' extremes phase goes with them.

    python tools/hole_census.py [frames=24]

Oracle edge maps of both passes (remove_stars -> flip -> bright / dim, Canny of the image fit_minAreaRect sees) of the
synthetic SDSS frames bench.py uses (frame k = synth.make_frame(k)).  A slot update is one contact of an edge stretch with a
run of a hole: the edge pixel left and right of every hole run, and every stretch of edge pixels above or below it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy import ndimage

from lfd_amd import synth
from lfd_amd.detecttrails import default_params
from oracle import lfd_oracle as O


def rejected(n, wb, hb, min_len, lw):
    """hole_border_rejected of hole_prune.h on arrays."""
    d2 = (wb.astype(np.int64) ** 2 + hb.astype(np.int64) ** 2).astype(np.float64)
    if not lw > 0:
        return np.zeros(len(n), bool)
    r = d2 < lw * n.astype(np.float64) * 0.999
    if min_len > 0:
        r |= d2 <= (lw * min_len) ** 2 * 0.999
    return r


def census(edge, min_len, lw):
    e = edge != 0
    lab, nl = ndimage.label(~e, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    outside = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    is_hole = np.ones(nl + 1, bool)
    is_hole[0] = False
    is_hole[outside] = False
    n = np.bincount(lab.ravel(), minlength=nl + 1)
    wb, hb = np.zeros(nl + 1, np.int64), np.zeros(nl + 1, np.int64)
    for i, sl in enumerate(ndimage.find_objects(lab), 1):
        if sl is not None and is_hole[i]:
            hb[i] = sl[0].stop - sl[0].start + 1
            wb[i] = sl[1].stop - sl[1].start + 1
    hl = np.where(is_hole[lab], lab, 0)
    upd = np.zeros(nl + 1, np.int64)
    ep = np.pad(e, 1)
    hp = np.pad(hl, 1)
    core = hp[1:-1, 1:-1]
    upd += np.bincount(core[(core > 0) & ep[1:-1, :-2]], minlength=nl + 1)   # the edge pixel left of a hole run
    upd += np.bincount(core[(core > 0) & ep[1:-1, 2:]], minlength=nl + 1)    # ... and right of it
    for dy in (0, 2):                                                          # stretches of edge pixels above / below
        c = (core > 0) & ep[dy:dy + core.shape[0], 1:-1]
        cl = np.where(c, core, 0)
        prev = np.pad(cl, ((0, 0), (1, 0)))[:, :-1]
        upd += np.bincount(cl[c & (prev != cl)], minlength=nl + 1)
    ids = np.flatnonzero(is_hole)
    rej = rejected(n[ids], wb[ids], hb[ids], min_len, lw)
    return len(ids), int(rej.sum()), int(upd[ids].sum()), int(upd[ids][rej].sum()), int((hb[ids] + 1).sum()), int((hb[ids] + 1)[rej].sum())


def main():
    nf = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    pb, pd, prs = default_params()
    rs = O.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    tot = {"bright": np.zeros(6, np.int64), "dim": np.zeros(6, np.int64)}
    for k in range(nf):
        img, cat, _ = synth.make_frame(k)
        O.remove_stars(img, cat, rs)
        _, equ_b, _ = O.process_bright(img.copy(), pb, flip=True, want_images=True)
        _, equ_d, _ = O.process_dim(img.copy(), pd, flip=True, after_bright=True, want_images=True)
        for name, equ, p in (("bright", equ_b, pb), ("dim", equ_d, pd)):
            tot[name] += census(O.canny(equ, 0, 255), p["minAreaRectMinLen"], p["lwTresh"])
    print("%d frames; per pass: holes, rejected, hole slot updates, of rejected holes, hole row slots, of rejected holes" % nf)
    for name, t in tot.items():
        print("%-6s holes %d rejected %d (%.1f %%) | slot updates %d with rejected holes %d (%.1f %%) | row slots %d with rejected holes %d (%.1f %%)"
              % (name, t[0], t[1], 100.0 * t[1] / max(t[0], 1), t[2], t[3], 100.0 * t[3] / max(t[2], 1), t[4], t[5], 100.0 * t[5] / max(t[4], 1)))


if __name__ == "__main__":
    main()
