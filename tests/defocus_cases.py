"""The bank geometries and synthetic rows of tests/test_gpu_defocus_shapes.py, shared with the CPU test of their conditions in
tests/test_defocus_model.py.  Each geometry names the edge of k_def_gemm / k_def_pick it is there for; `expect` holds the tile
facts that make it that edge, checked on the CPU against the restatement."""
import functools

import numpy as np

import defocus_ref as R

SDSS, LSST = (1250.0, 585.0), (4180.0, 2558.0)
BM = BN = 128   # the GEMM's block tile; 32: one MFMA tile, 64: a wave's column pair; 16: one k-step


def geom(expect, heights, radii, seeings, instrument=SDSS, ovs=8, max_shift=5, **trail):
    return {"expect": expect, "heights": heights, "radii": radii, "seeings": seeings, "instrument": instrument, "ovs": ovs,
            "max_shift": max_shift, "trail": trail}


SMALL = dict(pixscale=1.0, prof_step=1.0, wing=1)
GEOMS = {
    # the prefetch branch of the k loop never runs; one partial column tile; every column is its own group
    "one_k_step": geom(dict(K=7, nbp=16, ncol=10, group=1), [50.0, 100.0, 200.0, 400.0], [0.0], [0.9, 1.4], ovs=8, max_shift=0,
                       prof_half=7.0, **SMALL),
    # the prefetch runs once; eight group heads in one 32-column tile
    "two_k_steps": geom(dict(K=8, nbp=32, ncol=48, group=6), [100.0, 200.0, 400.0], [0.0, 1.0], [0.9, 1.4], ovs=4, max_shift=1,
                        prof_half=8.0, **SMALL),
    # F = 26.67 fine steps per px: box and triangle of non-integer width
    "fractional_F": geom(dict(K=80, nbp=176, ncol=378, group=21), [60.0, 80.0, 100.0, 130.0, 200.0], [0.0, 0.5, 2.0],
                         [0.9, 1.43, 2.0], ovs=8, max_shift=3, pixscale=0.396, prof_half=24.0, prof_step=0.3, wing=8),
    # the other instrument; fewer than 128 columns
    "lsst": geom(dict(K=96, nbp=208, ncol=100, group=10), [300.0, 500.0, 800.0, 1500.0], [0.0, 2.0], [0.67, 1.0], instrument=LSST,
                 ovs=4, max_shift=2, pixscale=0.2, prof_half=24.0, prof_step=0.25, wing=8),
    # groups of exactly one MFMA tile, a whole number of block tiles
    "group_32": geom(dict(K=8, nbp=32, ncol=256, group=32), [100.0, 150.0, 250.0], list(np.linspace(0.0, 6.2, 32)), [0.9, 1.4],
                     ovs=4, max_shift=0, prof_half=8.0, **SMALL),
    # one group per wave's pair of MFMA column tiles (n_r at its bound)
    "group_64": geom(dict(K=8, nbp=32, ncol=256, group=64), [100.0, 150.0, 250.0], list(np.linspace(0.0, 12.6, 64)), [0.9],
                     ovs=4, max_shift=0, prof_half=8.0, **SMALL),
    # S at its bound (129 shifts): a group of 258 columns spans block tiles, its maximum is assembled by atomicMax
    "widest_shift": geom(dict(K=240, nbp=496, ncol=5418, group=258), [60.0, 100.0, 140.0, 200.0, 280.0, 400.0], [0.0, 4.0],
                         [0.9, 1.15, 1.4], ovs=8, max_shift=64, pixscale=0.396, prof_half=24.0, prof_step=0.1, wing=8),
    # the ends of the accepted over-sampling
    "ovs_1": geom(dict(K=8, nbp=32, ncol=48, group=6), [100.0, 200.0, 400.0], [0.0, 1.0], [0.9, 1.4], ovs=1, max_shift=1,
                  prof_half=8.0, **SMALL),
    "ovs_64": geom(dict(K=8, nbp=32, ncol=48, group=6), [100.0, 200.0, 400.0], [0.0, 1.0], [0.9, 1.4], ovs=64, max_shift=1,
                   prof_half=8.0, **SMALL),
    # 385 columns: the last column tile holds one column
    "last_tile_of_one": geom(dict(K=16, nbp=48, ncol=385, group=77), [60.0, 100.0, 200.0, 400.0], [0.0, 1.0, 2.0, 4.0, 6.0, 8.0, 10.0],
                             [1.2], ovs=4, max_shift=5, prof_half=16.0, **SMALL),
}
# the geometry-specific tile properties, as predicates over the facts of tile_facts()
PROPERTIES = {
    "one_k_step": lambda f: f["k_steps"] == 1 and f["ncol"] < BN and f["group"] == 1,
    "two_k_steps": lambda f: f["k_steps"] == 2 and f["heads_in_first_tile"] >= 6,
    "fractional_F": lambda f: f["F"] != round(f["F"]) and f["ncol"] % BN not in (0, 1),
    "lsst": lambda f: f["ncol"] < BN and f["k_steps"] > 2,
    "group_32": lambda f: f["group"] == 32 and f["ncol"] % BN == 0,
    "group_64": lambda f: f["group"] == 64 and f["ncol"] % BN == 0,
    "widest_shift": lambda f: f["ns"] == 129 and f["group"] > BN and f["group"] % BN != 0,
    "ovs_1": lambda f: f["ovs"] == 1,
    "ovs_64": lambda f: f["ovs"] == 64,
    "last_tile_of_one": lambda f: f["ncol"] % BN == 1 and f["k_steps"] == 3,
}
LARGEST = "widest_shift"   # by groups and by nbp: the workspace-reuse test's bank A


def grid(ge):
    return R.Grid(ovs=ge["ovs"], max_shift=ge["max_shift"], instrument=ge["instrument"], **ge["trail"])


def bank_kwargs(ge):
    """the keyword arguments of lfd_amd.defocus.DefocusBank"""
    return dict(heights=ge["heights"], radii=ge["radii"], seeings=ge["seeings"], instrument=ge["instrument"], ovs=ge["ovs"],
                max_shift=ge["max_shift"], **ge["trail"])


def restate(ge):
    return R.Restated(grid(ge), ge["heights"], ge["radii"], ge["seeings"])


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restated bank of a named geometry: computed once, shared, never changed"""
    return restate(GEOMS[name])


def tile_facts(rb):
    heads = np.flatnonzero(np.arange(rb.ncol) % rb.group == 0)
    return {"K": rb.g.K, "nbp": rb.nbp, "ncol": rb.ncol, "group": rb.group, "ns": rb.ns, "ovs": rb.g.ovs, "F": rb.g.F,
            "k_steps": rb.nbp // 16, "n_groups": rb.n_se * (rb.n_h + 1), "heads_in_first_tile": int((heads < 32).sum()),
            "n_valid": int(rb.valid.sum()), "n_models": len(rb.models)}


def make_trails(n, noise=0.05):
    from lfd_amd import _native
    t = np.zeros(n, _native.TRAIL_DTYPE)
    t["status"], t["noise"] = _native.TRAIL_OK, noise
    return t


def make_rows(rb, n, seed, noise=0.05):
    """(trails, float32 profiles [n, 2K+1], kind): 80 % noisy copies of random valid columns at random amplitude and offset, 10 %
    pure noise, 10 % the negative of a column (no column scores above 0 but by the noise), all with N(0, noise) added."""
    rng = np.random.default_rng(seed)
    vj = np.flatnonzero(rb.vcol)
    j = rng.choice(vj, n)
    kind = rng.choice(3, n, p=[0.8, 0.1, 0.1])   # 0 copy, 1 noise, 2 negative
    amp = rng.uniform(2.0, 4.0, n) * np.where(kind == 2, -1.0, 1.0) * (kind != 1)
    off = rng.uniform(-1.0, 1.0, n)
    prof = amp[:, None] * rb.c64[j] + off[:, None] + rng.normal(0.0, noise, (n, rb.nb))
    return make_trails(n, noise), prof.astype(np.float32), kind


def non_decisive_share(rb, trails, prof, seeing=None):
    J = R.judge(rb, trails, prof, seeing)
    return float(1.0 - J["decisive"].mean()), J


N_ROWS = {"ovs_1": 64, "ovs_64": 64}   # bank parity is what these two are for: a short fit


def fit_inputs(name):
    """the rows every geometry is fitted with: (restated bank, trails, profiles)"""
    rb = restated(name)
    trails, prof, _ = make_rows(rb, N_ROWS.get(name, 300), 100 + list(GEOMS).index(name))
    return rb, trails, prof


def variant(name, **grids):
    """a named geometry with some of heights / radii / seeings replaced"""
    return dict(GEOMS[name], **grids)


def column_index(rb, ise, ih, ir, s):
    return ((ise * (rb.n_h + 1) + ih) * rb.n_r + ir) * rb.ns + s + rb.g.S


def clean_rows(rb, cols, seed, noise=1e-3):
    """rows 3 * column + 0.5 + N(0, noise) of the given columns: noise small enough that every row is decisive"""
    rng = np.random.default_rng(seed)
    cols = np.asarray(cols)
    prof = 3.0 * rb.c64[cols] + 0.5 + rng.normal(0.0, noise, (len(cols), rb.nb))
    return make_trails(len(cols), noise), prof.astype(np.float32)


# ---- ties: banks that hold bit-identical columns --------------------------------------------------------------------------------
def tie_cases():
    """name -> (geometry, restated bank, trails, profiles, the column each row must return)"""
    out = {}
    # the focus model's n_r radius entries are the same point: radius index 0 must come back
    ge = variant("two_k_steps", radii=[0.0, 0.5, 2.0])
    rb = restate(ge)
    src = [column_index(rb, ise, rb.n_h, ir, s) for ise in range(rb.n_se) for ir in range(rb.n_r) for s in (-1, 0, 1)]
    want = [column_index(rb, ise, rb.n_h, 0, s) for ise in range(rb.n_se) for ir in range(rb.n_r) for s in (-1, 0, 1)]
    out["focus_duplicates"] = (ge, rb) + clean_rows(rb, src, 1) + (np.array(want),)
    # two equal radii: every height's two models are identical
    ge = variant("two_k_steps", radii=[0.0, 0.0])
    rb = restate(ge)
    src = np.flatnonzero(rb.vcol)
    want = [column_index(rb, j // rb.ns // rb.n_r // (rb.n_h + 1), (j // rb.ns // rb.n_r) % (rb.n_h + 1), 0, j % rb.ns - rb.g.S)
            for j in src]
    out["equal_radii"] = (ge, rb) + clean_rows(rb, src, 2) + (np.array(want),)
    # two equal heights: two bit-identical groups, the first must win
    ge = variant("two_k_steps", heights=[100.0, 100.0])
    rb = restate(ge)
    src = [column_index(rb, ise, ih, ir, s) for ise in range(rb.n_se) for ih in (0, 1) for ir in range(rb.n_r) for s in (-1, 0, 1)]
    src = [j for j in src if rb.vcol[j]]
    want = [j - rb.group if (j // rb.group) % (rb.n_h + 1) == 1 else j for j in src]
    out["equal_heights"] = (ge, rb) + clean_rows(rb, src, 3) + (np.array(want),)
    # two equal seeings: two bit-identical slices, the lower must win
    ge = variant("two_k_steps", seeings=[0.9, 0.9])
    rb = restate(ge)
    src = np.flatnonzero(rb.vcol)
    per = rb.ncol // 2
    want = src % per
    focus = (want // rb.group) == rb.n_h     # the focus model's radius entries are one point as well
    want = np.where(focus, want - (want % rb.group) // rb.ns * rb.ns, want)
    out["equal_seeings"] = (ge, rb) + clean_rows(rb, src, 4) + (want,)
    return out
