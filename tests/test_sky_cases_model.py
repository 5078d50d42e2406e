"""The named frames of tests/sky_cases.py on the CPU: every case sits on the kernel seam it is named for, shown with the numpy
restatement of the kernels' index arithmetic in the same file (sky_key, the kmin / rem / pass schedule of sky_select, the
rounds of k_sky_cells, the host's path choices, the grid of k_sky_apply), and that restated radix schedule returns what
np.partition returns -- on random keys and on every cell of every case.  So when tests/test_gpu_sky_seams.py finds the device
and tests/sky_ref.py apart, the selection schedule as written is not the reason.  Every case also runs through sky_ref here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sky_cases as K  # noqa: E402
import sky_ref as S  # noqa: E402

F32 = np.float32
N_CASES = 154


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in K.cases()}


def family(cases, prefix):
    return [c for c in cases.values() if c.name.startswith(prefix)]


def cells_of(x, cell):
    h, w = x.shape
    for j in range(-(-h // cell)):
        for i in range(-(-w // cell)):
            yield (j, i), x[j * cell:(j + 1) * cell, i * cell:(i + 1) * cell]


def trace(c, f=0, ji=(0, 0)):
    cell = c.params["cell"]
    j, i = ji
    pix = c.frames[f][j * cell:(j + 1) * cell, i * cell:(i + 1) * cell]
    return K.cell_trace(pix, c.params.get("k_clip", 3.0), c.params["n_clip"])


def passes_of(rem):
    """sky_select: min(8, rem) bits at a time from the top"""
    return [8] * (rem // 8) + ([rem % 8] if rem % 8 else [])


def test_the_set_is_whole_and_every_case_runs_through_the_restatement(cases):
    all_cases = K.cases()
    assert len(all_cases) == N_CASES == len(cases)                    # no name twice
    for fam in K.FAMILIES:
        assert family(cases, fam + "_"), fam
    assert {c.family for c in all_cases} == set(K.FAMILIES)
    assert K.BIG_ENDIAN and K.BIG_ENDIAN <= set(cases) and set(K.MAX_FRAMES) <= set(cases)
    for c in all_cases:
        n, h, w = c.frames.shape
        assert c.note and n >= 1
        assert max(h, w) <= 300 or c.name.startswith(("apply_20x", "mesh_17x17")), c.name
        for x in c.frames:
            out, rec, mb, ms = S.normalize(x, **c.params)
            assert out.shape == x.shape and np.isfinite(out).all(), c.name
            assert mb.shape == (rec["ny"], rec["nx"]) == (-(-h // c.params["cell"]), -(-w // c.params["cell"]))
            # (inside the supported range: no |v - med| overflows)
            for _, pix in cells_of(x, c.params["cell"]):
                assert not any(r["overflow"] for r in K.cell_trace(pix, c.params.get("k_clip", 3.0), c.params["n_clip"])["rounds"]), c.name
    # the same draw every time
    again = K.rng_of("cell_17_w4_40x52")
    assert np.array_equal(K.sky_frame(again, 40, 52, 17, nan_frac=0.02), cases["cell_17_w4_40x52"].frames[0], equal_nan=True)


def test_key_and_radix_schedule_give_np_partition(cases):
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.normal(0, 1, 500), [0.0, 1e-40, -1e-40, 3e38, -3e38, 1e-45, -1e-45]]).astype(F32)
    k = K.f2k(v)
    assert np.array_equal(np.argsort(k, kind="stable"), np.argsort(v, kind="stable"))          # order-preserving
    assert np.array_equal(K.k2f(k).view(np.uint32), v.view(np.uint32)) and K.valid_key(k).all()
    assert not K.valid_key(K.f2k(np.array([np.inf, -np.inf, -0.0], F32))).any()
    for m in (1, 2, 3, 4, 255, 256, 257, 1000):
        for bits in (0, 1, 5, 8, 9, 20, 32):
            keys = (rng.integers(0, 1 << bits, size=m, dtype=np.int64) + (rng.integers(0, (1 << 32) - (1 << bits)) if bits < 32 else 0)).astype(np.uint32)
            t = K.select_trace(keys)
            assert t["key"] == int(np.partition(keys, (m - 1) // 2)[(m - 1) // 2]), (m, bits)
            assert t["widths"] == passes_of(t["rem"]) and t["rem"] <= bits
    n_sel = 0
    for c in cases.values():
        p = c.params
        for x in c.frames:
            for _, pix in cells_of(x, p["cell"]):
                tr = K.cell_trace(pix, p.get("k_clip", 3.0), p["n_clip"])
                b, s, n0 = S.cell_stat(pix, p.get("k_clip", 3.0), p["n_clip"])
                assert n0 == tr["n0"]
                if n0:
                    assert (b.view(np.uint32), s.view(np.uint32)) == (tr["b"].view(np.uint32), tr["s"].view(np.uint32)), c.name
                    n_sel += 2 * len(tr["rounds"])
    assert n_sel > 5000


def test_sel_cases_sit_on_the_selection_seams(cases):
    for nc in (0, 1):
        for rem in K.REMS:
            c = cases[f"sel_rem_{rem}_c{nc}"]
            assert c.frames.shape == (1, 16, 16) and c.params == dict(K.ONE_CELL, n_clip=nc)
            t = trace(c)["rounds"][0]["sel_med"]
            assert t["m"] == 256 and t["rem"] == rem and t["widths"] == passes_of(rem), (rem, t)
            assert len(t["widths"]) == -(-rem // 8)
            if rem:
                assert t["widths"][-1] == (rem - 1) % 8 + 1 and (t["widths"][-1] == 1) == (rem in (1, 9, 17, 25))
                assert t["cands"][-1] >= 100 and t["distinct"][-1] >= 2 and t["ties"] >= 20    # decided in the last pass, among ties
            if rem == 32:
                x = c.frames[0]
                assert x.min() < -9e29 and x.max() > 9e29
        for rem in K.MAD_REMS:
            c = cases[f"sel_mad_{rem}_c{nc}"]
            r0 = trace(c)["rounds"][0]
            t = r0["sel_mad"]
            assert t["kmin"] == 0 and t["rem"] == rem and t["widths"] == passes_of(rem), (rem, t)
            if rem:
                assert r0["med"].view(np.uint32) == 0 and t["ties"] >= 20 and t["distinct"][-1] >= 2 - (rem == 1)
                assert t["cands"][-1] >= 100
        for m in K.LIVE_COUNTS:
            c = cases[f"sel_m_{m}_c{nc}"]
            tr = trace(c)
            t = tr["rounds"][0]["sel_med"]
            area = c.frames[0].size
            assert tr["n0"] == m == t["m"] and 8 * m >= area and t["rem"] >= (m > 1)
            want = np.sort(c.frames[0][np.isfinite(c.frames[0])])[(m - 1) // 2]
            assert K.k2f(np.uint32(t["key"]))[()] == want
            assert K.host_paths(*c.frames.shape[1:], c.params["cell"])["use_lds"]
        for m in (1, 2, 3):                                           # the smallest counts sit on 8 m == area as well
            assert 8 * m == cases[f"sel_m_{m}_c{nc}"].frames[0].size
        x = cases[f"sel_negative_c{nc}"].frames[0]
        assert (x < 0).all() and (K.f2k(x) < 0x80000000).all() and trace(cases[f"sel_negative_c{nc}"])["rounds"][0]["sel_med"]["rem"] >= 16
        c = cases[f"sel_signed_zeros_c{nc}"]
        b = c.frames[0].view(np.uint32)
        assert (b == 0x80000000).sum() == 70 and (b == 0).sum() == 70
        r0 = trace(c)["rounds"][0]
        assert r0["med"].view(np.uint32) == 0 and r0["sel_med"]["rem"] >= 31 and r0["sel_med"]["ties"] == 140
        c = cases[f"sel_zeros_only_c{nc}"]
        assert set(c.frames[0].view(np.uint32).ravel().tolist()) == {0, 0x80000000}
        assert trace(c)["rounds"][0]["sel_med"]["rem"] == 0          # (told apart, the zeros would be two keys: rem 1)
        c = cases[f"sel_subnormal_c{nc}"]
        r0 = trace(c)["rounds"][0]
        assert (np.abs(c.frames[0]) < np.finfo(F32).tiny).all() and 0 < r0["med"] < np.finfo(F32).tiny and 0 < r0["mad"] < np.finfo(F32).tiny
        r0 = trace(cases[f"sel_all_equal_c{nc}"])["rounds"][0]
        assert r0["sel_med"]["rem"] == 0 and r0["sel_mad"]["rem"] == 0 and r0["med"] == F32(-7.5) and r0["mad"] == 0


def test_cell_cases_sit_on_the_cell_and_path_seams(cases):
    seen = set()
    for cell in K.CELLS:
        a, b = [c for c in family(cases, f"cell_{cell}_w")]
        (ha, wa), (hb, wb) = a.frames.shape[1:], b.frames.shape[1:]
        assert wa % 4 == 0 and wb % 4 != 0 and a.params["cell"] == b.params["cell"] == cell
        pa, pb = K.host_paths(ha, wa, cell), K.host_paths(hb, wb, cell)
        assert pa["v4"] and pa["vec_in"] == (cell % 4 == 0) and not pb["v4"] and not pb["vec_in"]
        assert pa["use_lds"] == pb["use_lds"] == (cell <= 128) or cell == 256
        seen.add((pa["vec_in"], pa["v4"], pa["use_lds"]))
        if cell < 255:
            assert hb == cell + 1 and wb == 2 * cell + 1              # the last cells are 1 px high and 1 px wide
    assert seen == {(True, True, True), (False, True, True), (True, True, False), (False, True, False)}
    assert K.host_paths(130, 260, 128)["lds_px"] == K.SKY_LDS_MAX and not K.host_paths(140, 260, 129)["use_lds"]
    for cell, lds, glob in K.LDS_FLIPS:
        a = cases[f"cell_{cell}_flip_lds_{lds[0]}x{lds[1]}"]
        b = cases[f"cell_{cell}_flip_global_{glob[0]}x{glob[1]}"]
        assert K.host_paths(*a.frames.shape[1:], cell)["use_lds"] and not K.host_paths(*b.frames.shape[1:], cell)["use_lds"]
    assert K.host_paths(64, 256, 256)["lds_px"] == K.SKY_LDS_MAX and K.host_paths(65, 256, 256)["lds_px"] == 0
    small = family(cases, "cell_16_small_") + family(cases, "cell_256_small_")
    assert {c.frames.shape[1:] for c in small} == set(K.SMALL_FRAMES) and len(small) == 2 * len(K.SMALL_FRAMES)
    assert {c.frames.shape[2] for c in small} >= {1, 2, 3}
    for c in small:
        assert K.host_paths(*c.frames.shape[1:], c.params["cell"])["use_lds"]
    for c in family(cases, "cell_"):                                  # no cell of this family is empty: the paths run to their end
        assert all(S.normalize(x, **c.params)[1]["n_empty"] == 0 for x in c.frames), c.name


def test_empty_cases_sit_on_the_threshold(cases):
    for tag, area, keep, empty in (("full_32_kept", 256, 32, False), ("full_31_empty", 256, 31, True),
                                   ("part_9_kept", 65, 9, False), ("part_8_empty", 65, 8, True)):
        for filt in (1, 3):
            c = cases[f"empty_edge_{tag}_f{filt}"]
            pix = c.frames[0][16:, 16:]
            assert pix.size == area and np.isfinite(pix).sum() == keep and (8 * keep < area) == empty
            assert np.isnan(pix).any() and np.isposinf(pix).any() and np.isneginf(pix).any()
            out, rec, mb, ms = S.normalize(c.frames[0], **c.params)
            assert rec["n_empty"] == int(empty) and rec["status"] == S.OK
            if filt == 1:
                assert (mb[1, 1] > 400) == (not empty) and (mb[:1] < 200).all()      # the mesh shows which happened
    assert 8 * 32 == 256 and 8 * 8 < 65 <= 8 * 9 and 65 // 8 == 8    # equality; and an area / 8 in integers would keep 8


def test_clip_cases_sit_on_the_clip_edges(cases):
    c = cases["clip_mad0"]
    for ji, pix in cells_of(c.frames[0], 16):
        r = trace(c, 0, ji)["rounds"]
        assert 2 * (pix == F32(20.25)).sum() > pix.size
        assert r[0]["mad"] == 0 and r[0]["lo"] == r[0]["hi"] == float(r[0]["med"]) == 20.25
        assert r[1]["sel_med"]["m"] == (pix == F32(20.25)).sum() and r[1]["sel_med"]["rem"] == 0
    assert S.normalize(c.frames[0], **c.params)[1]["status"] == S.NO_NOISE
    c = cases["clip_n8"]
    assert c.params["n_clip"] == 8
    live = [[r["sel_med"]["m"] for r in trace(c, 0, ji)["rounds"]] for ji, _ in cells_of(c.frames[0], 16)]
    assert all(len(m) == 9 for m in live) and max(len(set(m)) for m in live) >= 4       # rounds that still drop pixels
    k, kk = K.find_k_clip()
    assert k * 1.4826 == float(kk) and 2 <= kk <= 8 and abs(k - kk / 1.4826) < 1e-15
    for M in (0, 1000):
        for nc in (1, 2):
            c = cases[f"clip_edge_M{M}_c{nc}"]
            assert c.params["k_clip"] == k and (c.frames[0] == np.round(c.frames[0])).all()
            tr = trace(c)
            r0 = tr["rounds"][0]
            assert (r0["med"], r0["mad"], r0["lo"], r0["hi"]) == (M, 1, M - float(kk), M + float(kk)) and r0["on_edge"] == 116
            assert tr["rounds"][1]["sel_med"]["m"] == 252
            opened = K.cell_trace(c.frames[0], k, nc, closed=False)
            assert opened["rounds"][1]["sel_med"]["m"] == 136
            assert tr["s"] == F32(1.4826) and opened["s"] == 0 and tr["b"] == opened["b"] == M   # dropping the edge changes s


def test_mesh_cases_sit_on_the_mesh_seams(cases):
    sizes = set()
    for ny, nx in ((1, 1), (1, 5), (5, 1), (2, 2), (2, 3)):
        got = family(cases, f"mesh_{ny}x{nx}_")
        assert {(c.params["filter"], c.params["mode"]) for c in got} == set(K.MODES)
        for c in got:
            assert c.frames.shape == (2, 16 * ny, 16 * nx)
            rec, mb, ms, b, s, ne = S.meshes(c.frames[0], **c.params)
            assert ne.all() and len(set(b.ravel().tolist())) == ny * nx and len(set(s.ravel().tolist())) == ny * nx
            rec, mb, ms, b, s, ne = S.meshes(c.frames[1], **c.params)
            assert ne.all() and (ny * nx == 1 or len(set(b.ravel().tolist())) < ny * nx) and rec["sigma"] > 0
        for j in range(ny):
            for i in range(nx):
                sizes.add(len(S._neigh(None, j, i, ny, nx, True)))
    assert sizes == {1, 2, 3, 4, 6}                                   # lower-median ranks 0, 0, 1, 1, 2
    for c in family(cases, "mesh_17x17_"):
        rec, mb, ms, b, s, ne = S.meshes(c.frames[0], **c.params)
        assert ne.size == 289 > K.SKY_THREADS and rec["n_empty"] == 5 and not ne[0, 0] and not ne[16, 16]
    for c in family(cases, "mesh_corner_one_neighbour_"):
        rec, mb, ms, b, s, ne = S.meshes(c.frames[0], **c.params)
        assert not ne[0, 0] and [bool(ne[q]) for q in S._neigh(None, 0, 0, 3, 3, False)] == [False, False, True]
        if c.params["filter"] == 1:
            assert mb[0, 0] == b[1, 1]
    for name, lone in (("mesh_ring_of_empties_", [(2, 2)]), ("mesh_block_in_corner_", [(0, 0), (0, 1), (1, 0), (1, 1)])):
        for c in family(cases, name):
            rec, mb, ms, b, s, ne = S.meshes(c.frames[0], **c.params)
            ny, nx = ne.shape
            assert rec["n_empty"] == 9 and rec["status"] == S.OK
            alone = [q for q in zip(*np.nonzero(~ne)) if not any(ne[r] for r in S._neigh(None, *q, ny, nx, False))]
            assert sorted(alone) == lone
            if c.params["filter"] == 1:
                assert all(mb[q] == F32(rec["sky"]) and ms[q] == F32(rec["sigma"]) for q in lone)
    got = family(cases, "mesh_status_mix_")
    assert {(c.params["filter"], c.params["mode"]) for c in got} == set(K.MODES)
    for c in got:
        st = [S.normalize(x, **c.params)[1]["status"] for x in c.frames]
        assert st == [S.OK, S.NO_SKY, S.NO_NOISE if c.params["mode"] == S.NORMALISE else S.OK, S.OK, S.NO_SKY]
        assert K.MAX_FRAMES[c.name] == 2 and len(c.frames) == 5        # chunks (0, 1), (2, 3), (4)
    assert len(family(cases, "mesh_")) == 32


def test_apply_cases_sit_on_the_apply_seams(cases):
    def grid(name):
        c = cases[name]
        n, h, w = c.frames.shape
        hp = K.host_paths(h, w, c.params["cell"])
        return hp, K.apply_grid(h, w, c.params["cell"], hp["v4"])
    hp, (spans, last, rstart, rows) = grid("apply_20x1028_c16")
    assert hp["v4"] and hp["vec_in"] and (spans, last) == (2, 4) and rstart == [0, 18, 20]
    assert rows == [[5, 5, 4, 4], [1, 1, 0, 0]]                       # an interval of fewer rows than SKY_ROW_SPLIT
    hp, (spans, last, rstart, rows) = grid("apply_20x2052_c16")
    assert hp["v4"] and (spans, last) == (3, 4) and 2 * -(-2052 // 16) == 258 > K.SKY_THREADS
    hp, (spans, last, rstart, rows) = grid("apply_20x1024_c18")
    assert hp["v4"] and not hp["vec_in"] and (spans, last) == (1, 1024) and rstart == [0, 19, 20]
    hp, (spans, last, rstart, rows) = grid("apply_20x257_c100")
    assert not hp["v4"] and (spans, last) == (2, 1) and rstart == [0, 20]
    for h, w in ((1, 40), (2, 40), (3, 41)):
        hp, (spans, last, rstart, rows) = grid(f"apply_{h}x{w}_c16")
        assert hp["v4"] == (w % 4 == 0) and rstart == [0, h] and rows == [[1] * h + [0] * (4 - h)]
    # misaligned by one float, as tests/test_gpu_sky_seams.py runs the w % 4 == 0 cases: every 16-byte path goes scalar
    assert K.host_paths(20, 1028, 16, src_off=1) == dict(K.host_paths(20, 1028, 16), vec_in=False, v4=False, span=256, spans=5)
    assert K.host_paths(20, 1028, 16, dst_off=1) == dict(K.host_paths(20, 1028, 16), v4=False, span=256, spans=5)
    c = cases["apply_70x88_c24"]
    for x in c.frames:                                                # the plane and the pedestals reach every pixel
        out, rec, mb, ms = S.normalize(x, **c.params)
        assert len(set(mb.ravel().tolist())) == mb.size == 12
        j, j2, ty, _ = S.axis_table(70, 24)
        i, i2, tx, _ = S.axis_table(88, 24)
        assert ((ty > 0) & (ty < 1)).sum() >= 40 and ((tx > 0) & (tx < 1)).sum() >= 60
    assert K.BIG_ENDIAN == {"apply_20x1028_c16", "apply_20x2052_c16", "apply_20x257_c100", "apply_2x40_c16"}
    assert len(family(cases, "apply_")) == 8
