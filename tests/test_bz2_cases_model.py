"""The crafted bzip2 files of tests/bz2_cases.py on the CPU: libbz2 (Python's ``bz2``) makes of every case what the case says,
every case sits on the kernel seam it names (a numpy restatement of the index arithmetic of k_bz2.h: mark residues, staging fill
at each run, head stretch and cycle length of the walk, where a nominal stretch start lands in a run of four, bytes per tile),
and the shared block core (tools/bz2_core_check.cpp over lfd_amd/csrc/bz2_core.h) agrees -- once as a plain build, once under
AddressSanitizer + UBSan (a stand-alone program).  tests/test_gpu_bz2_seams.py runs the same cases on the device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bz2_cases as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what libbz2 does with the cases that are not "decode" (True = it decodes them, to the writer's bytes)
LIBBZ2_ACCEPTS = {
    "marks_257_one_stream": True, "marks_258_joined": True,           # valid files, beyond the decoder's BZ_MARK_CAP
    "max_block_plus_1_run_1": False, "max_block_plus_1_symbol_1": False, "max_block_plus_1_run_9": False,
    "max_block_plus_1_symbol_9": False, "ends_in_four": False,
}


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in B.cases()}


def family(cases, name):
    return [c for c in cases.values() if c.family == name]


def test_libbz2_makes_of_every_case_what_the_case_says(cases):
    declines = {n for n, c in cases.items() if c.expect != "decode"}
    assert declines == set(LIBBZ2_ACCEPTS)
    for n, c in cases.items():
        assert c.expect in ("decode", "decline_or_equal") and c.seam
        if c.expect == "decode" or LIBBZ2_ACCEPTS[n]:
            assert c.want is not None and c.want == c.intended, n
        else:
            assert c.want is None, n
    # inside the decoder's documented scope
    for c in cases.values():
        for b in c.blocks:
            assert len(b.selectors) <= B.BZ_MAX_SELECTORS
    assert sum(len(c.blocks) for c in cases.values() if len(c.marks or ()) <= B.BZ_MARK_CAP) < 700   # 8.6 MB of tables each


def test_magic_cases_sit_on_the_mark_seams(cases):
    for c in family(cases, "magics"):
        assert B.find_marks(c.data) == c.marks, c.name                # no magic-like pattern anywhere else
    c = cases["magic_residues"]
    starts = [bit for bit, _ in c.marks]
    assert {bit % 64 for bit in starts} == set(range(64))             # every o of the kernel's loop
    assert any(bit % 64 > 16 for bit in starts)                       # 48 bits from o > 16: the magic spills into the next unit
    end = c.marks[-1][0]
    assert 8 * (end // 64) + 16 > len(c.data)                         # the end mark's 16-byte read passes the file's end (zero padding)
    assert len(cases["marks_256_one_stream"].marks) == B.BZ_MARK_CAP and len(cases["marks_257_one_stream"].marks) == B.BZ_MARK_CAP + 1
    assert len(cases["marks_256_joined"].marks) == B.BZ_MARK_CAP and len(cases["marks_258_joined"].marks) == B.BZ_MARK_CAP + 2
    for name in ("marks_256_one_stream", "marks_256_joined"):
        offs = np.cumsum([0] + [len(b.out) for b in cases[name].blocks])[:-1]
        assert all(len(b.out) % 2 == 1 for b in cases[name].blocks)
        assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}              # head / word / tail stores of k_bz2_expand


def test_table_cases_sit_on_the_table_seams(cases):
    F = B.BZ_FAST_BITS
    b = cases["len_all_9"].blocks[0]
    assert (b.sym_len == F).all()
    b = cases["len_all_10"].blocks[0]
    assert (b.sym_len == F + 1).all()
    b = cases["len_9_and_10"].blocks[0]
    assert set(b.sym_len.tolist()) == {F, F + 1}
    b = cases["len_all_20"].blocks[0]
    assert (b.sym_len == B.BZ_MAX_CODE_LEN).all()
    for nt in (2, 3, 4, 5, 6):
        b = cases[f"tables_{nt}"].blocks[0]
        assert b.n_tables == nt and b.n_groups >= 2 * nt and len(b.selectors) == b.n_groups
        assert b.selectors == [g % nt for g in range(b.n_groups)]
        assert len({int(l[0]) for l in b.lengths}) == nt
    b = cases["selectors_spare_7"].blocks[0]
    assert len(b.selectors) == b.n_groups + 7
    b = cases["len_1_to_20"].blocks[0]
    assert set(b.lengths[0].tolist()) == set(range(1, 21)) and b.lengths[0][2] == 1
    ones = (b.syms[:B.BZ_GROUP_SYMS * 4] == 2)
    assert ones[1:B.BZ_GROUP_SYMS].all() and ones[B.BZ_GROUP_SYMS:2 * B.BZ_GROUP_SYMS].all()   # 50 one-bit symbols: one window
    assert len(cases["in_use_1"].blocks[0].used) == 1 and len(cases["in_use_256"].blocks[0].used) == 256


def test_symbol_cases_sit_on_the_staging_seams(cases):
    for n in B.RUN_LENGTHS:
        assert B.stage_trace(cases[f"run_{n}_first"].blocks[0])[0] == (0, n, 0)
        b = cases[f"run_{n}_last"].blocks[0]
        assert B.stage_trace(b)[-1][1] == n and b.syms[-2] <= 1        # run, then end of block
        b = cases[f"run_{n}_switch"].blocks[0]
        digits = [i for i in range(1, len(b.syms)) if b.syms[i] <= 1]
        assert digits[0] == B.BZ_GROUP_SYMS - 1 and (n < 3 or digits[-1] >= B.BZ_GROUP_SYMS)
        assert b.sym_table[B.BZ_GROUP_SYMS - 1] != b.sym_table[B.BZ_GROUP_SYMS] and b.lengths[0][0] != b.lengths[1][0]
        assert n in [t[1] for t in B.stage_trace(b)]
    assert {n >= B.RUN_DIRECT for n in B.RUN_LENGTHS} == {True, False} and {63, 64, 65} <= set(B.RUN_LENGTHS)
    for k in (191, 192, 193):                                          # around cnt > 256 - 64
        assert (k, 5) in [t[:2] for t in B.stage_trace(cases[f"stage_{k}_run_5"].blocks[0])]
    sums = set()
    for k, n in ((193, 62), (193, 63), (194, 63), (197, 59), (197, 60)):
        assert (k, n) in [t[:2] for t in B.stage_trace(cases[f"stage_{k}_run_{n}"].blocks[0])]
        sums.add(k + n)
    assert {B.STAGE - 1, B.STAGE, B.STAGE + 1} <= sums                  # cnt + n > 256
    for fill in (192, 224):
        w = []
        B.stage_trace(cases[f"window_starts_at_{fill}"].blocks[0], w)
        assert (fill, B.BZ_GROUP_SYMS + (fill if fill <= B.STAGE_FLUSH else 0)) in w, w[:8]
    assert B.STAGE_FLUSH + B.BZ_GROUP_SYMS <= B.STAGE < 224 + B.BZ_GROUP_SYMS
    for c in family(cases, "symbols"):                                 # (stage_trace asserts that never more than 256 bytes are in flight)
        if len(c.blocks[0].syms) < 20000:
            B.stage_trace(c.blocks[0])
    for level in (1, 9):
        mb = 100000 * level
        b = cases[f"run_ends_at_max_block_{level}"].blocks[0]
        assert len(b.L) == mb and b.syms[-2] <= 1
        assert len(cases[f"max_block_plus_1_run_{level}"].blocks[0].L) == mb + 1
        b = cases[f"max_block_plus_1_symbol_{level}"].blocks[0]
        assert len(b.L) == mb + 1 and b.syms[-2] >= 2
        assert len(cases[f"full_block_{level}"].blocks[0].L) == mb
    n = 900000
    assert (n + B.BZ_SPLIT - 1) // B.BZ_SPLIT + 1 == 3517 <= B.BZ_MAX_SPLIT and (n + B.BZ_TILE - 1) // B.BZ_TILE == B.BZ_MAX_TILES
    assert n + B.STAGE + 255 < B.BZ_LSTRIDE                            # the decliners' last flush stays inside the block's buffer
    for n in (1, 255, 256, 257, 1024, 1025):
        assert len(cases[f"size_{n}"].blocks[0].L) == n
    assert B.sort_segment(1024) == 64 and B.sort_segment(1025) == 128 and B.sort_segment(1) == 64


def test_walk_cases_sit_on_the_splitter_seams(cases):
    n = 100000
    Ks = (n + 255) // 256
    for r in (0, 255, 256, 257, (Ks - 1) * 256, n - 1):
        b = cases[f"orig_{r}"].blocks[0]
        assert b.orig == r and len(b.L) == n and B.walk_model(b.L, b.orig)["period"] == n
    for want in (B.BZ_SEG_CAP - 1, B.BZ_SEG_CAP, B.BZ_SEG_CAP + 1, 2 * B.BZ_SEG_CAP + 1):
        b = cases[f"head_stretch_{want}"].blocks[0]
        m = B.walk_model(b.L, b.orig)
        assert m["head"] == want and m["period"] == n, (want, m["head"])
    for name, period in (("period_1", 1), ("period_5", 5), ("period_5_no_splitter", 5), ("period_256", 256), ("period_512", 512)):
        b = cases[name].blocks[0]
        m = B.walk_model(b.L, b.orig)
        assert m["period"] == period and period < len(b.L), name
        assert (len(m["hits"]) == 0) == (name == "period_5_no_splitter"), name
    assert 5 < B.BZ_SPLIT


def test_rle_cases_sit_on_the_stretch_and_tile_seams(cases):
    for c in family(cases, "rle"):
        if "at" not in c.info:
            continue
        pre, at = c.blocks[0].pre, c.info["at"]
        role = B.rle_layout(pre)[0]
        assert at % B.BZ_RT == 0 and role[at] == c.info["role"], c.name
        slid = B.tile_boundary(pre, at)
        if c.info["role"] < 5:
            assert role[slid] == 5 and pre[slid] != pre[slid - 1], c.name      # the start slides onto the count: the c = 1 entry
        elif c.name.endswith("_same"):
            assert slid > at + 4 and role[slid] == 0, c.name                  # count == value and more of it: the start slides on
        else:
            assert slid == at, c.name
            assert pre[at] == {"other": 3, "zero": 0, "255": 255}[c.name.rsplit("_", 1)[1]]
    pre = cases["all_fb"].blocks[0].pre
    assert len(pre) == 40000 and B.tile_boundary(pre, B.BZ_RT) == len(pre) and B.tile_boundary(pre, B.BZ_TILE) == len(pre)
    assert B.tile_outputs(pre) == [8000 * 255, 0]
    for c in family(cases, "rle"):
        if "tile" in c.info:
            outs = B.tile_outputs(c.blocks[0].pre)
            assert outs[c.info["tile"]] == c.info["out"] and len(outs) == c.info["tile"] + 1, (c.name, outs)
    assert {cases[f"tile_out_{B.BZ_OUTW + d}"].info["out"] for d in (-1, 0, 1)} == {B.BZ_OUTW - 1, B.BZ_OUTW, B.BZ_OUTW + 1}
    b = cases["ends_in_four"].blocks[0]
    assert b.dangling and B.rle_layout(b.pre)[0][-1] == 4
    # four equal bytes as a tile's last four, the count the next tile's first byte
    role = B.rle_layout(cases["tile_on_count_other"].blocks[0].pre)[0]
    assert role[B.BZ_TILE - 1] == 4 and role[B.BZ_TILE] == 5


def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp / name
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *extra, "-o", str(exe), os.path.join(ROOT, "tools", "bz2_core_check.cpp")],
                       capture_output=True, text=True)
    return (str(exe) if r.returncode == 0 else None), r.stderr


def _through_checker(exe, cases, tmp, env=None):
    ran = 0
    for c in cases.values():
        if not c.single_stream:
            continue
        src, dst = tmp / "case.bz2", tmp / "case.out"
        src.write_bytes(c.data)
        r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env)
        assert r.returncode in (0, 3, 4, 5, 6), (c.name, r.returncode, r.stderr[-2000:])     # (anything else: a sanitizer report, a crash)
        if c.expect == "decode":
            assert r.returncode == 0 and dst.read_bytes() == c.want, (c.name, c.seam, r.stderr)
        else:
            assert r.returncode != 0 or (c.want is not None and dst.read_bytes() == c.want), (c.name, c.seam)
        ran += 1
    assert ran > 100


def test_every_single_stream_case_through_the_block_core(cases, tmp_path):
    exe, err = _build(tmp_path, "bz2_core_check", ["-O2"])
    assert exe, err
    _through_checker(exe, cases, tmp_path)
    src = tmp_path / "four.bz2"
    src.write_bytes(cases["ends_in_four"].data)
    r = subprocess.run([exe, str(src), str(tmp_path / "four.out")], capture_output=True, text=True)
    assert r.returncode == 4 and "no count" in r.stderr               # declined, as libbz2 declines it


def test_the_block_core_under_address_and_ub_sanitizers(cases, tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    exe, err = _build(tmp_path, "bz2_core_check_san", san + ["-static-libasan", "-static-libubsan"])   # (runtimes inside the program)
    if exe is None:
        exe, err = _build(tmp_path, "bz2_core_check_san", san)
    if exe is None:
        pytest.skip("no sanitizer runtime: " + err[-200:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    _through_checker(exe, cases, tmp_path, env)
