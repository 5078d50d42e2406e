"""Crafted bzip2 files for the device decoder (lfd_amd/csrc/k_bz2.h, bz2_core.h, bz2dev.hip) and a plain restatement of the
index arithmetic of its kernels.

libbz2's compressor chooses code lengths (never above 17), complete tables, blocks 19 bytes short of their level's size, the
exact selector count and wherever ``orig_ptr`` happens to fall.  The small *writer* here leaves those choices to the case: a
block is given as its bytes before the run-length layer (``pre``; the forward BWT is a cyclic-rotation sort by prefix doubling)
or as the BWT column ``L`` plus ``orig_ptr`` (the output then follows from the inverse permutation walk), with the number of
tables, the selectors, spare selectors and every code length free.  The oracle is never the writer: ``Case.want`` is what
Python's ``bz2`` (libbz2) makes of the file, ``None`` where it raises.  ``expect`` is "decode" (libbz2 accepts and the file is
inside the decoder's documented scope: status 0 and the same bytes) or "decline_or_equal".

The second half restates what the kernels compute with their constants -- mark residues (k_bz2_magics), the staging fill at
every run (bz_dev_symbols / BzDevIO), the walk from ``orig_ptr`` to the first splitter and the cycle length (k_bz2_walk), the
slide of a nominal stretch start and the bytes a tile writes (k_bz2_rle_*, k_bz2_expand) -- so that
tests/test_bz2_cases_model.py can prove on the CPU that every case sits on the seam it names; tests/test_gpu_bz2_seams.py runs
them on the device.
"""
import bisect
import bz2
import zlib

import numpy as np

# constants of bz2_core.h / k_bz2.h that the cases sit on
BZ_FAST_BITS = 9
BZ_GROUP_SYMS = 50
BZ_MAX_SELECTORS = 18002
BZ_MAX_CODE_LEN = 20
BZ_LSTRIDE = 900608
BZ_SPLIT = 256
BZ_MAX_SPLIT = 3520
BZ_MARK_CAP = 256
BZ_SEG_CAP = 1024
BZ_RT = 32
BZ_TILE = 1024 * BZ_RT
BZ_MAX_TILES = 28
BZ_OUTW = 36 * 1024
STAGE = 256                      # bytes of BzDevIO::stage
STAGE_FLUSH = 256 - 64           # `if (io.cnt > 256 - 64) io.flush()`
RUN_DIRECT = 64                  # emit_run: n >= 64 goes straight to memory

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
_REV8 = bytes(int(f"{i:08b}"[::-1], 2) for i in range(256))


def crc32_bz(data):
    """bzip2's CRC (polynomial 0x04c11db7, most significant bit first) from zlib's reflected one."""
    r = zlib.crc32(bytes(data).translate(_REV8)) & 0xFFFFFFFF
    return int(f"{r:032b}"[::-1], 2)


# ---- bit writer -----------------------------------------------------------------------------------------------------------

class Bits:
    """(value, width) pairs, expanded to bits in chunks when the bytes are asked for."""

    def __init__(self):
        self.parts, self.pv, self.pl, self.nbits = [], [], [], 0

    def put(self, value, width):
        self.pv.append(int(value))
        self.pl.append(int(width))
        self.nbits += int(width)

    def _close(self):
        if self.pv:
            self.parts.append((np.array(self.pv, np.int64), np.array(self.pl, np.int64)))
            self.pv, self.pl = [], []

    def put_many(self, values, widths):
        self._close()
        v, l = np.asarray(values, np.int64), np.asarray(widths, np.int64)
        self.parts.append((v, l))
        self.nbits += int(l.sum())

    def extend(self, other):
        self._close()
        other._close()
        self.parts += other.parts
        self.nbits += other.nbits

    def pad_to_byte(self):
        if self.nbits & 7:
            self.put(0, 8 - (self.nbits & 7))

    def tobytes(self, chunk=1 << 16):
        self._close()
        out = []
        for v, l in self.parts:
            for i in range(0, len(v), chunk):
                vv, ll = v[i:i + chunk], l[i:i + chunk]
                tot = int(ll.sum())
                first = np.cumsum(ll) - ll
                within = np.arange(tot, dtype=np.int64) - np.repeat(first, ll)
                out.append(((np.repeat(vv, ll) >> (np.repeat(ll, ll) - 1 - within)) & 1).astype(np.uint8))
        return np.packbits(np.concatenate(out)).tobytes() if out else b""


# ---- the layers of a block ------------------------------------------------------------------------------------------------

def bwt(pre):
    """Forward BWT by sorting the cyclic rotations (prefix doubling, np.lexsort): (L, orig_ptr, order).  Equal rotations
    (periodic data) keep their index order."""
    a = np.frombuffer(bytes(pre), np.uint8).astype(np.int64)
    n = len(a)
    idx = np.arange(n)
    rank, k = a.copy(), 1
    while n > 1:
        r2 = rank[(idx + k) % n]
        order = np.lexsort((r2, rank))
        ro, r2o = rank[order], r2[order]
        new = np.empty(n, np.int64)
        new[order] = np.cumsum(np.r_[0, ((ro[1:] != ro[:-1]) | (r2o[1:] != r2o[:-1])).astype(np.int64)])
        rank, k = new, k * 2
        if rank.max() == n - 1 or k >= n:
            break
    order = np.lexsort((idx, rank))
    return a[(order - 1) % n].astype(np.uint8), int(np.flatnonzero(order == 0)[0]), order


def tt_perm(L):
    """k_bz2_sort: tt[q] >> 8 for every q (a stable counting sort of the column)."""
    return np.argsort(np.asarray(L, np.uint8), kind="stable")


def walk_seq(L, orig, steps):
    """q_0 = orig_ptr, q_{j+1} = tt[q_j] >> 8 for j < steps (pointer doubling)."""
    T = tt_perm(L)
    seq, J = np.array([orig], np.int64), T
    while len(seq) < steps:
        seq = np.concatenate([seq, J[seq]])
        J = J[J]
    return seq[:steps], T


def inverse_bwt(L, orig):
    L = np.asarray(L, np.uint8)
    seq, T = walk_seq(L, orig, len(L))
    return L[T[seq]]


def rle_layout(pre):
    """The run-length layer read sequentially: (role, reps, vals, dangling).  role: 1..4 = the bytes of a run of four, 5 = its
    count, 0 = anything else; the output is np.repeat(vals, reps); dangling = the block ends right after four equal bytes."""
    a = np.frombuffer(bytes(pre), np.uint8)
    n = len(a)
    role = np.zeros(n, np.int8)
    reps, vals = np.ones(n, np.int64), a.copy()
    dangling = False
    if n >= 4:
        idx4 = np.flatnonzero((a[:-3] == a[1:-2]) & (a[1:-2] == a[2:-1]) & (a[2:-1] == a[3:])).tolist()
        p = 0
        while True:
            k = bisect.bisect_left(idx4, p)
            if k == len(idx4):
                break
            j = idx4[k]
            role[j:j + 4] = (1, 2, 3, 4)
            if j + 4 >= n:
                dangling = True
                break
            role[j + 4] = 5
            reps[j + 4], vals[j + 4] = a[j + 4], a[j]
            p = j + 5
    return role, reps, vals, dangling


def rle_decode(pre):
    _, reps, vals, dangling = rle_layout(pre)
    return np.repeat(vals, reps).tobytes(), dangling


_SYM_CACHE = {}


def mtf_symbols(L):
    """Move-to-front + RUNA / RUNB: (symbols incl. end of block, used byte values)."""
    L = np.asarray(L, np.uint8)
    key = (len(L), zlib.crc32(L.tobytes()))
    if key in _SYM_CACHE:
        return _SYM_CACHE[key]
    used = np.unique(L)
    index = np.zeros(256, np.int64)
    index[used] = np.arange(len(used))
    starts = np.flatnonzero(np.r_[True, L[1:] != L[:-1]])
    lens = np.diff(np.r_[starts, len(L)]).tolist()
    heads = index[L[starts]].tolist()
    lst = bytearray(range(len(used)))
    syms, zrun = [], 0

    def flush(n):
        while n > 0:
            if n & 1:
                syms.append(0)
                n = (n - 1) >> 1
            else:
                syms.append(1)
                n = (n - 2) >> 1
    for v, m in zip(heads, lens):
        p = lst.index(v)
        if p == 0:
            zrun += m
        else:
            flush(zrun)
            syms.append(p + 1)
            del lst[p]
            lst.insert(0, v)
            zrun = m - 1
    flush(zrun)
    syms.append(len(used) + 1)
    _SYM_CACHE[key] = (np.array(syms, np.int64), used)
    return _SYM_CACHE[key]


def canonical_codes(lengths):
    """bzip2's code assignment: by length, then by symbol.  Incomplete tables are fine, over-subscribed ones are not."""
    ln = np.asarray(lengths, np.int64)
    assert ln.min() >= 1 and ln.max() <= BZ_MAX_CODE_LEN
    assert sum(2.0 ** -int(x) for x in ln) <= 1.0, "over-subscribed code"
    codes = np.zeros(len(ln), np.int64)
    vec = 0
    for n in range(int(ln.min()), int(ln.max()) + 1):
        for i in np.flatnonzero(ln == n):
            codes[i] = vec
            vec += 1
        vec <<= 1
    return codes


def fixed_len(alpha):
    return max(2, int(np.ceil(np.log2(alpha))))


class Block:
    """One block, written.  Give ``pre`` (bytes before the run-length layer) or ``L`` and ``orig`` (``orig="auto"``: the first
    orig_ptr whose output does not end right after four equal bytes).  ``lengths``: None (one fixed length, the shortest that
    holds the alphabet), a list with one int per table (fixed lengths) or per table an array of alpha lengths, or a callable
    (alpha, symbols) -> such a list.  ``selectors``: None = tables cycling group by group."""

    def __init__(self, pre=None, L=None, orig=None, n_tables=2, lengths=None, selectors=None, spare=0, allow_dangling=False):
        if L is None:
            self.pre = bytes(pre)
            self.L, self.orig, _ = bwt(self.pre)
        else:
            self.L = np.frombuffer(bytes(L), np.uint8) if not isinstance(L, np.ndarray) else L.astype(np.uint8)
            cand = range(len(self.L)) if orig == "auto" else [int(orig)]
            for o in cand:
                self.orig, self.pre = o, inverse_bwt(self.L, o).tobytes() if pre is None else bytes(pre)
                if allow_dangling or not rle_layout(self.pre)[3]:
                    break
        self.out, self.dangling = rle_decode(self.pre)
        assert allow_dangling or not self.dangling
        self.crc = crc32_bz(self.out)
        self.syms, self.used = mtf_symbols(self.L)
        alpha = len(self.used) + 2
        self.n_groups = -(-len(self.syms) // BZ_GROUP_SYMS)
        self.selectors = list(selectors) if selectors is not None else [g % n_tables for g in range(self.n_groups)]
        assert len(self.selectors) >= self.n_groups
        self.selectors += [0] * spare
        assert 1 <= len(self.selectors) <= 32767
        if callable(lengths):
            lengths = lengths(alpha, self.syms)
        if lengths is None:
            lengths = [fixed_len(alpha)] * n_tables
        self.lengths = [np.full(alpha, l, np.int64) if np.isscalar(l) else np.asarray(l, np.int64) for l in lengths]
        assert len(self.lengths) == n_tables and all(len(l) == alpha for l in self.lengths)
        self.n_tables = n_tables
        tab = np.array(self.selectors[:self.n_groups], np.int64)[np.arange(len(self.syms)) // BZ_GROUP_SYMS]
        self.sym_table = tab
        self.sym_len = np.stack(self.lengths)[tab, self.syms]
        self.bits = self._write(np.stack([canonical_codes(l) for l in self.lengths])[tab, self.syms])

    def _write(self, codes):
        w = Bits()
        w.put(BLOCK_MAGIC, 48)
        w.put(self.crc, 32)
        w.put(0, 1)
        w.put(self.orig, 24)
        present = np.zeros(256, bool)
        present[self.used] = True
        rows = present.reshape(16, 16)
        w.put(int("".join("1" if r.any() else "0" for r in rows), 2), 16)
        for r in rows:
            if r.any():
                w.put(int("".join("1" if x else "0" for x in r), 2), 16)
        w.put(self.n_tables, 3)
        w.put(len(self.selectors), 15)
        order = list(range(self.n_tables))
        for s in self.selectors:
            j = order.index(s)
            w.put((1 << (j + 1)) - 2, j + 1)                         # j ones and a zero
            order.insert(0, order.pop(j))
        for ln in self.lengths:
            cur = int(ln[0])
            w.put(cur, 5)
            for x in ln.tolist():
                while cur != x:
                    w.put(2 if x > cur else 3, 2)
                    cur += 1 if x > cur else -1
                w.put(0, 1)
        w.put_many(codes, self.sym_len)
        return w


def write_file(streams):
    """streams: [(level, [Block, ...]), ...] -> (bytes, marks): marks = (bit offset, is_end_mark) of every magic."""
    w, marks = Bits(), []
    for level, blocks in streams:
        w.put(int.from_bytes(b"BZh" + str(level).encode(), "big"), 32)
        comb = 0
        for b in blocks:
            marks.append((w.nbits, 0))
            w.extend(b.bits)
            comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ b.crc
        marks.append((w.nbits, 1))
        w.put(END_MAGIC, 48)
        w.put(comb, 32)
        w.pad_to_byte()
    return w.tobytes(), marks


# ---- restatement of the kernels' index arithmetic -------------------------------------------------------------------------

def find_marks(data):
    """k_bz2_magics: every 48-bit magic at any bit offset that ends inside the file -> [(bit, is_end)] in file order."""
    bits = np.unpackbits(np.frombuffer(data, np.uint8))
    out = []
    for magic, end in ((BLOCK_MAGIC, 0), (END_MAGIC, 1)):
        pat = np.array([(magic >> (47 - i)) & 1 for i in range(48)], np.uint8)
        ok = np.ones(len(bits) - 47, bool)
        for i in range(48):
            ok &= bits[i:len(bits) - 47 + i] == pat[i]
        out += [(int(b), end) for b in np.flatnonzero(ok)]
    return sorted(out)


def stage_trace(block, windows=None):
    """bz_dev_symbols: the staging buffer's fill when each run arrives -> [(cnt, run length, flushed)]; also checks the
    window loop's own promise (never more than 256 bytes in flight).  ``windows``: a list that receives (fill at the start of a
    64-bit window, before its flush; fill at its end)."""
    syms, lens = block.syms.tolist(), block.sym_len.tolist()
    eob = len(block.used) + 1
    cnt = flushed = 0
    i, group_pos, run_n, run_len = 0, 0, 0, 0
    trace = []
    while True:
        if group_pos == 0:
            group_pos = BZ_GROUP_SYMS
        start = cnt
        if cnt > STAGE_FLUSH:
            flushed, cnt = flushed + cnt, 0
        pos = 0
        done = False
        while True:
            window_over = False
            while run_n == 0 and 2 <= syms[i] < eob and lens[i] <= BZ_FAST_BITS:      # the ordinary symbols
                pos += lens[i]
                i += 1
                cnt += 1
                group_pos -= 1
                if group_pos == 0 or pos >= 64:
                    window_over = True
                    break
            assert cnt <= STAGE
            if window_over:
                break
            s = syms[i]
            pos += lens[i]
            i += 1
            if s <= 1:
                if run_n == 0:
                    run_n, run_len = 1, 0
                run_len += run_n << s
                run_n <<= 1
            else:
                if run_n:
                    trace.append((cnt, run_len, flushed))
                    if run_len >= RUN_DIRECT:
                        flushed, cnt = flushed + cnt + run_len, 0
                    else:
                        if cnt + run_len > STAGE:
                            flushed, cnt = flushed + cnt, 0
                        cnt += run_len
                    run_n = 0
                    if cnt > STAGE_FLUSH:
                        flushed, cnt = flushed + cnt, 0
                if s == eob:
                    done = True
                    break
                cnt += 1
            assert cnt <= STAGE
            group_pos -= 1
            if group_pos == 0 or pos >= 64:
                break
        if windows is not None:
            windows.append((start, cnt))
        if done:
            assert flushed + cnt == len(block.L)
            return trace


def sort_segment(n):
    """k_bz2_sort: positions per wave."""
    return (((n + 15) // 16) + 63) & ~63


def walk_model(L, orig):
    """k_bz2_walk: (Ks, head stretch length, cycle length through orig_ptr, splitter gaps along that cycle)."""
    n = len(L)
    seq, T = walk_seq(L, orig, n + 1)
    back = np.flatnonzero(seq[1:] == orig)
    period = int(back[0]) + 1
    stops = np.flatnonzero((seq[1:period + 1] % BZ_SPLIT == 0) | (seq[1:period + 1] == orig)) + 1
    on_cycle = np.flatnonzero(seq[:period] % BZ_SPLIT == 0)
    return dict(Ks=(n + BZ_SPLIT - 1) // BZ_SPLIT, head=int(stops[0]), period=period, seq=seq, hits=on_cycle)


def tile_boundary(pre, start):
    """bz_tile_boundary: the first position >= start where a run of equal bytes starts."""
    n = len(pre)
    p = min(n, start)
    while 0 < p < n and pre[p] == pre[p - 1]:
        p += 1
    return p


def tile_outputs(pre):
    """bytes every 32 kB tile writes (k_bz2_rle_tiles / k_bz2_expand under the true entry state)."""
    _, reps, _, _ = rle_layout(pre)
    n = len(pre)
    nt = (n + BZ_TILE - 1) // BZ_TILE
    b = [tile_boundary(pre, t * BZ_TILE) for t in range(nt + 1)]
    return [int(reps[b[t]:b[t + 1]].sum()) for t in range(nt)]


# ---- the cases --------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, family, seam, streams, expect="decode", **info):
        self.name, self.family, self.seam, self.expect, self.info = name, family, seam, expect, info
        self.streams = streams
        self.data, self.marks = write_file(streams)
        self.blocks = [b for _, bl in streams for b in bl]
        self.intended = b"".join(b.out for b in self.blocks)
        try:
            self.want = bz2.decompress(self.data)
        except (OSError, ValueError, EOFError):
            self.want = None

    @property
    def single_stream(self):
        return len(self.streams) == 1

    def __repr__(self):
        return f"<{self.name}: {self.seam}>"


def no_repeat_bytes(rng, n, lo=0, hi=256):
    """n bytes, no two neighbours equal (nothing for the run-length layer to find)."""
    step = rng.integers(1, hi - lo, n)
    return ((np.cumsum(step) % (hi - lo)) + lo).astype(np.uint8).tobytes()


RUN_LENGTHS = (1, 2, 3, 62, 63, 64, 65, 127, 128, 129, 255, 256, 257, 70000)
WALK_SEED = 2            # seeds 0 and 1 have no gap between splitters above 2 049 steps (1 203, 1 299); this one has 2 394


def _cycling(k, lo=1, m=8):
    """k bytes lo, lo + 1, ... cycling through m values: every one is an ordinary symbol at list position m - 1 (after the start)."""
    return bytes(lo + (i % m) for i in range(k))


def _magic_cases():
    out = []
    # candidates of every bit length residue: d distinct values, m bytes
    cands = []
    for d in range(1, 7):
        for m in range(d, d + 9):
            cands.append(bytes(97 + (i % d) for i in range(m)) if d > 1 else b"a" * min(m, 3))
    cands = list(dict.fromkeys(cands))
    blocks_of = {c: Block(pre=c) for c in cands}
    pos, seen, blocks = 32, set(), []
    while len(blocks) < 130:
        seen.add(pos % 64)
        pick = next((c for c in cands if (pos + blocks_of[c].bits.nbits) % 64 not in seen), cands[len(blocks) % len(cands)])
        blocks.append(blocks_of[pick])
        pos += blocks_of[pick].bits.nbits
    out.append(Case("magic_residues", "magics", "k_bz2_magics: a magic at every o = 0..63 of the 64-bit loop, spills into the next unit",
                    [(1, blocks)]))
    tiny = [Block(pre=bytes([65 + (k % 7)]) * (1 + 2 * (k % 3)) if k % 3 < 2 else _cycling(5, 65 + k % 7, 5)) for k in range(256)]
    out.append(Case("marks_256_one_stream", "magics", "BZ_MARK_CAP: 255 blocks + end mark = 256 marks", [(1, tiny[:255])]))
    out.append(Case("marks_257_one_stream", "magics", "BZ_MARK_CAP + 1: 256 blocks + end mark", [(1, tiny[:256])],
                    expect="decline_or_equal"))
    out.append(Case("marks_256_joined", "magics", "BZ_MARK_CAP as 128 one-block streams; block offsets 1, 2, 3 mod 4 (k_bz2_expand head / tail)",
                    [(1 + k % 9, [tiny[k]]) for k in range(128)]))
    out.append(Case("marks_258_joined", "magics", "129 one-block streams: 258 marks > BZ_MARK_CAP",
                    [(1 + k % 9, [tiny[k]]) for k in range(129)], expect="decline_or_equal"))
    return out


def _table_cases():
    rng = np.random.default_rng(21)
    pre = rng.integers(0, 200, 3000).astype(np.uint8).tobytes()
    out = []

    def add(name, seam, **kw):
        out.append(Case(name, "tables", seam, [(1, [Block(pre=pre, **kw)])]))
    add("len_all_9", "every code BZ_FAST_BITS long: the fast table alone", lengths=[9, 9])
    add("len_all_10", "every code BZ_FAST_BITS + 1: fast table all zero, bz_slow_symbol for every symbol", lengths=[10, 10])
    add("len_9_and_10", "codes of BZ_FAST_BITS and BZ_FAST_BITS + 1 mixed in one table",
        lengths=lambda alpha, s: [np.where(np.arange(alpha) % 2 == 0, 9, 10)] * 2)
    add("len_all_20", "every code BZ_MAX_CODE_LEN long", lengths=[20, 20])
    for nt in (2, 3, 4, 5, 6):
        add(f"tables_{nt}", f"{nt} tables of lengths 9 .. {8 + nt}, the selector cycling every group of BZ_GROUP_SYMS",
            n_tables=nt, lengths=list(range(9, 9 + nt)))
    add("selectors_spare_7", "7 selectors more than the groups need", n_tables=6, lengths=list(range(8, 14)), spare=7)
    # lengths 1 .. 20 in one table, the 1-bit code on the commonest ordinary symbol: L = "abab..." is one symbol (list position 1)
    L = b"ab" * 3000 + bytes(range(99, 99 + 17))

    def one_to_twenty(alpha, syms):
        assert alpha == 21
        ln = np.zeros(alpha, np.int64)
        ln[2] = 1
        ln[[i for i in range(alpha) if i != 2]] = list(range(2, 21)) + [20]
        return [ln, ln]
    out.append(Case("len_1_to_20", "tables", "lengths 1 .. BZ_MAX_CODE_LEN in one table; BZ_GROUP_SYMS one-bit symbols in one 64-bit window",
                    [(1, [Block(L=L, orig="auto", lengths=one_to_twenty)])]))
    out.append(Case("in_use_1", "tables", "n_in_use 1: alpha 3", [(1, [Block(pre=b"zzz")])]))
    allb = np.random.default_rng(5).permutation(np.tile(np.arange(256, dtype=np.uint8), 4)).tobytes()
    out.append(Case("in_use_256", "tables", "n_in_use 256: alpha 258, all 64 lanes of the move-to-front list", [(1, [Block(pre=allb)])]))
    return out


def _symbol_cases():
    out = []
    two = dict(n_tables=2, lengths=[9, 5])          # the second table has another length: a digit decoded under the wrong one breaks

    def add(name, seam, L, expect="decode", level=1, **kw):
        b = Block(L=L, orig="auto", allow_dangling=expect != "decode", **kw)
        out.append(Case(name, "symbols", seam, [(level, [b])], expect=expect))
    for n in RUN_LENGTHS:
        add(f"run_{n}_first", "a run as the block's first symbols (emit_run n >= 64 direct path / staging)", bytes(n) + _cycling(20))
        add(f"run_{n}_last", "a run, then end of block", _cycling(20) + bytes([4]) * n)
        # 49 ordinary symbols, then the run's digits: the first is the group's 50th symbol, the rest come under the next table
        add(f"run_{n}_switch", "run digits on both sides of a BZ_GROUP_SYMS table switch", _cycling(49) + bytes([1]) * n + _cycling(9, 2), **two)
    # Staging fill: the fill is looked at where a 64-bit window starts, and a window ends with its table's BZ_GROUP_SYMS symbols,
    # so a fill above 256 - 64 needs many symbols in one window: a one-bit code on the only ordinary symbol ("baba...": list
    # position 1), three bits on everything else.  Seven bytes from three digits first: the fill is the symbol index + 5, and the
    # run's digits and the symbol that closes it still belong to the window that starts at symbol 150.
    def staged(k, n):
        L = b"\x01" * 7 + bytes(2 - (i & 1) for i in range(k - 7))
        return L + L[-1:] * n + b"\x03"
    short = dict(lengths=[[3, 3, 1, 3, 3]] * 2)
    for k in (191, 192, 193):
        add(f"stage_{k}_run_5", f"a run arriving at cnt = {k} (cnt > 256 - 64 flush)", staged(k, 5), **short)
    for k, n in ((193, 62), (193, 63), (194, 63), (197, 59), (197, 60)):
        add(f"stage_{k}_run_{n}", f"cnt + n = {k + n} against 256 (cnt + n > 256 flush)", staged(k, n), **short)
    # a window that starts at a fill of exactly 256 - 64 (no flush) and then takes its table's 50 one-bit symbols: 242 bytes in
    # flight, the most the loop can hold; and one that starts at 224, which a flush at 256 - 32 would let run to 274
    # (ten two-bit symbols among each table's 50, in no regular order: bytes that a lost flush cannot reproduce by chance)
    mixed = dict(lengths=[[4, 4, 1, 2, 4, 4]] * 2)
    rng = np.random.default_rng(61)
    for r, fill in ((47, 192), (28, 224)):
        lst, body = [1, 2, 3], []
        for g in range(1, 9):
            two = set(rng.choice(BZ_GROUP_SYMS, 10, replace=False).tolist())
            for i in range(BZ_GROUP_SYMS):
                lst.insert(0, lst.pop(2 if i in two else 1))
                body.append(lst[0])
        lead = BZ_GROUP_SYMS - len(mtf_symbols(np.frombuffer(b"\x01" * r + b"\x02", np.uint8))[0]) + 2      # group 0: the digits, then "2121..."
        add(f"window_starts_at_{fill}", f"a window of BZ_GROUP_SYMS short symbols starting at cnt = {fill} (cnt > 256 - 64)",
            b"\x01" * r + bytes(2 - (i & 1) for i in range(lead)) + bytes(body) + b"\x04", **mixed)
    # block sizes: exactly max_block, and one more (the decliners stay inside BZ_LSTRIDE: a refused run writes nothing, an
    # ordinary symbol too many leaves flushed + 255 <= max_block + 256 + 255 = 900 511 < 900 608 at the last flush)
    for level in (1, 9):
        mb = 100000 * level
        head = _cycling(193)
        add(f"run_ends_at_max_block_{level}", "a last run that ends exactly at max_block", head + bytes([head[-1]]) * (mb - 193), level=level)
        add(f"max_block_plus_1_run_{level}", "max_block + 1 by a run", head + bytes([head[-1]]) * (mb - 192), level=level,
            expect="decline_or_equal")
        add(f"max_block_plus_1_symbol_{level}", "max_block + 1 by an ordinary symbol", head + bytes([head[-1]]) * (mb - 193) + b"\x02",
            level=level, expect="decline_or_equal")
    rng = np.random.default_rng(31)
    out.append(Case("full_block_1", "symbols", "a block of exactly max_block = 100 000 bytes (the compressor stops 19 short)",
                    [(1, [Block(pre=rng.integers(0, 256, 100000).astype(np.uint8).tobytes())])]))
    out.append(Case("full_block_9", "symbols", "max_block = 900 000: 3 516 + 1 splitters of BZ_MAX_SPLIT, all BZ_MAX_TILES tiles, BZ_LSTRIDE slack",
                    [(9, [Block(pre=rng.integers(0, 4, 900000).astype(np.uint8).tobytes())])]))
    for n in (1, 255, 256, 257, 1024, 1025):
        out.append(Case(f"size_{n}", "symbols", f"nblock {n}: k_bz2_sort segment {sort_segment(n)}, Ks {(n + 255) // 256}",
                        [(1, [Block(pre=rng.integers(0, 256, n).astype(np.uint8).tobytes())])]))
    return out


def walk_base(seed=None):
    rng = np.random.default_rng(WALK_SEED if seed is None else seed)
    pre = rng.integers(0, 256, 100000).astype(np.uint8).tobytes()
    L, orig, order = bwt(pre)
    return pre, L, orig, order


def _walk_cases():
    out = []
    pre, L, orig, order = walk_base()
    n = len(L)
    Ks = (n + 255) // 256

    def at_rank(name, seam, r):
        s = int(order[r])                                             # the rotation whose rank is r
        out.append(Case(name, "walk", seam, [(1, [Block(pre=pre[s:] + pre[:s], L=L, orig=r)])], orig=r))
    for r in (0, 255, 256, 257, (Ks - 1) * 256, n - 1):
        at_rank(f"orig_{r}", f"orig_ptr {r}: on / beside a regular splitter (BZ_SPLIT_LOG), first and last rank", r)
    m = walk_model(L, orig)
    hits, seq = m["hits"], m["seq"]
    gaps = np.diff(np.r_[hits, hits[0] + n])
    g = int(np.argmax(gaps))
    end = int(hits[g] + gaps[g])                                      # cycle index of the splitter that closes the longest gap
    for want in (BZ_SEG_CAP - 1, BZ_SEG_CAP, BZ_SEG_CAP + 1, 2 * BZ_SEG_CAP + 1):
        assert gaps[g] > want, "WALK_SEED: the longest gap is too short"
        at_rank(f"head_stretch_{want}", f"head stretch of {want} steps against BZ_SEG_CAP", int(seq[(end - want) % n]))
    rng = np.random.default_rng(41)
    out.append(Case("period_1", "walk", "cycle of 1 through orig_ptr", [(1, [Block(pre=b"\x07" * 3000)])]))
    out.append(Case("period_5", "walk", "cycle of 5; splitter 0 on it", [(1, [Block(pre=b"abcde" * 600)])]))
    L5, o5, _ = bwt(b"abcde" * 600)
    out.append(Case("period_5_no_splitter", "walk", "cycle of 5 through orig_ptr with no multiple of 256 on it: the head alone",
                    [(1, [Block(L=L5, orig=o5 + 1)])]))
    for p in (256, 512):
        unit = no_repeat_bytes(rng, p)
        out.append(Case(f"period_{p}", "walk", f"cycle of {p} = {p // 256} x the splitter distance", [(1, [Block(pre=unit * 8)])]))
    return out


def _rle_cases():
    out = []
    rng = np.random.default_rng(51)

    def add(name, seam, pre, expect="decode", **info):
        out.append(Case(name, "rle", seam, [(1, [Block(pre=pre, allow_dangling=expect != "decode")])], expect=expect, **info))

    def filler(n, avoid):
        f = bytearray(no_repeat_bytes(rng, n, 0, 200))
        if n and f[-1] == avoid:
            f[-1] = 199 if avoid != 199 else 198
            if n > 1 and f[-2] == f[-1]:
                f[-2] = 197
        return bytes(f)
    # a run of four whose j-th byte (2, 3, 4) or count (5) lies on a nominal stretch start (a multiple of BZ_RT) and on a tile
    # start (BZ_TILE); kinds of count: another value (c = 1 entry), the run's own value with more of it behind (the start
    # slides), 0, 255
    for B, tag in ((32 * 7, "stretch"), (BZ_TILE, "tile")):
        for j in (2, 3, 4):
            start = B - (j - 1)
            pre = filler(start, 0xE0) + b"\xE0" * 4 + b"\x03" + filler(B + 100 - start - 5, 0xFF)
            add(f"{tag}_on_byte_{j}", f"a multiple of {'BZ_RT' if tag == 'stretch' else 'BZ_TILE'} on byte {j} of a run of four", pre, at=B, role=j)
        start = B - 4
        for kind, count, more in (("other", 3, b""), ("same", 0xE0, b"\xE0" * 6), ("zero", 0, b""), ("255", 255, b"")):
            pre = filler(start, 0xE0) + b"\xE0" * 4 + bytes([count]) + more + b"\xF0" + filler(B + 100 - start - 6 - len(more), 0xFF)
            add(f"{tag}_on_count_{kind}", f"a multiple of {'BZ_RT' if tag == 'stretch' else 'BZ_TILE'} on the count byte ({kind})", pre, at=B, role=5)
    add("all_fb", "40 000 x 0xFB: one stretch spans two tiles, all others empty, the carry passes through a tile", b"\xFB" * 40000)
    # tile 1 writes BZ_OUTW - 1, BZ_OUTW, BZ_OUTW + 1 bytes: 17 groups of (four + count 255) = 259 bytes each, literals for the rest
    for d in (-1, 0, 1):
        target = BZ_OUTW + d
        body = b"".join(bytes([0xD0 + (i & 1)]) * 4 + b"\xFF" for i in range(17)) + b"\xC0"      # 17 * 259 + 1 from 86 bytes
        lit = target - (17 * 259 + 1)                                 # 86 + lit <= BZ_TILE: tile 1 is the block's last
        pre = filler(BZ_TILE, 0xD0) + body + filler(lit, 0xFF)
        add(f"tile_out_{target}", f"a tile writing {target} bytes against BZ_OUTW = {BZ_OUTW}", pre, tile=1, out=target)
    pre = filler(BZ_TILE, 0xD0) + b"".join(bytes([0xD0 + (i & 1)]) * 4 + b"\xFF" for i in range(6000))
    add("tile_out_far_above", "a tile far above BZ_OUTW (all counts 255): direct stores", pre, tile=1, out=6000 * 259)
    add("ends_in_four", "the block ends right after four equal bytes: no count (libbz2 declines)", filler(500, 0xE0) + b"\xE0" * 4,
        expect="decline_or_equal")
    base = np.random.default_rng(99)
    base.integers(0, 256, 150000, dtype=np.uint8)
    few = bytes(base.integers(0, 4, 200000, dtype=np.uint8))
    runs = b"".join(bytes([b]) * int(n) for b, n in zip(base.integers(0, 256, 3000), base.integers(1, 300, 3000)))
    for name, plain in (("base_four_symbols", few), ("base_run_heavy", runs)):
        c = Case.__new__(Case)
        c.name, c.family, c.seam, c.expect, c.info = name, "rle", "undamaged base of the damaged-files test, written by libbz2", "decode", {}
        c.streams, c.blocks, c.marks, c.data, c.intended, c.want = [None], [], None, bz2.compress(plain, 9), plain, plain
        out.append(c)
    return out


_CASES = None


def cases():
    """Every case, built once per process."""
    global _CASES
    if _CASES is None:
        _CASES = _magic_cases() + _table_cases() + _symbol_cases() + _walk_cases() + _rle_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES
