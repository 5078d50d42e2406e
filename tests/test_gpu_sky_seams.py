"""lfdmi_sky_normalize (k_sky.h, sky.hip) on the named frames of tests/sky_cases.py: the widths the radix selection can be left
with, live counts around its ranks and around area / 8, pixels on the closed clip interval, meshes of 1 to 289 cells and their
empty cells, every cell edge at which the cell copy or the loads change path, and the column spans and row intervals of the
apply kernel -- records, both meshes and every output pixel bit for bit against tests/sky_ref.py, on device, host, big-endian
and handle-buffer routes, and again from and to device memory that is not 16-byte aligned.  tests/test_sky_cases_model.py
proves on the CPU that every case sits on the seam it names."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sky_cases as K  # noqa: E402
import sky_ref as S  # noqa: E402
from test_gpu_sky import bits, same_rec  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 12345.0
# groups that also go through the handle's own buffer (with the big-endian ones)
HANDLE_ROUTE = {"sel_rem_32_c1", "sel_m_257_c0", "cell_128_w4_130x260", "cell_129_w4_140x260", "cell_256_flip_global_100x256",
                "empty_edge_full_31_empty_f3", "clip_edge_M1000_c2", "mesh_17x17_f3_m1", "mesh_ring_of_empties_f1_m0"}


class Group:
    """the cases of one (shape, params, slots): one handle, their frames as one batch"""

    def __init__(self, ctx, cs):
        from lfd_amd import _native
        self.cases = cs
        self.frames = np.concatenate([c.frames for c in cs])
        self.shape = self.frames.shape[1:]
        self.names = [f"{c.name}[{k}]" for c in cs for k in range(len(c.frames))]
        self.slots = K.MAX_FRAMES.get(cs[0].name) or len(self.frames)
        self.sky = _native.Sky(ctx, self.shape, max_frames=self.slots, **cs[0].params)


@pytest.fixture(scope="module")
def groups(gpu_ctx):
    by_key = {}
    for c in K.cases():
        by_key.setdefault((c.frames.shape[1:], tuple(sorted(c.params.items())), K.MAX_FRAMES.get(c.name)), []).append(c)
    made = [Group(gpu_ctx, cs) for cs in by_key.values()]
    assert sum(len(g.cases) for g in made) == len(K.cases())
    yield made
    for g in made:
        g.sky.close()


@pytest.fixture(scope="module")
def ref():
    """the restatement of every frame of every case, once: name -> [(out, record, sky mesh, sigma mesh)]"""
    return {c.name: [S.normalize(x, **c.params) for x in c.frames] for c in K.cases()}


def failures(g, ref, out, rec, mb, ms):
    """one line per frame of the group that is not the restatement's"""
    want = [r for c in g.cases for r in ref[c.name]]
    bad = []
    for i, (name, (w_out, w_rec, w_mb, w_ms)) in enumerate(zip(g.names, want)):
        msg = same_rec(rec[i], w_rec)
        if msg is None and not np.array_equal(bits(mb[i]), bits(w_mb)):
            msg = f"sky mesh differs: device {mb[i].ravel()[:4]} restatement {w_mb.ravel()[:4]}"
        if msg is None and not np.array_equal(bits(ms[i]), bits(w_ms)):
            msg = f"sigma mesh differs: device {ms[i].ravel()[:4]} restatement {w_ms.ravel()[:4]}"
        if msg is None and not np.array_equal(bits(out[i]), bits(w_out)):
            d = np.argwhere(bits(out[i]) != bits(w_out))
            msg = f"{len(d)} output pixels differ, the first at {tuple(d[0])}"
        if msg:
            bad.append(f"{name}: {msg}")
    return bad


def report(bad):
    assert not bad, f"{len(bad)} frames differ; the first:\n" + "\n".join(bad[:8])


def device_run(g, src=None, dst=None):
    """device frames -> a device buffer (None: fresh, aligned allocations) -> (out, rec, mb, ms)"""
    import torch
    src = torch.from_numpy(g.frames).cuda() if src is None else src
    dst = torch.full(g.frames.shape, GUARD, dtype=torch.float32, device="cuda") if dst is None else dst
    rec, mb, ms = g.sky.normalize(src, out=dst if dst is not src else "inplace", meshes=True)
    return dst.cpu().numpy(), rec, mb, ms


def test_every_case_device_to_device(groups, ref):
    import torch
    bad = []
    for g in groups:
        src = torch.from_numpy(g.frames).cuda()
        assert src.data_ptr() % 16 == 0
        bad += failures(g, ref, *device_run(g, src))
        assert np.array_equal(bits(src.cpu().numpy()), bits(g.frames)), g.names[0]     # only read
    report(bad)


def test_every_case_host_to_host(groups, ref):
    bad = []
    for g in groups:
        out = np.full(g.frames.shape, GUARD, np.float32)
        rec, mb, ms = g.sky.normalize(g.frames, out=out, meshes=True)
        bad += failures(g, ref, out, rec, mb, ms)
    report(bad)


def test_big_endian_and_the_handles_buffer(gpu_ctx, groups, ref):
    from lfd_amd import _native
    again_p = dict(cell=16, n_clip=0, filter=1, mode=S.SUBTRACT)
    bad, n_be, n_own = [], 0, 0
    for g in groups:
        names = {c.name for c in g.cases}
        if names & K.BIG_ENDIAN:
            n_be += 1
            be = g.frames.astype(">f4")
            out = np.full(g.frames.shape, GUARD, np.float32)
            rec, mb, ms = g.sky.normalize(be, out=out, meshes=True)
            bad += failures(g, ref, out, rec, mb, ms)
            assert be.tobytes() == g.frames.astype(">f4").tobytes()                     # only read
        if names & (K.BIG_ENDIAN | HANDLE_ROUTE):
            n_own += 1
            n = len(g.frames)
            rec, mb, ms = g.sky.normalize(g.frames, meshes=True)                       # out=None: the handle's buffer
            want = np.stack([r[0] for c in g.cases for r in ref[c.name]])
            bad += failures(g, ref, want, rec, mb, ms)                                # (records and meshes)
            with _native.Sky(gpu_ctx, g.shape, max_frames=n, **again_p) as again:      # its pixels, read through a second handle
                out2 = np.full(g.frames.shape, GUARD, np.float32)
                again.normalize(g.sky.frames(n), out=out2)
            for i in range(n):
                if not np.array_equal(bits(out2[i]), bits(S.normalize(want[i], **again_p)[0])):
                    bad.append(f"{g.names[i]}: the handle's buffer differs")
    assert n_be == len(K.BIG_ENDIAN) == 4 and n_own == len(K.BIG_ENDIAN | HANDLE_ROUTE) == 13   # (each name in a group of its own)
    report(bad)


def off_by_one_float(shape, fill=None):
    """a contiguous view one float into a larger allocation -> (allocation, view)"""
    import torch
    n = int(np.prod(shape))
    big = torch.full((n + 9,), GUARD, dtype=torch.float32, device="cuda")
    view = big[1:1 + n].view(*shape)
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    assert view.is_contiguous() and big.data_ptr() % 16 == 0 and view.data_ptr() == big.data_ptr() + 4
    return big, view


def guards_intact(big):
    b = big.cpu().numpy()
    return b[0] == np.float32(GUARD) and (b[-8:] == np.float32(GUARD)).all()


def test_misaligned_source_destination_and_in_place(groups, ref):
    """the apply_ and cell_ cases with w % 4 == 0, whose aligned runs take the 16-byte loads and stores"""
    from lfd_amd import _native
    chosen = [g for g in groups if g.cases[0].family in ("apply", "cell") and g.shape[1] % 4 == 0]
    assert len(chosen) >= 15 and any(g.shape[1] > 1024 for g in chosen)
    bad = []
    for g in chosen:
        p = g.cases[0].params
        assert K.host_paths(*g.shape, p["cell"])["v4"] and not K.host_paths(*g.shape, p["cell"], src_off=1)["v4"]
        aligned = device_run(g)
        bad += failures(g, ref, *aligned)
        for what in ("source", "destination", "in place"):
            big_s, src = off_by_one_float(g.frames.shape, g.frames) if what != "destination" else (None, None)
            big_d, dst = off_by_one_float(g.frames.shape) if what == "destination" else (None, None)
            if what == "source":
                assert _native._ptr(src).value == src.data_ptr() and src.data_ptr() % 16 == 4   # the view goes by its own address
            got = device_run(g, src, src if what == "in place" else dst)
            same = all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[0::2] + got[3:], aligned[0::2] + aligned[3:]))
            same = same and all(same_rec(got[1][i], {k: aligned[1][i][k].item() for k in aligned[1].dtype.names}) is None
                                for i in range(len(g.frames)))
            if not same:
                bad.append(f"{g.names[0]} ...: misaligned {what} differs from the aligned run")
            for big in (big_s, big_d):
                if big is not None and not guards_intact(big):
                    bad.append(f"{g.names[0]} ...: misaligned {what}: floats outside the view were written")
            if what == "source" and not np.array_equal(bits(src.cpu().numpy()), bits(g.frames)):
                bad.append(f"{g.names[0]} ...: misaligned source was written")
    report(bad)
