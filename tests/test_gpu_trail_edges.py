"""lfdmi_measure_trails off its defaults: the named cases of tests/trail_cases.py (small frames, parameter corners, geometry,
ties, bad samples, k_trail_final's paths, mask words) on the device against the restatement tests/trail_ref.py, every field
and profile bin equal in value, no tolerance; then the same frames in both byte orders from host, pinned and device memory,
chunked calls that mix found and not-found frames, a frame smaller than its context, and one context across parameter sets.
tests/test_trail_cases_model.py shows on the CPU that every case is the edge it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trail_cases as TC  # noqa: E402
import trail_ref as T  # noqa: E402
from test_gpu_trail_profiles import same, star_masks  # noqa: E402

pytestmark = pytest.mark.gpu


def rs_struct():
    from lfd_amd import _native
    return _native.make_rs_params(**TC.RS)


def inputs(cases, cats=None, found=None):
    """(frames [n, h, w], records, packed catalogue or None) of one call"""
    from lfd_amd import _native
    from lfd_amd.catalogs import pack_catalogs
    frames = np.stack([TC.frame(c["name"]) for c in cases])
    recs = np.zeros(len(cases), _native.RESULT_DTYPE)
    recs["found"] = [c["found"] for c in cases] if found is None else found
    recs["rho"], recs["theta"] = [c["rho"] for c in cases], [c["theta"] for c in cases]
    cats = [c["cat"] for c in cases] if cats is None else cats
    return frames, recs, (pack_catalogs(cats) if any(c is not None for c in cats) else None)


def measure(ctx, frames, recs, packed, params, **kw):
    return ctx.measure_trails(frames, recs, packed, rs_struct() if packed is not None else None, **kw, **params)


def own_context(frames, G=2):        # calls of three frames and more cross a chunk
    from lfd_amd import _native
    return _native.Context(0, frames.shape[1], frames.shape[2], G)


def equal_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


_HOST = {}


def host_result(cases):
    """the host '<f4' call of a list of cases through a context of the frames' size: run once, shared"""
    key = tuple(c["name"] for c in cases)
    if key not in _HOST:
        frames, recs, packed = inputs(cases)
        with own_context(frames) as ctx:
            _HOST[key] = measure(ctx, frames, recs, packed, cases[0]["params"])
    return _HOST[key]


@pytest.mark.parametrize("group", TC.GROUPS)
def test_cases_equal_the_restatement(group):
    bad = []
    for cases in TC.calls(group):
        frames, recs, packed = inputs(cases)
        out, prof = host_result(cases)
        masks = [None] * len(cases)
        if packed is not None:
            with own_context(frames) as ctx:
                masks = star_masks(ctx, len(cases), frames.shape[1:], packed, rs_struct())
        for i, c in enumerate(cases):
            r, p = TC.restated(c["name"], masks[i] if c["cat"] is not None else None)
            assert r["status"] == c["status"]
            msg = same(out[i], prof[i], r, p)
            if msg:
                bad.append((c["name"], msg))
    assert not bad, bad


def device_frames(frames):
    """(native torch frames, the big-endian bytes of the same frames as device memory, what keeps that alive)"""
    import torch
    from lfd_amd import _native
    dev = torch.from_numpy(frames).to("cuda:0")
    raw = torch.from_numpy(frames.astype(">f4").view(np.uint8)).to("cuda:0")
    return dev, _native.DeviceFrames(raw.data_ptr(), frames.shape), raw


@pytest.mark.parametrize("group", TC.GROUPS)
def test_byte_orders_and_locations_return_the_same_bytes(group):
    import torch
    for cases in TC.calls(group):
        frames, recs, packed = inputs(cases)
        want = host_result(cases)
        be = frames.astype(">f4")
        par = cases[0]["params"]
        names = [c["name"] for c in cases]
        with own_context(frames) as ctx:
            assert equal_bytes(measure(ctx, be, recs, packed, par), want), ("host >f4", names)
            assert be.tobytes() == frames.astype(">f4").tobytes()      # only read
            buf = ctx.pinned_buffer(frames.nbytes)
            try:
                for src, dt in ((frames, "<f4"), (be, ">f4")):
                    pin = buf.array.view(dt).reshape(frames.shape)
                    pin[:] = src
                    assert equal_bytes(measure(ctx, pin, recs, packed, par, pinned=True), want), ("pinned " + dt, names)
                    del pin
            finally:
                buf.close()
            dev, dev_be, keep = device_frames(frames)
            dcat = None if packed is None else {k: torch.from_numpy(v).to("cuda:0") for k, v in packed.items()}
            assert equal_bytes(measure(ctx, dev, recs, dcat, par), want), ("device <f4", names)
            assert equal_bytes(measure(ctx, dev_be, recs, dcat, par), want), ("device >f4", names)
            assert equal_bytes(measure(ctx, dev, recs, packed, par), want), ("device <f4, host catalogue", names)
            assert dev.cpu().numpy().tobytes() == frames.tobytes()
            del dev, dev_be, keep


# found = [1,0,0,1,1,0,1] in chunks of two leaves every chunk an active frame, with the active one first, second or alone;
# [1,1,0,0,0,1,1] has a chunk without one (frames 2 and 3) and a chunk whose only active frame is its second
@pytest.mark.parametrize("found", [[1, 0, 0, 1, 1, 0, 1], [1, 1, 0, 0, 0, 1, 1]])
def test_chunks_of_two_with_found_and_not_found_frames(found):
    from lfd_amd import _native
    base = [TC.CASES[n] for n in ("mask_w100", "mask_w100_tilted", "not_found_b")]
    cases = [base[i % 3] for i in range(7)]
    cats = [TC.mask_catalog(100, c["rho"], c["theta"], shift=i) for i, c in enumerate(cases)]   # every frame its own catalogue
    frames, recs, packed = inputs(cases, cats, found)
    par = base[0]["params"]
    with _native.Context(0, 96, 100, 2) as ctx:
        out, prof = measure(ctx, frames, recs, packed, par)
        masks = star_masks(ctx, 7, (96, 100), packed, rs_struct())
    assert len({m.tobytes() for m in masks}) == 7
    with _native.Context(0, 96, 100, 2) as ctx:
        for i in range(7):
            one = measure(ctx, frames[i], recs[i:i + 1], {k: v[i:i + 1] for k, v in packed.items()}, par)
            assert equal_bytes(one, (out[i:i + 1], prof[i:i + 1])), i
    for i, c in enumerate(cases):
        r, p = T.measure(frames[i], c["rho"], c["theta"], found=found[i], star_mask=masks[i], **par)
        assert r["status"] == (T.OK if found[i] else T.NOT_FOUND)
        assert same(out[i], prof[i], r, p) is None, (i, same(out[i], prof[i], r, p))


def test_frame_smaller_than_its_context():
    from lfd_amd import _native
    calls = [cs for cs in TC.calls() if TC.frame(cs[0]["name"]).shape == (96, 100)]
    assert len(calls) >= 8 and any(c["cat"] is not None and c["found"] for cs in calls for c in cs)
    with _native.Context(0, 200, 333, 4) as ctx:
        for cases in calls:
            frames, recs, packed = inputs(cases)
            assert equal_bytes(measure(ctx, frames, recs, packed, cases[0]["params"]), host_result(cases)), [c["name"] for c in cases]


def test_one_context_across_parameter_sets():
    from lfd_amd import _native
    C = TC.CASES
    big = [C["all_max"]]                                                    # 200 x 333, R = 64, K = 512
    small = [C["all_min"]]                                                  # 64 x 65, R = 1, K = 1
    stars = [C["mask_w100"], C["mask_w100_tilted"], C["not_found_b"]]       # the mask planes come late, and at another stride
    mid = [C["mask_w333"], C["mask_w333_tilted"]]
    sizes = []
    with _native.Context(0, 200, 333, 4) as ctx:
        for cases in (big, small, stars, big, mid, small, big):
            frames, recs, packed = inputs(cases)
            assert equal_bytes(measure(ctx, frames, recs, packed, cases[0]["params"]), host_result(cases)), [c["name"] for c in cases]
            sizes.append(ctx.workspace_bytes())
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] == sizes[3] and sizes[4:] == [sizes[4]] * 3   # grown, then reused
