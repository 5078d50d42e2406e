"""Calls in flight on one workspace: lfdmi_detect_batch_begin / lfdmi_process_multiscale_begin / lfdmi_end_oldest, through
BatchDetector.submit / submit_multiscale and Context.*_begin, against the synchronous calls (byte for byte) and the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def params():
    from lfd_amd.detecttrails import default_params
    return default_params()


def rs_pair(oracle, prs, flt="r"):
    from lfd_amd import _native
    kw = {k: v for k, v in prs.items() if k != "debug"}
    return _native.make_rs_params(flt, **kw), oracle.rs_params(flt, **kw)


def same(rec_gpu, rec_oracle):
    return all(rec_gpu[k].item() == v for k, v in rec_oracle.items())


def sdss_batches(nb, per, seed0=0):
    from lfd_amd import synth
    out = []
    for b in range(nb):
        frames, cats = zip(*[synth.make_frame(seed0 + 10 * b + k)[:2] for k in range(per)])
        out.append((np.stack(frames), synth.pack_catalogs(list(cats)), frames, cats))
    return out


def to_dev(packed):
    import torch
    return {k: torch.from_numpy(v).to("cuda:0") for k, v in packed.items()}


def test_submit_records_and_blotting_match_the_synchronous_call(oracle):
    """Eight calls over three device-resident batches with catalogues, two in flight, in the order of
    test_batch_detector_with_two_calls_in_flight: every future equals the synchronous detect on its batch, the device frames
    come back blotted as the synchronous call leaves them, and one batch equals the oracle."""
    import torch
    from lfd_amd import synth
    from lfd_amd.batch import BatchDetector
    pb, pd, prs = params()
    rs_g, rs_o = rs_pair(oracle, prs)
    batches = sdss_batches(3, 4)
    dcats = [to_dev(p) for _, p, _, _ in batches]
    det = BatchDetector(0, synth.SDSS_SHAPE, 4)
    want, blotted = [], []
    for (b, _, _, _), c in zip(batches, dcats):
        t = torch.from_numpy(b).to("cuda:0")
        want.append(det.detect(t, pb, pd, c, rs_g))
        blotted.append(t.cpu().numpy())
    order = [0, 1, 2, 0, 2, 1, 1, 0]
    dframes = [torch.from_numpy(batches[b][0]).to("cuda:0") for b in order]
    futs = [det.submit(dframes[i], pb, pd, dcats[b], rs_g) for i, b in enumerate(order)]
    assert det.ctx.calls_in_flight() == 2
    for i, (f, b) in enumerate(zip(futs, order)):
        assert f.result().tobytes() == want[b].tobytes(), (i, b)
        assert np.array_equal(dframes[i].cpu().numpy(), blotted[b]), (i, b)
    assert det.ctx.calls_in_flight() == 0
    assert det.spill_count() == 0
    with pytest.raises(RuntimeError):
        BatchDetector(0, synth.SDSS_SHAPE, 4, calls_in_flight=2).submit(dframes[0], pb, pd, dcats[0], rs_g)
    det.close()
    assert same(want[2][1], oracle.detect_frame(batches[2][2][1].copy(), pb, pd, batches[2][3][1], rs_o))


def test_submit_pinned_and_big_endian_frames(oracle):
    """Pinned float32 frames with a host catalogue: records equal, the caller's array blotted as by the synchronous call once
    result() returns.  Pinned '>f4' frames: records equal, bytes untouched.  Big-endian device frames: swapped in place."""
    import torch
    from lfd_amd import _native
    pb, pd, prs = params()
    rs_g, _ = rs_pair(oracle, prs)
    (batch, packed, _, _), (batch2, packed2, _, _) = sdss_batches(2, 3, seed0=40)
    with _native.Context(0, 1489, 2048, 4) as ctx:
        want = ctx.detect_batch(batch.copy(), pb, pd, packed, rs_g)
        want2 = ctx.detect_batch(batch2.copy(), pb, pd, packed2, rs_g)
        blotted = batch.copy()
        ctx.detect_batch(blotted, pb, pd, packed, rs_g)
        with pytest.raises(_native.NativeError) as e:                  # pageable host frames are refused
            ctx.detect_batch_begin(batch.copy(), pb, pd, packed, rs_g)
        assert e.value.code == _native.ERR_ARG and "lfdmi_host_alloc" in str(e.value)
        pin = ctx.pinned_buffer(2 * batch.nbytes)
        try:
            nat = pin.array[:batch.nbytes].view(np.float32).reshape(batch.shape)
            be = pin.array[batch.nbytes:].view(">f4").reshape(batch2.shape)
            nat[...] = batch
            be[...] = batch2
            a = ctx.detect_batch_begin(nat, pb, pd, packed, rs_g, pinned=True)
            b = ctx.detect_batch_begin(be, pb, pd, packed2, rs_g, pinned=True)
            assert a.result().tobytes() == want.tobytes()
            assert np.array_equal(nat, blotted)
            assert b.result().tobytes() == want2.tobytes()
            assert np.array_equal(be.astype(np.float32), batch2)
            del nat, be
        finally:
            pin.close()
        dbe = torch.from_numpy(batch2.astype(">f4").view(np.uint8)).to("cuda:0")
        frames = _native.DeviceFrames(dbe.data_ptr(), batch2.shape)
        c = ctx.detect_batch_begin(frames, pb, pd, to_dev(packed2), rs_g)
        assert c.result().tobytes() == want2.tobytes()
        swapped = dbe.cpu().numpy().view(np.float32).reshape(batch2.shape)
        blotted2 = batch2.copy()
        ctx.detect_batch(blotted2, pb, pd, packed2, rs_g)
        assert np.array_equal(swapped, blotted2)


def test_refused_call_leaves_big_endian_device_frames_untouched():
    """A call its checks refuse (here: rs.filter_index out of range with a catalogue of objects) does not swap big-endian
    device frames in place: through detect_batch and detect_batch_begin they stay byte for byte as they were."""
    import torch
    from lfd_amd import _native
    pb, pd, prs = params()
    bad = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    bad.filter_index = 5
    ((batch, packed, _, _),) = sdss_batches(1, 2, seed0=100)
    assert packed["NOBSERVE"].shape[1] > 0
    with _native.Context(0, 1489, 2048, 2) as ctx:
        dbe = torch.from_numpy(batch.astype(">f4").view(np.uint8)).to("cuda:0")
        before = dbe.cpu().numpy()
        frames = _native.DeviceFrames(dbe.data_ptr(), batch.shape)
        for call in (ctx.detect_batch, ctx.detect_batch_begin):
            with pytest.raises(_native.NativeError) as e:
                call(frames, pb, pd, to_dev(packed), bad)
            assert e.value.code == _native.ERR_ARG, call.__name__
            assert np.array_equal(dbe.cpu().numpy(), before), call.__name__
        assert ctx.calls_in_flight() == 0


@pytest.mark.parametrize("shape", [(4096, 4096), (1489, 2048)])
def test_submit_multiscale_matches_process_multiscale(shape):
    import torch
    from lfd_amd import synth
    from lfd_amd.batch import BatchDetector
    _, pd, _ = params()
    per = 2 if shape == synth.LSST_SHAPE else 3
    imgs = [np.stack([synth.make_frame(per * b + k, shape=shape, with_catalog=False)[0] for k in range(per)]) for b in range(3)]
    n = imgs[0].shape[0]
    det = BatchDetector(0, shape, n)
    rhos = [20.0, 10.0, 5.0]
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in imgs]
    want = [det.multiscale(d, pd, rhos) for d in dev]
    futs = [det.submit_multiscale(dev[i % 3], pd, rhos) for i in range(5)]
    for i, f in enumerate(futs):
        assert f.result().tobytes() == want[i % 3].tobytes(), i
    det.close()


def test_two_calls_in_flight_share_one_workspace():
    import torch
    from lfd_amd import synth
    from lfd_amd.batch import BatchDetector
    pb, pd, _ = params()
    frames = [torch.from_numpy(np.stack([synth.make_frame(k + 4 * b, with_catalog=False)[0] for k in range(4)])).to("cuda:0") for b in range(2)]
    det = BatchDetector(0, synth.SDSS_SHAPE, 4)
    det.detect(frames[0].clone(), pb, pd)
    before = det.workspace_bytes()
    a, b = det.submit(frames[0], pb, pd), det.submit(frames[1], pb, pd)
    assert det.workspace_bytes() == before
    a.result(), b.result()
    assert det.workspace_bytes() == before
    two = BatchDetector(0, synth.SDSS_SHAPE, 4, calls_in_flight=2)
    two.detect_async(frames[0].clone(), pb, pd).result()
    assert two.workspace_bytes() == 2 * before
    two.close()
    det.close()


def test_growth_and_spill_with_a_call_queued_behind(oracle, monkeypatch):
    """Tiny tables with two calls in flight: both records equal a default context's and the tables grew; with LFDMI_GROW=0 a
    frame spills to the worst-case workspace while the other call is queued, and the records are still equal."""
    import torch
    from lfd_amd import _native
    pb, pd, prs = params()
    rs_g, _ = rs_pair(oracle, prs)
    (b0, p0, _, _), (b1, p1, _, _) = sdss_batches(2, 3, seed0=60)
    with _native.Context(0, 1489, 2048, 3) as ref:
        w0, w1 = ref.detect_batch(b0.copy(), pb, pd, p0, rs_g), ref.detect_batch(b1.copy(), pb, pd, p1, rs_g)
    caps = {"run_cap": 3000, "key_cap": 64, "slot_cap": 2000, "list_cap": 1500, "peak_cap": 256}
    for grow in ("1", "0"):
        monkeypatch.setenv("LFDMI_GROW", grow)
        with _native.Context(0, 1489, 2048, 3, caps=caps) as ctx:
            d0, d1 = torch.from_numpy(b0).to("cuda:0"), torch.from_numpy(b1).to("cuda:0")
            f0 = ctx.detect_batch_begin(d0, pb, pd, to_dev(p0), rs_g)
            f1 = ctx.detect_batch_begin(d1, pb, pd, to_dev(p1), rs_g)
            assert f0.result().tobytes() == w0.tobytes(), grow
            assert f1.result().tobytes() == w1.tobytes(), grow
            st = ctx.stats()
            if grow == "1":
                assert st["cap_growths"] >= 1, st
            else:
                assert st["cap_growths"] == 0 and st["spilled_frames"] >= 1, st


def test_multi_chunk_call_beside_another(oracle):
    """One begin of n = 2G + 1 frames (three chunks), on the device and pinned, while another call is in flight."""
    import torch
    from lfd_amd import _native, synth
    pb, pd, prs = params()
    rs_g, _ = rs_pair(oracle, prs)
    frames, cats = zip(*[synth.make_frame(70 + k)[:2] for k in range(5)])
    big, packed = np.stack(frames), synth.pack_catalogs(list(cats))
    small = np.stack([synth.make_frame(80, with_catalog=False)[0]])
    with _native.Context(0, 1489, 2048, 2) as ctx:
        want = ctx.detect_batch(big.copy(), pb, pd, packed, rs_g)
        want_s = ctx.detect_batch(small.copy(), pb, pd)
        ds, db = torch.from_numpy(small).to("cuda:0"), torch.from_numpy(big).to("cuda:0")
        a = ctx.detect_batch_begin(ds, pb, pd)
        b = ctx.detect_batch_begin(db, pb, pd, to_dev(packed), rs_g)
        assert a.result().tobytes() == want_s.tobytes() and b.result().tobytes() == want.tobytes()
        pin = ctx.pinned_buffer(big.nbytes)
        try:
            nat = pin.array.view(np.float32).reshape(big.shape)
            nat[...] = big
            a = ctx.detect_batch_begin(torch.from_numpy(small).to("cuda:0"), pb, pd)
            b = ctx.detect_batch_begin(nat, pb, pd, packed, rs_g, pinned=True)
            assert a.result().tobytes() == want_s.tobytes() and b.result().tobytes() == want.tobytes()
            del nat
        finally:
            pin.close()


def test_contract_through_ctypes(oracle):
    """FIFO completion, every LFDMI_ERR_ARG refusal, overlapping frames, a begin that fails in its second chunk while another
    call is in flight, and close() with calls in flight."""
    import torch
    from lfd_amd import _native, synth
    lib = _native.lib()
    pb, pd, _ = params()
    P1, k1 = _native.make_params(pb)
    P2, k2 = _native.make_params(pd, dim=True)
    imgs = [np.stack([synth.make_frame(90 + 3 * b + k, with_catalog=False)[0] for k in range(3)]) for b in range(3)]
    ctx = _native.Context(0, 1489, 2048, 1)
    want = [ctx.detect_batch(x.copy(), pb, pd) for x in imgs]
    dev = [torch.from_numpy(x).to("cuda:0") for x in imgs]
    h = ctx._h
    res = [np.zeros(3, _native.RESULT_DTYPE) for _ in range(3)]

    def begin(i, n=3, ptr=None):
        return lib.lfdmi_detect_batch_begin(h, C.c_void_p(ptr or dev[i].data_ptr()), _native.F32, n, 1489, 2048, None, None,
                                            C.byref(P1), C.byref(P2), res[i].ctypes.data_as(C.c_void_p), _native.DEVICE)

    assert lib.lfdmi_end_oldest(h) == _native.ERR_ARG                   # nothing in flight
    assert begin(0) == 0 and begin(1) == 0
    assert lib.lfdmi_calls_in_flight(h) == 2
    assert begin(2) == _native.ERR_ARG                                  # a third begin
    with pytest.raises(_native.NativeError):                            # every other workspace user
        ctx.detect_batch(imgs[2].copy(), pb, pd)
    with pytest.raises(_native.NativeError):
        ctx.process_dim(imgs[2][0], pd)
    with pytest.raises(_native.NativeError):
        ctx.canny(np.zeros((64, 64), np.uint8))
    with pytest.raises(_native.NativeError):
        ctx.get_stage(0, _native.STAGE_CANNY, 1489, 2048)
    with pytest.raises(_native.NativeError):
        ctx.get_counters()
    assert lib.lfdmi_end_oldest(h) == 0 and lib.lfdmi_calls_in_flight(h) == 1
    assert res[0].tobytes() == want[0].tobytes()
    assert begin(2, n=2, ptr=dev[1].data_ptr() + 4) == _native.ERR_ARG  # overlaps the call in flight
    assert lib.lfdmi_end_oldest(h) == 0 and res[1].tobytes() == want[1].tobytes()
    ctx.enable_timing(True)
    assert begin(0) == _native.ERR_ARG                                  # timing on
    ctx.enable_timing(False)
    # FIFO: a, b ended in order; a failure in chunk 1 of a three-chunk begin leaves the earlier call intact
    res = [np.zeros(3, _native.RESULT_DTYPE) for _ in range(3)]
    dev = [torch.from_numpy(x).to("cuda:0") for x in imgs]
    assert begin(0) == 0
    ctx.debug_fail_chunk(1)
    assert begin(1) == _native.ERR_ARG
    assert lib.lfdmi_calls_in_flight(h) == 1
    assert lib.lfdmi_end_oldest(h) == 0 and res[0].tobytes() == want[0].tobytes()
    assert lib.lfdmi_calls_in_flight(h) == 0
    assert ctx.detect_batch(imgs[2].copy(), pb, pd).tobytes() == want[2].tobytes()
    # close() with calls in flight: they end, their results stay readable
    p0 = ctx.detect_batch_begin(torch.from_numpy(imgs[0]).to("cuda:0"), pb, pd)
    p1 = ctx.detect_batch_begin(torch.from_numpy(imgs[1]).to("cuda:0"), pb, pd)
    ctx.close()
    assert p0.result().tobytes() == want[0].tobytes() and p1.result().tobytes() == want[1].tobytes()
    # destroy with calls in flight, straight through the C-ABI
    raw = C.c_void_p()
    assert lib.lfdmi_ctx_create(0, 1489, 2048, 2, C.byref(raw)) == 0
    r2 = np.zeros(3, _native.RESULT_DTYPE)
    d2 = torch.from_numpy(imgs[2]).to("cuda:0")
    assert lib.lfdmi_detect_batch_begin(raw, C.c_void_p(d2.data_ptr()), _native.F32, 3, 1489, 2048, None, None, C.byref(P1), C.byref(P2),
                                        r2.ctypes.data_as(C.c_void_p), _native.DEVICE) == 0
    lib.lfdmi_ctx_destroy(raw)
    torch.cuda.synchronize()
