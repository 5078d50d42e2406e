"""Frame-parallel sharding of a batch over the GPUs of one node.

Frames are independent (process_field keeps no cross-frame state, detecttrails.py:30-143) and
the reference itself scales by handing disjoint run lists to separate PBS jobs
(createjobs/createjobs.py:173-202).  Here every rank (one process per GPU) takes a contiguous
block of frames, runs ``lfdmi_detect_batch`` on its own device, and the per-frame result
records (48 B each) are gathered once at the end.  There is no collective on the data path.
"""
import threading
import time

import numpy as np

from . import _native


def shard_bounds(n_frames, world_size):
    """Contiguous blocks of ceil(n/world) frames: [(start, stop)] per rank (config 4: 1024 each)."""
    per = -(-n_frames // world_size) if world_size > 0 else n_frames
    return [(min(r * per, n_frames), min((r + 1) * per, n_frames)) for r in range(world_size)]


def shard_range(n_frames, rank, world_size):
    return shard_bounds(n_frames, world_size)[rank]


def gather_results(local, n_frames, group=None):
    """All ranks contribute their structured result array; every rank gets the full batch back.

    Uses torch.distributed (gloo on CPU tensors, RCCL on device tensors); the payload is
    48 B x frames, so this is a latency-bound bookkeeping exchange, not data-path traffic."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return local
    world = dist.get_world_size(group)
    bounds = shard_bounds(n_frames, world)
    per = max(b - a for a, b in bounds)
    rec = _native.RESULT_DTYPE.itemsize
    buf = np.zeros(per * rec, np.uint8)
    raw = np.ascontiguousarray(local).view(np.uint8).reshape(-1)
    buf[:raw.size] = raw
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    mine = torch.from_numpy(buf).to(dev)
    out = torch.empty(world * per * rec, dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, mine, group=group)
    allrec = out.cpu().numpy().reshape(world, per * rec)
    parts = [allrec[r, :(b - a) * rec].copy().view(_native.RESULT_DTYPE) for r, (a, b) in enumerate(bounds)]
    return np.concatenate(parts)


class BatchDetector:
    """Runs the full pipe over this rank's share of a batch on one GPU.

    ``lanes`` independent contexts (own HIP stream, own workspace for ``inflight // lanes``
    frames) work on disjoint slices of the batch concurrently, each driven by its own host
    thread (ctypes releases the GIL).  Most kernels of this path are latency-bound with long
    tails (a few tall contours, the largest Hough lists), so two or more streams keep the CUs
    busy where one stream would idle between dependent launches.  Frames are independent, so
    this is the same frame-parallel sharding as across GPUs, one level down.
    """

    def __init__(self, device=0, shape=(1489, 2048), inflight=32, stream=None, lanes=1, caps=None, stage_images=False,
                 calls_in_flight=1, sky=None, stars=None):
        """stars: None, or a dict of lfdmi_stars_params fields ({} = the defaults): ``detect`` / ``submit`` called without
        ``catalogs`` then find each frame's compact sources first (include/lfdmi.h: source finder) and hand the device-resident
        catalogue built from them to the call; after ``sky=`` the normalised buffer is searched, with sigma = target_sigma.
        ``last_stars`` holds the frame records of the last call.  An explicit ``catalogs=`` wins.  Needs lanes == 1 and
        calls_in_flight == 1.  Host frames without ``sky=`` are uploaded twice (by the finder, then by the detect call, which
        blots the caller's array): keep frames on the device where that matters.
        sky: None, or a dict of lfdmi_sky_params fields ({} = the defaults): ``detect`` / ``submit`` / ``multiscale`` then
        first normalise the frames into a ``Sky`` handle's device buffer (include/lfdmi.h: sky normalisation) and work on that
        buffer, ``measure_trails`` measures it, and ``last_sky`` holds the records of the last call.  Needs lanes == 1 and
        calls_in_flight == 1."""
        from concurrent.futures import ThreadPoolExecutor
        self.lanes = max(1, int(lanes))
        self.calls_in_flight = max(1, int(calls_in_flight))
        if self.calls_in_flight > 1 and self.lanes > 1:
            raise ValueError("calls_in_flight > 1 needs lanes == 1")
        if stars is not None:                              # (checked before any context exists)
            if self.lanes != 1 or self.calls_in_flight != 1:
                raise ValueError("stars= needs lanes == 1 and calls_in_flight == 1")
            from .stars import as_params as stars_params
            stars = stars_params(stars)
        per = max(1, inflight // self.lanes)
        self.ctxs = [_native.Context(device, shape[0], shape[1], per, caps=caps) for _ in range(self.lanes * self.calls_in_flight)]
        for c in self.ctxs:  # a batch detector is for throughput: no 8-bit debug images per frame unless asked for
            c.set_stage_images(1 if stage_images else 0)
        self.ctx = self.ctxs[0]
        self._own_stream = None
        if self.calls_in_flight > 1 and stream is None:
            import torch                                   # (a stream for the contexts to share when the caller names none)
            self._own_stream = torch.cuda.Stream(device)
            stream = self._own_stream.cuda_stream
        if self.lanes == 1 and stream is not None:
            # several calls in flight: every context launches into the SAME stream (one after the other on the GPU, each in its
            # own workspace)
            for c in self.ctxs:
                c.set_stream(stream)
        self.pool = ThreadPoolExecutor(self.lanes) if self.lanes > 1 else None
        # detect_async / multiscale_async: a host thread per context, calls dealt out in turn
        self._turn_pool = [ThreadPoolExecutor(1) for _ in self.ctxs] if self.calls_in_flight > 1 else None
        self._turn = 0
        self._pending = []
        self._start_lock = threading.Lock()
        self._last_start = 0.0
        self._spacing = 0.001
        self.shape = shape
        self.sky, self.last_sky, self._sky_src = None, None, None
        if sky is not None:
            if self.lanes != 1 or self.calls_in_flight != 1:
                raise ValueError("sky= needs lanes == 1 and calls_in_flight == 1")
            from .sky import as_params
            self.sky = _native.Sky(self.ctx, shape, max_frames=per, **as_params(sky))
        self.stars, self.last_stars = None, None
        if stars is not None:
            self.stars = stars
            self._stars_sigma = None if self.sky is None else float(_native.make_sky_params(**as_params(sky)).target_sigma)

    # ---- the source finder in front of a call without catalogues (stars=...) ------------------------------------------------------
    def _finds(self, catalogs, rs):
        """whether this call's catalogue comes from the finder"""
        if self.stars is None or catalogs is not None:
            return False
        if rs is None:
            raise ValueError("stars=: the call needs rs (remove_stars' parameters) to blot what the finder finds")
        return True

    def _found_catalog(self, frames, rs):
        """(device-resident catalogue of the frames' sources, frame records); the squares use rs.pixscale"""
        self._drain()
        rec, frec = self.ctx.find_stars(frames, sigma=self._stars_sigma, device_out=True, **self.stars)
        return self.ctx.stars_catalog(rec, frec, rs.pixscale, device=True), frec

    # ---- sky normalisation in front of every call (sky=...) ------------------------------------------------------------------
    def _drain(self):
        for f in list(self._pending):
            f.result()
        self._pending = []
        while self.ctx.calls_in_flight():
            self.ctx._end_oldest()

    def _normalized(self, frames, a, b, pinned=False):
        """frames[a:b] normalised into the handle's buffer -> (NativeDeviceFrames, records)"""
        self._drain()                                        # (the buffer is the pending calls' input)
        part = frames.slice(a, b) if isinstance(frames, _native.DeviceFrames) else frames[a:b]
        rec = self.sky.normalize(part, pinned=pinned)
        return self.sky.frames(b - a), rec

    def _sky_chunks(self, frames, call):
        """call(buffer, a, b) on every max_frames chunk of the normalised frames; the sky records go to ``last_sky``"""
        n = frames.shape[0]
        outs, recs = [], []
        for a in range(0, n, self.sky.max_frames):
            b = min(n, a + self.sky.max_frames)
            buf, rec = self._normalized(frames, a, b)
            recs.append(rec)
            outs.append(call(buf, a, b))
        self.last_sky = np.concatenate(recs)
        self._sky_src = frames if n <= self.sky.max_frames else None
        return outs

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
        for ex in self._turn_pool or ():
            ex.shutdown()
        for c in self.ctxs:
            c.close()

    # ---- several calls in flight ---------------------------------------------------------------------------------------------
    # A synchronous call returns when its records are on the host; the next call's first kernel then starts ~0.1 ms later (the
    # return, the caller, the re-entry, a launch on an idle queue: profiles/r04_gap_trace.txt).  With ``calls_in_flight=2`` the
    # detector owns two contexts (a workspace each) that launch into one stream, and a host thread per context: while call k runs,
    # call k + 1 is already queued behind it, and the GPU goes from one to the other without waiting for the host.  The calls
    # still run one after the other on the GPU and their results are what the synchronous call returns.
    def _in_turn(self, method, args):
        if self.sky is not None:
            raise RuntimeError("detect_async / multiscale_async are not routed through sky=: use detect / submit")
        if self.stars is not None:
            raise RuntimeError("detect_async / multiscale_async are not routed through stars=: use detect / submit")
        if self._turn_pool is None:
            raise RuntimeError("BatchDetector(calls_in_flight=1): use detect / multiscale")
        i = self._turn
        self._turn = (i + 1) % len(self.ctxs)
        fut = self._turn_pool[i].submit(self._call, i, method, args)
        self._pending = [f for f in self._pending if not f.done()] + [fut]
        return fut

    def _busy(self):
        """Calls still in flight (a context serves one host thread at a time: a synchronous call then takes its turn too)."""
        self._pending = [f for f in self._pending if not f.done()]
        return bool(self._pending)

    def _call(self, i, method, args):
        # two calls that start together interleave their launches and finish together -- and would keep doing so: the starts are
        # kept a quarter of a call apart (in the steady state they are half a call apart by themselves)
        with self._start_lock:
            wait = self._last_start + self._spacing - time.perf_counter()
            if wait > 0:
                time.sleep(wait)
            self._last_start = t0 = time.perf_counter()
        out = getattr(self.ctxs[i], method)(*args)
        self._spacing = min(0.05, max(0.0005, 0.25 * (time.perf_counter() - t0)))
        return out

    def detect_async(self, frames, params_bright, params_dim, catalogs=None, rs=None):
        """``detect`` as a ``concurrent.futures.Future`` (``calls_in_flight`` > 1): submit the next batch before asking for the
        previous one's ``result()``.  Device-resident frames must stay untouched until the result is there."""
        return self._in_turn("detect_batch", (frames, params_bright, params_dim, catalogs, rs))

    def multiscale_async(self, frames, params, rhos, dim=True, flip=True, after_bright=False):
        return self._in_turn("process_multiscale", (frames, params, rhos, dim, flip, after_bright))

    # ---- calls in flight on one workspace ------------------------------------------------------------------------------------
    # ``submit`` / ``submit_multiscale`` enqueue a call on the detector's single context (lfdmi_detect_batch_begin /
    # lfdmi_process_multiscale_begin) and return its ``Pending``: the next call is queued behind the current one on the same
    # stream, in the same workspace, with no host thread and no second context (half the device memory of ``detect_async``).
    # Two calls are in flight at most; a third submit first ends the oldest (its records wait in its ``Pending``).
    def _submit_ctx(self):
        if self.lanes != 1 or self.calls_in_flight != 1:
            raise RuntimeError("submit needs BatchDetector(lanes=1, calls_in_flight=1): one context that takes the calls in flight")
        ctx = self.ctx
        while ctx.calls_in_flight() >= _native.MAX_CALLS_IN_FLIGHT:
            ctx._end_oldest()
        return ctx

    def submit(self, frames, params_bright, params_dim, catalogs=None, rs=None, pinned=False):
        """``detect`` without waiting: returns a ``Pending`` (``.result()`` = ``detect``'s records).  Frames are device-resident
        (or ``PinnedBuffer`` memory with ``pinned=True``) and, with the catalogue, must stay untouched until the call has ended."""
        if self.sky is not None:
            if frames.shape[0] > self.sky.max_frames:
                raise ValueError("submit with sky=: at most `inflight` frames per call (the handle's buffer)")
            buf, self.last_sky = self._normalized(frames, 0, frames.shape[0], pinned=pinned)
            self._sky_src = frames
            if self._finds(catalogs, rs):
                catalogs, self.last_stars = self._found_catalog(buf, rs)
            return self._submit_ctx().detect_batch_begin(buf, params_bright, params_dim, catalogs, rs)
        if self._finds(catalogs, rs):
            catalogs, self.last_stars = self._found_catalog(frames, rs)
        return self._submit_ctx().detect_batch_begin(frames, params_bright, params_dim, catalogs, rs, pinned=pinned)

    def submit_multiscale(self, frames, params, rhos, dim=True, flip=True, after_bright=False):
        """``multiscale`` without waiting (device-resident frames): a ``Pending`` whose ``.result()`` is its records."""
        if self.sky is not None:
            if frames.shape[0] > self.sky.max_frames:
                raise ValueError("submit_multiscale with sky=: at most `inflight` frames per call (the handle's buffer)")
            buf, self.last_sky = self._normalized(frames, 0, frames.shape[0])
            self._sky_src = frames
            return self._submit_ctx().process_multiscale_begin(buf, params, rhos, dim=dim, flip=flip, after_bright=after_bright)
        return self._submit_ctx().process_multiscale_begin(frames, params, rhos, dim=dim, flip=flip, after_bright=after_bright)

    def enable_timing(self, on=True):
        for c in self.ctxs:
            c.enable_timing(on)

    def timing_select(self, names=None):
        for c in self.ctxs:
            c.timing_select(names)

    def get_timing(self):
        out = {}
        for c in self.ctxs:
            for k, (ms, n, u) in c.get_timing().items():
                a = out.get(k, (0.0, 0, 0))
                out[k] = (a[0] + ms, a[1] + n, a[2] + u)
        return out

    def workspace_bytes(self):
        return sum(c.workspace_bytes() for c in self.ctxs)

    def spill_count(self):
        return sum(c.spill_count() for c in self.ctxs)

    def stats(self):
        """Sum of every lane's ``Context.stats()``."""
        out = {}
        for c in self.ctxs:
            for k, v in c.stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def get_counters(self):
        """Work counters ([slots, 22] int32, see lfdmi_get_counters) the last pass left, all lanes."""
        return np.concatenate([c.get_counters() for c in self.ctxs])

    @staticmethod
    def _slice_cat(cat, a, b):
        if cat is None:
            return None
        return {k: v[a:b] for k, v in cat.items()}

    def multiscale(self, frames, params, rhos, dim=True, flip=True, after_bright=False):
        """One pass (dim or bright) with HoughLines at every rho of ``rhos`` over the batch: records [len(rhos), n]."""
        if self.sky is not None:
            return np.concatenate(self._sky_chunks(frames, lambda buf, a, b: self.ctx.process_multiscale(
                buf, params, rhos, dim=dim, flip=flip, after_bright=after_bright)), axis=1)
        if self.lanes == 1:
            if self._turn_pool is not None and self._busy():
                return self.multiscale_async(frames, params, rhos, dim, flip, after_bright).result()
            return self.ctx.process_multiscale(frames, params, rhos, dim=dim, flip=flip, after_bright=after_bright)
        n = frames.shape[0]
        bounds = shard_bounds(n, self.lanes)
        futs = [self.pool.submit(c.process_multiscale, frames[a:b], params, rhos, dim, flip, after_bright)
                for c, (a, b) in zip(self.ctxs, bounds) if b > a]
        return np.concatenate([f.result() for f in futs], axis=1)

    def detect(self, frames, params_bright, params_dim, catalogs=None, rs=None):
        """frames: (n, h, w) float32, numpy (staged through the library) or a torch CUDA tensor
        (used in place; must be complete on the device before the call when lanes > 1).
        catalogs: dict from synth.pack_catalogs (numpy or torch CUDA tensors)."""
        find = self._finds(catalogs, rs)
        if self.sky is not None:
            found = []

            def call(buf, a, b):
                cat = self._slice_cat(catalogs, a, b)
                if find:
                    cat, frec = self._found_catalog(buf, rs)
                    found.append(frec)
                return self.ctx.detect_batch(buf, params_bright, params_dim, cat, rs)
            out = np.concatenate(self._sky_chunks(frames, call))
            if find:
                self.last_stars = np.concatenate(found)
            return out
        if find:
            catalogs, self.last_stars = self._found_catalog(frames, rs)
        if self.lanes == 1:
            if self._turn_pool is not None and self._busy():
                return self.detect_async(frames, params_bright, params_dim, catalogs, rs).result()
            return self.ctx.detect_batch(frames, params_bright, params_dim, catalogs, rs)
        n = frames.shape[0]
        bounds = shard_bounds(n, self.lanes)
        futs = [self.pool.submit(c.detect_batch, frames[a:b], params_bright, params_dim,
                                 self._slice_cat(catalogs, a, b), rs)
                for c, (a, b) in zip(self.ctxs, bounds) if b > a]
        return np.concatenate([f.result() for f in futs])

    def detect_rounds(self, frames, params_bright, params_dim, catalogs=None, rs=None, pinned=False, rounds_params=None):
        """``detect`` for up to ``max_trails`` trails per frame (include/lfdmi.h: detection rounds; rounds_params: a dict of
        lfdmi_rounds_params fields, None = the defaults): (records [n, max_trails], n_found [n], dup_of [n, max_trails]), record
        0 being ``detect``'s.  Sharded over the lanes like ``detect``; with calls in flight it runs after them.  Not routed
        through ``sky=``."""
        from .rounds import as_params
        rp = as_params(rounds_params)
        if self.sky is not None:
            raise RuntimeError("detect_rounds is not routed through sky=: normalise the frames first")
        if self._finds(catalogs, rs):
            catalogs, self.last_stars = self._found_catalog(frames, rs)
        if self.lanes == 1:
            self._drain()
            return self.ctx.detect_rounds(frames, params_bright, params_dim, catalogs, rs, pinned=pinned, **rp)
        n = frames.shape[0]
        bounds = shard_bounds(n, self.lanes)
        futs = [self.pool.submit(lambda c=c, a=a, b=b: c.detect_rounds(frames[a:b], params_bright, params_dim,
                                                                      self._slice_cat(catalogs, a, b), rs, pinned=pinned, **rp))
                for c, (a, b) in zip(self.ctxs, bounds) if b > a]
        res = [f.result() for f in futs]
        return tuple(np.concatenate([r[j] for r in res]) for j in range(3))

    def measure_trails(self, frames, records, catalogs=None, rs=None, **params):
        """``Context.measure_trails`` over the batch (trail profiles of the frames whose record has found != 0), sharded like
        ``detect``.  With calls in flight it runs after them: the calls that produced ``records`` have ended by then.
        With ``sky=`` the normalised frames are measured.  If ``frames`` is the very object the last detect / submit call was
        given (identity, not equality) and it fitted the handle's buffer, that buffer is measured as the call left it;
        any other array -- an equal copy included -- is normalised again, chunk by chunk, which gives the same values.  An
        array changed in place between the two calls must not be passed as the same object."""
        if self.sky is not None:
            # the frames the records describe are the normalised ones: the handle's buffer when it still holds them (the last
            # call's frames, blotted by remove_stars as detect left them), otherwise normalised again chunk by chunk
            self._drain()
            if frames is self._sky_src:
                return self.ctx.measure_trails(self.sky.frames(frames.shape[0]), records, catalogs, rs, **params)
            keep = self.last_sky
            res = self._sky_chunks(frames, lambda buf, a, b: self.ctx.measure_trails(buf, records[a:b], self._slice_cat(catalogs, a, b),
                                                                                   rs, **params))
            self.last_sky, self._sky_src = keep, None
            return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
        if self.lanes == 1:
            for f in list(self._pending):
                f.result()
            self._pending = []
            while self.ctx.calls_in_flight():
                self.ctx._end_oldest()
            return self.ctx.measure_trails(frames, records, catalogs, rs, **params)
        n = frames.shape[0]
        bounds = shard_bounds(n, self.lanes)
        futs = [self.pool.submit(c.measure_trails, frames[a:b], records[a:b], self._slice_cat(catalogs, a, b), rs, **params)
                for c, (a, b) in zip(self.ctxs, bounds) if b > a]
        res = [f.result() for f in futs]
        return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])

    def fit_defocus(self, bank, trails, profiles, seeing=None, **kw):
        """``Context.fit_defocus`` on the first lane's context (the bank's: build it with ``DefocusBank(bd.ctx, ...)``).  With
        calls in flight it runs after them, as ``measure_trails`` does."""
        for f in list(self._pending):
            f.result()
        self._pending = []
        while self.ctx.calls_in_flight():
            self.ctx._end_oldest()
        return self.ctx.fit_defocus(bank, trails, profiles, seeing, **kw)

    def measure_seeing(self, frames, sigma=None, stars_params=None, **params):
        """``psf.measure_seeing`` (the source finder with its records left on the device, then ``Context.measure_seeing``) on the
        first lane's context.  With calls in flight it runs after them, as ``fit_defocus`` does."""
        from . import psf
        for f in list(self._pending):
            f.result()
        self._pending = []
        while self.ctx.calls_in_flight():
            self.ctx._end_oldest()
        return psf.measure_seeing(self.ctx, frames, sigma=sigma, stars_params=stars_params, **params)
