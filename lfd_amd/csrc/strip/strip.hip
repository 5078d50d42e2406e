// strip.hip -- host side of the trail strips (include/lfdmi.h: trail strips; kernels in k_strip.h).  Its own translation unit in
// its own directory, like lc/: the detection kernels' code object does not change with it.  The context's internals are reached
// through unit.h.  The call keeps no state: its device memory comes from the stream's pool (hipMallocAsync) and goes back before
// the call's one wait.  The device returns three integers per cell; every double of a record is made here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_strip.h"
#include "k_strip_geo.h"

static_assert(sizeof(lfdmi_strip_segment) == 48 && sizeof(lfdmi_strip_params) == 48 && sizeof(lfdmi_strip_cell) == 16 &&
                  sizeof(lfdmi_strip_section) == 72 && sizeof(lfdmi_strip) == 56,
              "the header's layouts");
static_assert(sizeof(StripCell) == sizeof(lfdmi_strip_cell) && sizeof(StripSeg) == 104, "a cell is the header's; a chunk of segments is 13 KB of LDS");
static_assert(LFDMI_STRIP_MAX_OFF <= STRIP_TAB_B, "a segment's bins fit a row of the table");

#define STRIP_LIST_MAX (8u << 20)         // (job, tile) pairs listed at a time: 64 MB
#define STRIP_STAGE_BYTES (512ull << 20)  // device staging of host frames and host planes at a time
#define STRIP_CELL_BYTES (512ull << 20)   // device cells of a batch of segments
#define STRIP_RENDER_BLOCKS 2048          // persistent blocks that walk the list

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kFix = 9.313225746154785e-10;   // 2^-30

extern "C" void lfdmi_default_strip_params(lfdmi_strip_params *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->sec_len = 8.0;
    out->step = 1.0;
    out->wing = 6.0;
    out->k_mom = 5.0;
    out->clip = 0.125f;
    out->min_core = 8;
    out->min_wing = 8;
}

// step 5 of the definition, from the section's n_off cells
static void strip_section(int j, const lfdmi_strip_cell *c, const StripSeg &g, int K, const lfdmi_strip_params &p, double sigma,
                          lfdmi_strip_section &o) {
    memset(&o, 0, sizeof(o));
    const double hw = g.half - p.wing;
    int64_t n_geom = 0, n_core = 0, n_wing = 0, q_wing = 0;
    for (int b = 0; b < g.n_off; b++) {
        const double ub = (double)(b - K) * p.step;
        n_geom += c[b].n_geom;
        if (fabs(ub) >= hw) { n_wing += c[b].n; q_wing += c[b].q; }
        else n_core += c[b].n;
    }
    o.n_geom = (int32_t)n_geom; o.n_core = (int32_t)n_core; o.n_wing = (int32_t)n_wing;
    o.t0 = (double)j * p.sec_len;
    o.t1 = std::min((double)(j + 1) * p.sec_len, g.L);
    o.bkg = o.rate = o.rate_err = o.centre = o.width = kNaN;
    if (o.n_geom == 0) { o.status = LFDMI_STRIP_SEC_EMPTY; return; }
    if (o.n_core < p.min_core || o.n_wing < p.min_wing) { o.status = LFDMI_STRIP_SEC_LOW; return; }
    o.status = LFDMI_STRIP_SEC_OK;
    const double nw = (double)n_wing;
    const double bkg = (double)q_wing * kFix / nw;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, R = 0.0;
    int nc = 0;
    for (int b = 0; b < g.n_off; b++) {
        const double ub = (double)(b - K) * p.step;
        if (fabs(ub) >= hw || c[b].n <= 0) continue;
        const double nb = (double)c[b].n;
        const double m = (double)c[b].q * kFix / nb;
        const double v = m - bkg;
        S0 = S0 + v;
        S1 = S1 + v * ub;
        S2 = S2 + v * ub * ub;
        R = R + 1.0 / nb;
        nc++;
    }
    o.bkg = bkg;
    o.rate = S0 * p.step;
    o.rate_err = sigma * p.step * sqrt(R + (double)nc * (double)nc / nw);
    if (o.rate >= p.k_mom * o.rate_err) {
        o.centre = S1 / S0;
        const double d = S2 / S0 - o.centre * o.centre;
        o.width = sqrt(d > 0.0 ? d : 0.0);
    }
}

// step 6 of the definition, from the segment's section records
static void strip_record(const lfdmi_strip_section *sec, const StripSeg &g, int K, lfdmi_strip &o) {
    memset(&o, 0, sizeof(o));
    o.n_sec = g.n_sec; o.n_off = g.n_off; o.K = K;
    o.dev_section = -1;
    o.mean_centre = o.mean_width = o.max_dev = kNaN;
    double nc = 0.0, nw = 0.0, den = 0.0;
    for (int j = 0; j < g.n_sec; j++) {
        const lfdmi_strip_section &s = sec[j];
        if (s.status != LFDMI_STRIP_SEC_OK) continue;
        o.n_ok++;
        if (!std::isfinite(s.centre)) continue;
        o.n_mom++;
        nc = nc + (double)s.n_core * s.centre;
        nw = nw + (double)s.n_core * s.width;
        den = den + (double)s.n_core;
    }
    o.status = o.n_ok ? LFDMI_STRIP_OK : LFDMI_STRIP_EMPTY;
    if (o.n_mom == 0) return;
    o.mean_centre = nc / den;
    o.mean_width = nw / den;
    for (int j = 0; j < g.n_sec; j++) {
        const lfdmi_strip_section &s = sec[j];
        if (s.status != LFDMI_STRIP_SEC_OK || !std::isfinite(s.centre)) continue;
        const double d = fabs(s.centre - o.mean_centre);
        if (o.dev_section < 0 || d > o.max_dev) { o.dev_section = j; o.max_dev = d; }
    }
}

extern "C" int lfdmi_trail_strips(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                                  const lfdmi_strip_segment *segs, int n_seg, const float *sigma, const lfdmi_strip_params *pp, lfdmi_strip *out,
                                  lfdmi_strip_section *sections, int max_sections_per_seg, lfdmi_strip_cell *cells, int max_cells_per_seg) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_trail_strips", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (n < 0 || n_seg < 0 || h < 1 || w < 1 || h > 65536 || w > 65536 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: n, n_seg >= 0, h and w 1 .. 65536, h * w at most 1e9");
    if ((n > 0 && !frames) || (n_seg > 0 && (!segs || !out || !sections || !cells)))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: NULL argument");
    if (max_sections_per_seg < 1 || max_sections_per_seg > LFDMI_STRIP_MAX_SECTIONS)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: max_sections_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS");
    if (max_cells_per_seg < 1 || max_cells_per_seg > LFDMI_STRIP_MAX_SECTIONS * LFDMI_STRIP_MAX_OFF)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: max_cells_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS * LFDMI_STRIP_MAX_OFF");
    if (skip_bits < 0 || skip_bits > 255) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: skip_bits 0 .. 255");
    lfdmi_strip_params q;
    if (pp) q = *pp; else lfdmi_default_strip_params(&q);
    if (!(q.sec_len >= 4.0 && q.sec_len <= 4096.0) || !(q.step >= 0.5 && q.step <= 8.0) || !std::isfinite(q.wing) || !(q.wing > 0.0) ||
        !std::isfinite(q.k_mom) || !(q.k_mom >= 0.0) || !std::isfinite(q.clip) || !(q.clip > 0.0f && q.clip <= 1024.0f) || q.min_core < 1 ||
        q.min_wing < 1)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: params out of range (include/lfdmi.h: lfdmi_strip_params)");
    for (int i = 0; i < n_seg; i++)
        if (segs[i].frame < 0 || segs[i].frame >= n)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_trail_strips: segment " + std::to_string(i) + ": frame outside [0, n)");
    std::vector<float> sig;
    if ((rc = unit_sigma(ctx, "lfdmi_trail_strips", sigma, n, &sig))) return rc;
    if (n_seg == 0) return 0;

    // good segments by frame (a counting sort); the cells of the good segments in a row
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    std::vector<StripSeg> geo(n_seg);
    std::vector<int> status(n_seg), Ks(n_seg, 0);
    std::vector<int> start(n + 1, 0);
    for (int i = 0; i < n_seg; i++) {
        status[i] = strip_geometry(segs[i], q, max_sections_per_seg, max_cells_per_seg, geo[i], &Ks[i]);
        if (status[i] == LFDMI_STRIP_OK) start[segs[i].frame + 1]++;
    }
    for (int f = 0; f < n; f++) start[f + 1] += start[f];
    const int ng = start[n];
    std::vector<StripSeg> hs(ng);
    std::vector<int> place(n_seg, -1), sframe(ng);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int i = 0; i < n_seg; i++)
            if (status[i] == LFDMI_STRIP_OK) {
                place[i] = at[segs[i].frame]++;
                hs[place[i]] = geo[i];
                sframe[place[i]] = segs[i].frame;
            }
    }
    // batches of segments [k0, k1): at most STRIP_CELL_BYTES of cells on the device; StripSeg.base counts from the batch's first cell,
    // first[k] from the call's
    const size_t cell_max = unit->limit_of(LIM_CELL_BYTES, STRIP_CELL_BYTES) / sizeof(StripCell);
    std::vector<size_t> first(ng + 1, 0);
    std::vector<int> bstart(1, 0);
    {
        size_t in_batch = 0;
        for (int k = 0; k < ng; k++) {
            const size_t c = (size_t)hs[k].n_sec * hs[k].n_off;   // (at most 1024 * 129: below the compiled limit; a batch's first always fits)
            if (in_batch > 0 && in_batch + c > cell_max) { bstart.push_back(k); in_batch = 0; }
            hs[k].base = (int64_t)in_batch;
            in_batch += c;
            first[k + 1] = first[k] + c;
        }
        bstart.push_back(ng);
    }
    const size_t ncell = first[ng];
    size_t dev_cells = 0;
    for (size_t b = 0; b + 1 < bstart.size(); b++) dev_cells = std::max(dev_cells, first[bstart[b + 1]] - first[bstart[b]]);

    StripDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.ntx = (w + STRIP_TILE_W - 1) / STRIP_TILE_W; p.nty = (h + STRIP_TILE_H - 1) / STRIP_TILE_H;
    p.be = dtype == LFDMI_F32_BE;
    p.skip_bits = mask ? (uint32_t)skip_bits : 0u;
    memcpy(&p.clip_bits, &q.clip, sizeof(float));
    const size_t ntiles = (size_t)p.ntx * p.nty;

    // chunks of jobs: the list of a chunk holds at most STRIP_LIST_MAX pairs, what a chunk stages at most STRIP_STAGE_BYTES
    const bool stage = loc != LFDMI_DEVICE, m_stage = stage && mask;
    size_t CH = std::max<size_t>(1, unit->limit_of(LIM_LIST_PAIRS, STRIP_LIST_MAX) / ntiles);
    if (stage) CH = std::min(CH, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, STRIP_STAGE_BYTES) / (FB + (m_stage ? N : 0))));
    const size_t walk_max = unit->limit_of(LIM_RENDER_BLOCKS, STRIP_RENDER_BLOCKS);
    // the jobs of every batch in a row: a frame whose segments two batches share is a job of both
    std::vector<StripJob> hj;
    std::vector<int> jframe;
    std::vector<size_t> jstart(1, 0);
    for (size_t b = 0; b + 1 < bstart.size(); b++) {
        const int k0 = bstart[b], k1 = bstart[b + 1];
        for (int k = k0; k < k1;) {
            const int f = sframe[k];
            int e = k;
            while (e < k1 && sframe[e] == f) e++;
            StripJob j;
            j.foff = j.moff = (int64_t)((stage ? (hj.size() - jstart[b]) % CH : (size_t)f) * N);
            j.sb = k; j.se = e;
            hj.push_back(j);
            jframe.push_back(f);
            k = e;
        }
        jstart.push_back(hj.size());
    }
    const size_t nj = hj.size();
    {
        size_t most = 1;
        for (size_t b = 0; b + 1 < jstart.size(); b++) most = std::max(most, jstart[b + 1] - jstart[b]);
        CH = std::min(CH, most);   // (changes no staging slot: it only applies where the modulo does nothing)
    }

    hipStream_t st = ctx_stream(ctx);
    std::vector<lfdmi_strip_cell> hc(ncell);
    if (nj > 0) {
        Pool pool(st);
        StripSeg *d_seg = nullptr;
        StripJob *d_job = nullptr;
        uint32_t *d_buf = nullptr;
        uint8_t *d_mbuf = nullptr;
        int2 *d_list = nullptr;
        int *d_count = nullptr;
        StripCell *d_cell = nullptr;
        UHIP(pool.get(&d_seg, (size_t)ng));
        UHIP(pool.get(&d_job, nj));
        UHIP(pool.get(&d_list, CH * ntiles));
        UHIP(pool.get(&d_count, 1));
        UHIP(pool.get(&d_cell, dev_cells));
        if (stage) UHIP(pool.get(&d_buf, CH * N));
        if (m_stage) UHIP(pool.get(&d_mbuf, CH * N));
        UHIP(hipMemcpyAsync(d_seg, hs.data(), (size_t)ng * sizeof(StripSeg), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_job, hj.data(), nj * sizeof(StripJob), hipMemcpyHostToDevice, st));
        const uint32_t *fbase = stage ? d_buf : (const uint32_t *)frames;
        const uint8_t *mbase = !mask ? nullptr : m_stage ? d_mbuf : mask;
        p.vec = w % 4 == 0 && (uintptr_t)fbase % 16 == 0;
        p.mvec = mbase && w % 4 == 0 && (uintptr_t)mbase % 4 == 0;
        for (size_t b = 0; b + 1 < bstart.size(); b++) {
            const size_t bc = first[bstart[b + 1]] - first[bstart[b]];
            UHIP(hipMemsetAsync(d_cell, 0, bc * sizeof(StripCell), st));
            split->batches++;
            for (size_t j0 = jstart[b]; j0 < jstart[b + 1]; j0 += CH) {
                const size_t c = std::min(CH, jstart[b + 1] - j0);
                for (size_t k = 0; k < c; k++) {
                    const size_t f = (size_t)jframe[j0 + k];
                    if (stage) UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + f * FB, FB, hipMemcpyHostToDevice, st));
                    if (m_stage) UHIP(hipMemcpyAsync(d_mbuf + k * N, mask + f * N, N, hipMemcpyHostToDevice, st));
                }
                UHIP(hipMemsetAsync(d_count, 0, sizeof(int), st));
                const size_t pairs = c * ntiles, walk = std::min(pairs, walk_max);
                split->chunks++;
                split->grid = std::max<int64_t>(split->grid, (int64_t)walk);
                k_strip_cull<<<(unsigned)((pairs + STRIP_THREADS - 1) / STRIP_THREADS), STRIP_THREADS, 0, st>>>(d_job + j0, (int)c, d_seg, p, d_list,
                                                                                                              d_count);
                ULAUNCH("k_strip_cull");
                k_strip_render<<<(unsigned)walk, STRIP_THREADS, 0, st>>>(fbase, mbase, d_job + j0, d_seg, p, d_list, d_count, d_cell);
                ULAUNCH("k_strip_render");
            }
            UHIP(hipMemcpyAsync(hc.data() + first[bstart[b]], d_cell, bc * sizeof(StripCell), hipMemcpyDeviceToHost, st));
        }
        pool.release();
    }
    // (the host arrays above are read and written by the queued copies: they live until this wait)
    UHIP(hipStreamSynchronize(st));

    for (int i = 0; i < n_seg; i++) {
        lfdmi_strip &o = out[i];
        lfdmi_strip_section *row = sections + (size_t)i * max_sections_per_seg;
        lfdmi_strip_cell *crow = cells + (size_t)i * max_cells_per_seg;
        memset(row, 0, (size_t)max_sections_per_seg * sizeof(lfdmi_strip_section));
        memset(crow, 0, (size_t)max_cells_per_seg * sizeof(lfdmi_strip_cell));
        if (status[i] != LFDMI_STRIP_OK) {
            memset(&o, 0, sizeof(o));
            o.status = status[i];
            o.mean_centre = o.mean_width = o.max_dev = kNaN;
            continue;
        }
        const StripSeg &g = hs[place[i]];
        const double sg = (double)sig[segs[i].frame];
        const size_t nc = (size_t)g.n_sec * g.n_off;
        memcpy(crow, hc.data() + first[place[i]], nc * sizeof(lfdmi_strip_cell));
        for (int j = 0; j < g.n_sec; j++) strip_section(j, crow + (size_t)j * g.n_off, g, Ks[i], q, sg, row[j]);
        strip_record(row, g, Ks[i], o);
    }
    return 0;
}
