// sub.hip -- host side of the trail subtraction (include/lfdmi.h: trail subtraction; kernels in k_sub.h and, for the cells,
// ../strip/k_strip.h).  Its own translation unit in its own directory, like strip/: the detection kernels' code object does not
// change with it.  The context's internals are reached through unit.h.  The call keeps no state: its device memory comes from
// the stream's pool (hipMallocAsync) and goes back before the call's one wait.  The cells and the tables stay on the device; the
// device returns five integers and a key per segment, and every double of a record is made here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_sub.h"
#include "../strip/k_strip_geo.h"

static_assert(sizeof(lfdmi_sub_params) == 48 && sizeof(lfdmi_sub) == 56, "the header's layouts");
static_assert(sizeof(StripCell) == sizeof(lfdmi_strip_cell) && sizeof(SubStat) == 32, "a cell is the header's");
static_assert(LFDMI_STRIP_MAX_OFF <= STRIP_TAB_B && LFDMI_SUB_MAX_SMOOTH == SUB_MAX_R, "a row of excesses fits a row of the LDS table");

#define SUB_LIST_MAX (8u << 20)         // (job, tile) pairs listed at a time: 64 MB
#define SUB_STAGE_BYTES (512ull << 20)  // device staging of host frames and host planes at a time
#define SUB_CELL_BYTES (512ull << 20)   // device cells of a chunk of frames (a frame's segments are never split: one frame may exceed it)
#define SUB_RENDER_BLOCKS 2048          // persistent blocks that walk the list

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kFix = 9.313225746154785e-10;   // 2^-30

extern "C" void lfdmi_default_sub_params(lfdmi_sub_params *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->sec_len = 32.0;
    out->step = 1.0;
    out->wing = 6.0;
    out->clip = 0.125f;
    out->smooth = 2;
    out->min_sec = 3;
    out->min_n = 8;
    out->min_wing = 8;
    out->apply = 1;
}

static_assert(LFDMI_SUB_OK == LFDMI_STRIP_OK && LFDMI_SUB_BAD_SEGMENT == LFDMI_STRIP_BAD_SEGMENT && LFDMI_SUB_TOO_LONG == LFDMI_STRIP_TOO_LONG,
              "a segment's status is the strips'");

// the strips' step 2 (strip_geometry, ../strip/k_strip_geo.h) with the strips' parameters of this call, then step 2 of the
// subtraction: u_b = (double)(b - K) * step and fabs are symmetric in b - K and grow with it, so the wing bins are those with
// |b - K| >= kw, kw the first k with fabs((double)k * step) >= half - wing (K + 1: there is none)
static int sub_geometry(const lfdmi_strip_segment &s, const lfdmi_sub_params &p, int max_sec, int max_cells, StripSeg &o, SubSeg &x) {
    lfdmi_strip_params sp;
    memset(&sp, 0, sizeof(sp));
    sp.sec_len = p.sec_len; sp.step = p.step;   // (all that the geometry reads)
    int K = 0;
    const int status = strip_geometry(s, sp, max_sec, max_cells, o, &K);
    if (status != LFDMI_STRIP_OK) return status;
    const double hw = s.half - p.wing;
    int kw = K + 1;
    for (int k = 0; k <= K; k++)
        if (fabs((double)k * p.step) >= hw) { kw = k; break; }
    x.kw = kw; x.K = K;
    return LFDMI_SUB_OK;
}

extern "C" int lfdmi_subtract_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                                     const lfdmi_strip_segment *segs, int n_seg, const float *sigma, const lfdmi_sub_params *pp, lfdmi_sub *out,
                                     float *model, int max_sections_per_seg, int max_cells_per_seg) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_subtract_trails", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    lfdmi_sub_params q;
    if (pp) q = *pp; else lfdmi_default_sub_params(&q);
    if (q.apply != 0 && q.apply != 1) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: params out of range: apply is 0 or 1");
    if (q.apply && dtype != LFDMI_F32) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails changes LFDMI_F32 frames only (apply = 0 reads LFDMI_F32_BE)");
    if (n < 0 || n_seg < 0 || h < 1 || w < 1 || h > 65536 || w > 65536 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: n, n_seg >= 0, h and w 1 .. 65536, h * w at most 1e9");
    if ((n > 0 && !frames) || (n_seg > 0 && (!segs || !out))) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: NULL argument");
    if (max_sections_per_seg < 1 || max_sections_per_seg > LFDMI_STRIP_MAX_SECTIONS)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: max_sections_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS");
    if (max_cells_per_seg < 1 || max_cells_per_seg > LFDMI_STRIP_MAX_SECTIONS * LFDMI_STRIP_MAX_OFF)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: max_cells_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS * LFDMI_STRIP_MAX_OFF");
    if (skip_bits < 0 || skip_bits > 255) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: skip_bits 0 .. 255");
    if (!(q.sec_len >= 4.0 && q.sec_len <= 4096.0) || !(q.step >= 0.5 && q.step <= 8.0) || !std::isfinite(q.wing) || !(q.wing > 0.0) ||
        !std::isfinite(q.clip) || !(q.clip > 0.0f && q.clip <= 1024.0f) || q.smooth < 0 || q.smooth > LFDMI_SUB_MAX_SMOOTH || q.min_sec < 1 ||
        q.min_sec > 2 * q.smooth + 1 || q.min_n < 1 || q.min_wing < 1)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: params out of range (include/lfdmi.h: lfdmi_sub_params)");
    for (int i = 0; i < n_seg; i++)
        if (segs[i].frame < 0 || segs[i].frame >= n)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_subtract_trails: segment " + std::to_string(i) + ": frame outside [0, n)");
    if ((rc = unit_sigma(ctx, "lfdmi_subtract_trails", sigma, n, nullptr))) return rc;
    if (n_seg == 0) return 0;

    // good segments by frame, ascending index within a frame (a counting sort): the order in which a pixel's subtractions apply
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    std::vector<StripSeg> geo(n_seg);
    std::vector<SubSeg> gx(n_seg);
    std::vector<int> status(n_seg);
    std::vector<int> start(n + 1, 0);
    for (int i = 0; i < n_seg; i++) {
        status[i] = sub_geometry(segs[i], q, max_sections_per_seg, max_cells_per_seg, geo[i], gx[i]);
        if (status[i] == LFDMI_SUB_OK) start[segs[i].frame + 1]++;
    }
    for (int f = 0; f < n; f++) start[f + 1] += start[f];
    const int ng = start[n];
    std::vector<StripSeg> hs(ng);
    std::vector<SubSeg> hx(ng);
    std::vector<int> place(n_seg, -1);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int i = 0; i < n_seg; i++)
            if (status[i] == LFDMI_SUB_OK) {
                place[i] = at[segs[i].frame]++;
                hs[place[i]] = geo[i];
                hx[place[i]] = gx[i];
            }
    }

    StripDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.ntx = (w + STRIP_TILE_W - 1) / STRIP_TILE_W; p.nty = (h + STRIP_TILE_H - 1) / STRIP_TILE_H;
    p.be = dtype == LFDMI_F32_BE;
    p.skip_bits = mask ? (uint32_t)skip_bits : 0u;
    memcpy(&p.clip_bits, &q.clip, sizeof(float));
    const size_t ntiles = (size_t)p.ntx * p.nty;

    // one job per frame that carries a good segment; chunks of jobs [cstart[c], cstart[c + 1]): a chunk's list holds at most
    // SUB_LIST_MAX pairs, what it stages at most SUB_STAGE_BYTES, its cells at most SUB_CELL_BYTES (a single job may exceed that).
    // StripSeg.base counts from the chunk's first cell, first[k] from the call's.
    const bool stage = loc != LFDMI_DEVICE, m_stage = stage && mask;
    size_t CH = std::max<size_t>(1, unit->limit_of(LIM_LIST_PAIRS, SUB_LIST_MAX) / ntiles);
    if (stage) CH = std::min(CH, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, SUB_STAGE_BYTES) / (FB + (m_stage ? N : 0))));
    const size_t cell_max = unit->limit_of(LIM_CELL_BYTES, SUB_CELL_BYTES) / sizeof(StripCell);
    const size_t walk_max = unit->limit_of(LIM_RENDER_BLOCKS, SUB_RENDER_BLOCKS);
    std::vector<StripJob> hj;
    std::vector<int> jframe;
    std::vector<size_t> cstart(1, 0), first(ng + 1, 0);
    size_t dev_cells = 1, most_jobs = 1;
    {
        size_t in_chunk = 0, jobs_in = 0;
        for (int f = 0; f < n; f++) {
            if (start[f + 1] == start[f]) continue;
            size_t c = 0;
            for (int k = start[f]; k < start[f + 1]; k++) c += (size_t)hs[k].n_sec * hs[k].n_off;
            if (jobs_in > 0 && (jobs_in >= CH || in_chunk + c > cell_max)) {
                cstart.push_back(hj.size());
                in_chunk = 0; jobs_in = 0;
            }
            for (int k = start[f]; k < start[f + 1]; k++) {
                const size_t ck = (size_t)hs[k].n_sec * hs[k].n_off;
                hs[k].base = (int64_t)in_chunk;
                in_chunk += ck;
                first[k + 1] = first[k] + ck;
            }
            StripJob j;
            j.foff = j.moff = (int64_t)((stage ? jobs_in : (size_t)f) * N);
            j.sb = start[f]; j.se = start[f + 1];
            hj.push_back(j);
            jframe.push_back(f);
            jobs_in++;
            dev_cells = std::max(dev_cells, in_chunk);
            most_jobs = std::max(most_jobs, jobs_in);
        }
        cstart.push_back(hj.size());
    }
    const size_t nj = hj.size(), ncell = first[ng];

    hipStream_t st = ctx_stream(ctx);
    std::vector<SubStat> hstat(ng);
    std::vector<float> hm(model ? ncell : 0);
    if (nj > 0) {
        Pool pool(st);
        StripSeg *d_seg = nullptr;
        SubSeg *d_sub = nullptr;
        StripJob *d_job = nullptr;
        uint32_t *d_buf = nullptr;
        uint8_t *d_mbuf = nullptr;
        int2 *d_list = nullptr;
        int *d_count = nullptr;
        StripCell *d_cell = nullptr;
        float *d_tab = nullptr;
        SubStat *d_stat = nullptr;
        UHIP(pool.get(&d_seg, (size_t)ng));
        UHIP(pool.get(&d_sub, (size_t)ng));
        UHIP(pool.get(&d_job, nj));
        UHIP(pool.get(&d_list, most_jobs * ntiles));
        UHIP(pool.get(&d_count, 1));
        UHIP(pool.get(&d_cell, dev_cells));
        UHIP(pool.get(&d_tab, dev_cells));
        UHIP(pool.get(&d_stat, (size_t)ng));
        if (stage) UHIP(pool.get(&d_buf, most_jobs * N));
        if (m_stage) UHIP(pool.get(&d_mbuf, most_jobs * N));
        UHIP(hipMemcpyAsync(d_seg, hs.data(), (size_t)ng * sizeof(StripSeg), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_sub, hx.data(), (size_t)ng * sizeof(SubSeg), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_job, hj.data(), nj * sizeof(StripJob), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_stat, 0, (size_t)ng * sizeof(SubStat), st));
        uint32_t *fbase = stage ? d_buf : (uint32_t *)frames;
        const uint8_t *mbase = !mask ? nullptr : m_stage ? d_mbuf : mask;
        p.vec = w % 4 == 0 && (uintptr_t)fbase % 16 == 0;
        p.mvec = mbase && w % 4 == 0 && (uintptr_t)mbase % 4 == 0;
        SubDev r;
        memset(&r, 0, sizeof(r));
        r.h = h; r.w = w; r.ntx = p.ntx; r.nty = p.nty; r.be = p.be; r.apply = q.apply; r.vec = p.vec;
        SubModelDev md;
        md.R = q.smooth; md.min_sec = q.min_sec; md.min_n = q.min_n; md.min_wing = q.min_wing;
        for (size_t ci = 0; ci + 1 < cstart.size(); ci++) {
            const size_t j0 = cstart[ci], c = cstart[ci + 1] - j0;
            const int k0 = hj[j0].sb, k1 = hj[j0 + c - 1].se;   // the chunk's segments [k0, k1)
            const size_t cc = first[k1] - first[k0];
            int top_sec = 1;
            for (int k = k0; k < k1; k++) top_sec = std::max(top_sec, hs[k].n_sec);
            for (size_t k = 0; k < c; k++) {
                const size_t f = (size_t)jframe[j0 + k];
                if (stage) UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + f * FB, FB, hipMemcpyHostToDevice, st));
                if (m_stage) UHIP(hipMemcpyAsync(d_mbuf + k * N, mask + f * N, N, hipMemcpyHostToDevice, st));
            }
            UHIP(hipMemsetAsync(d_cell, 0, cc * sizeof(StripCell), st));
            UHIP(hipMemsetAsync(d_count, 0, sizeof(int), st));
            const size_t pairs = c * ntiles;
            const unsigned walk = (unsigned)std::min(pairs, walk_max);
            split->chunks++;
            split->grid = std::max<int64_t>(split->grid, (int64_t)walk);
            k_strip_cull<<<(unsigned)((pairs + STRIP_THREADS - 1) / STRIP_THREADS), STRIP_THREADS, 0, st>>>(d_job + j0, (int)c, d_seg, p, d_list, d_count);
            ULAUNCH("k_strip_cull");
            k_strip_render<<<walk, STRIP_THREADS, 0, st>>>(fbase, mbase, d_job + j0, d_seg, p, d_list, d_count, d_cell);
            ULAUNCH("k_strip_render");
            k_sub_model<<<dim3((unsigned)(k1 - k0), (unsigned)((top_sec + SUB_ROWS - 1) / SUB_ROWS)), SUB_THREADS, 0, st>>>(d_seg + k0, d_sub + k0, d_cell,
                                                                                                                      md, d_tab, d_stat + k0);
            ULAUNCH("k_sub_model");
            k_sub_render<<<walk, SUB_THREADS, 0, st>>>(fbase, d_job + j0, d_seg, d_tab, r, d_list, d_count, d_stat);
            ULAUNCH("k_sub_render");
            if (stage && q.apply)
                for (size_t k = 0; k < c; k++)
                    UHIP(hipMemcpyAsync((char *)frames + (size_t)jframe[j0 + k] * FB, d_buf + k * N, FB, hipMemcpyDeviceToHost, st));
            if (model) UHIP(hipMemcpyAsync(hm.data() + first[k0], d_tab, cc * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        UHIP(hipMemcpyAsync(hstat.data(), d_stat, (size_t)ng * sizeof(SubStat), hipMemcpyDeviceToHost, st));
        pool.release();
    }
    // (the host arrays above are read and written by the queued copies: they live until this wait)
    UHIP(hipStreamSynchronize(st));

    for (int i = 0; i < n_seg; i++) {
        lfdmi_sub &o = out[i];
        memset(&o, 0, sizeof(o));
        float *mrow = model ? model + (size_t)i * max_cells_per_seg : nullptr;
        if (mrow) memset(mrow, 0, (size_t)max_cells_per_seg * sizeof(float));
        if (status[i] != LFDMI_SUB_OK) {
            o.status = status[i];
            o.removed = o.peak = kNaN;
            continue;
        }
        const int k = place[i];
        const StripSeg &g = hs[k];
        const SubStat &d = hstat[k];
        o.n_sec = g.n_sec; o.n_off = g.n_off; o.K = hx[k].K;
        o.n_usable = d.n_usable; o.n_model = d.n_model; o.n_pix = d.n_pix;
        o.q_removed = (int64_t)d.q_removed;
        o.removed = (double)o.q_removed * kFix;
        o.status = d.n_model ? LFDMI_SUB_OK : LFDMI_SUB_EMPTY;
        o.peak_section = -1;
        o.peak = kNaN;
        if (d.n_model) {
            // sub_peak_key back into the float and the cell
            const uint32_t ord = (uint32_t)(d.peak >> 32), cell = ~(uint32_t)(d.peak & 0xffffffffu);
            const uint32_t bits = (ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord;
            float m;
            memcpy(&m, &bits, sizeof(m));
            o.peak = (double)m;
            o.peak_section = (int32_t)(cell / (uint32_t)g.n_off);
        }
        if (mrow) memcpy(mrow, hm.data() + first[k], (size_t)g.n_sec * g.n_off * sizeof(float));
    }
    return 0;
}
