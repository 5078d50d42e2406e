// mask.hip -- host side of the trail masks (include/lfdmi.h: trail masks; kernels in k_mask.h).  Its own translation unit in its
// own directory, like inject/: the detection kernels' code object does not change with it.  The context's internals are reached
// through unit.h.  The call keeps no state: its device memory comes from the stream's pool (hipMallocAsync) and goes back before
// the call's one wait.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_mask.h"

static_assert(MSK_FILL_NONE == LFDMI_MASK_FILL_NONE && MSK_FILL_ZERO == LFDMI_MASK_FILL_ZERO && MSK_FILL_NAN == LFDMI_MASK_FILL_NAN &&
                  MSK_FILL_VALUE == LFDMI_MASK_FILL_VALUE,
              "the kernel's fill modes are the header's");
static_assert(sizeof(lfdmi_mask_segment) == 64 && sizeof(lfdmi_mask_stat) == 8 && sizeof(lfdmi_mask_params) == 8, "the header's layouts");

#define MSK_LIST_MAX (8u << 20)         // (job, tile) pairs listed at a time: 64 MB
#define MSK_STAGE_BYTES (512ull << 20)  // device staging of host frames and host planes at a time
#define MSK_RENDER_BLOCKS 2048          // persistent blocks that walk the list

extern "C" void lfdmi_default_mask_params(lfdmi_mask_params *out) {
    if (!out) return;
    out->fill_mode = LFDMI_MASK_FILL_NONE;
    out->clear = 1;
}

// step 2 of the definition: false for a LFDMI_MASK_BAD_SEGMENT
static bool mask_geometry(const lfdmi_mask_segment &s, MaskSeg &o) {
    const double c[4] = {s.x1, s.y1, s.x2, s.y2};
    for (double v : c)
        if (!std::isfinite(v) || fabs(v) > 1e6) return false;
    if (!std::isfinite(s.half) || s.half < 0.0) return false;
    if (std::isnan(s.cap) || s.cap < 0.0) return false;
    const double dx = s.x2 - s.x1, dy = s.y2 - s.y1;
    const double L = sqrt(dx * dx + dy * dy);
    if (L == 0.0) return false;
    o.x1 = s.x1; o.y1 = s.y1;
    o.ex = dx / L; o.ey = dy / L;
    o.nx = -o.ey; o.ny = o.ex;
    o.half = s.half; o.lo = -s.cap; o.hi = L + s.cap;
    o.fill = (float)s.fill; o.bits = s.bits;
    return true;
}

extern "C" int lfdmi_mask_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_mask_segment *segs,
                                 int n_seg, const lfdmi_mask_params *params, uint8_t *mask, int mask_loc, lfdmi_mask_stat *stats,
                                 int32_t *frame_counts) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    lfdmi_mask_params mp;
    lfdmi_default_mask_params(&mp);
    if (params) mp = *params;
    if (mp.fill_mode < LFDMI_MASK_FILL_NONE || mp.fill_mode > LFDMI_MASK_FILL_VALUE)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: fill_mode must be one of LFDMI_MASK_FILL_*");
    const bool fill = mp.fill_mode != LFDMI_MASK_FILL_NONE;
    if (fill && dtype != LFDMI_F32) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails fills LFDMI_F32 frames only");
    if (fill && (rc = unit_loc(ctx, loc))) return rc;
    if (mask && (rc = unit_loc(ctx, mask_loc))) return rc;
    if (n < 0 || n_seg < 0 || h < 1 || w < 1 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: n, n_seg >= 0, h, w positive, h * w at most 1e9");
    if (!fill && !mask) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: neither a mask nor a fill was asked for");
    if (fill && n > 0 && !frames) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: a fill needs frames");
    if (n_seg > 0 && !segs) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: NULL segs");
    for (int i = 0; i < n_seg; i++) {
        if (segs[i].frame < 0 || segs[i].frame >= n)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: segment " + std::to_string(i) + ": frame outside [0, n)");
        if (segs[i].bits == 0) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_mask_trails: segment " + std::to_string(i) + ": bits must not be 0");
    }
    if (frame_counts)
        for (int f = 0; f < n; f++) frame_counts[f] = 0;
    if (n == 0) return 0;

    // good segments by frame, ascending index within a frame (a counting sort); one job per frame that carries one
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    std::vector<MaskSeg> geo(n_seg);
    std::vector<char> good(n_seg);
    std::vector<int> start(n + 1, 0);
    for (int i = 0; i < n_seg; i++) {
        good[i] = mask_geometry(segs[i], geo[i]);
        if (good[i]) start[segs[i].frame + 1]++;
        if (stats) { stats[i].status = good[i] ? LFDMI_MASK_EMPTY : LFDMI_MASK_BAD_SEGMENT; stats[i].n_pix = 0; }
    }
    for (int f = 0; f < n; f++) start[f + 1] += start[f];
    const int ng = start[n];
    std::vector<MaskSeg> hs(ng);
    std::vector<int> orig(ng);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int i = 0; i < n_seg; i++)
            if (good[i]) {
                const int k = at[segs[i].frame]++;
                hs[k] = geo[i];
                orig[k] = i;
            }
    }
    MaskDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.ntx = (w + MSK_TILE_W - 1) / MSK_TILE_W; p.nty = (h + MSK_TILE_H - 1) / MSK_TILE_H;
    p.fill_mode = mp.fill_mode;
    const size_t ntiles = (size_t)p.ntx * p.nty;

    // chunks of jobs: the list of a chunk holds at most MSK_LIST_MAX pairs, what a chunk stages at most MSK_STAGE_BYTES
    const bool f_stage = fill && loc != LFDMI_DEVICE, m_stage = mask && mask_loc != LFDMI_DEVICE;
    size_t CH = std::max<size_t>(1, unit->limit_of(LIM_LIST_PAIRS, MSK_LIST_MAX) / ntiles);
    if (f_stage || m_stage)
        CH = std::min(CH, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, MSK_STAGE_BYTES) / ((f_stage ? FB : 0) + (m_stage ? N : 0))));
    const size_t walk_max = unit->limit_of(LIM_RENDER_BLOCKS, MSK_RENDER_BLOCKS);
    // (a job's staging slot is its index modulo CH; CH is clamped to the number of jobs below, which changes no slot: the clamp
    // only applies when there are fewer jobs than CH, where the modulo does nothing)
    std::vector<MaskJob> hj;
    std::vector<int> jframe;
    for (int f = 0; f < n; f++)
        if (start[f + 1] > start[f]) {
            MaskJob j;
            j.foff = (int64_t)((f_stage ? hj.size() % CH : (size_t)f) * N);
            j.moff = (int64_t)((m_stage ? hj.size() % CH : (size_t)f) * N);
            j.sb = start[f]; j.se = start[f + 1];
            hj.push_back(j);
            jframe.push_back(f);
        }
    const size_t nj = hj.size();
    CH = std::min(CH, std::max<size_t>(nj, 1));

    hipStream_t st = ctx_stream(ctx);
    // the planes of a clearing call: a device buffer is zeroed as a whole, a host buffer here where no job will copy a plane back
    if (mask && mp.clear) {
        if (!m_stage) UHIP(hipMemsetAsync(mask, 0, (size_t)n * N, st));
        else
            for (int f = 0; f < n; f++)
                if (start[f + 1] == start[f]) memset(mask + (size_t)f * N, 0, N);
    }
    std::vector<int> hcnt(ng, 0), hjc(nj, 0);
    if (nj > 0) {
        Pool pool(st);
        MaskSeg *d_seg = nullptr;
        MaskJob *d_job = nullptr;
        float *d_buf = nullptr;
        uint8_t *d_mbuf = nullptr;
        int2 *d_list = nullptr;
        int *d_count = nullptr, *d_cnt = nullptr, *d_jc = nullptr;
        UHIP(pool.get(&d_seg, (size_t)ng));
        UHIP(pool.get(&d_job, nj));
        UHIP(pool.get(&d_list, CH * ntiles));
        UHIP(pool.get(&d_count, 1));
        UHIP(pool.get(&d_cnt, (size_t)ng));
        UHIP(pool.get(&d_jc, nj));
        if (f_stage) UHIP(pool.get(&d_buf, CH * N));
        if (m_stage) UHIP(pool.get(&d_mbuf, CH * N));
        UHIP(hipMemcpyAsync(d_seg, hs.data(), (size_t)ng * sizeof(MaskSeg), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_job, hj.data(), nj * sizeof(MaskJob), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_cnt, 0, (size_t)ng * sizeof(int), st));
        UHIP(hipMemsetAsync(d_jc, 0, nj * sizeof(int), st));
        float *fbase = !fill ? nullptr : f_stage ? d_buf : (float *)frames;
        uint8_t *mbase = !mask ? nullptr : m_stage ? d_mbuf : mask;
        for (size_t j0 = 0; j0 < nj; j0 += CH) {
            const size_t c = std::min(CH, nj - j0);
            for (size_t k = 0; k < c; k++) {
                const size_t f = (size_t)jframe[j0 + k];
                if (f_stage) UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + f * FB, FB, hipMemcpyHostToDevice, st));
                if (m_stage && !mp.clear) UHIP(hipMemcpyAsync(d_mbuf + k * N, mask + f * N, N, hipMemcpyHostToDevice, st));
            }
            if (m_stage && mp.clear) UHIP(hipMemsetAsync(d_mbuf, 0, c * N, st));
            UHIP(hipMemsetAsync(d_count, 0, sizeof(int), st));
            const size_t pairs = c * ntiles, walk = std::min(pairs, walk_max);
            split->chunks++;
            split->grid = std::max<int64_t>(split->grid, (int64_t)walk);
            k_mask_cull<<<(unsigned)((pairs + MSK_THREADS - 1) / MSK_THREADS), MSK_THREADS, 0, st>>>(d_job + j0, (int)c, d_seg, p, d_list, d_count);
            ULAUNCH("k_mask_cull");
            k_mask_render<<<(unsigned)walk, MSK_THREADS, 0, st>>>(fbase, mbase, d_job + j0, d_seg, p, d_list, d_count, d_cnt, d_jc + j0);
            ULAUNCH("k_mask_render");
            for (size_t k = 0; k < c; k++) {
                const size_t f = (size_t)jframe[j0 + k];
                if (f_stage) UHIP(hipMemcpyAsync((char *)frames + f * FB, d_buf + k * N, FB, hipMemcpyDeviceToHost, st));
                if (m_stage) UHIP(hipMemcpyAsync(mask + f * N, d_mbuf + k * N, N, hipMemcpyDeviceToHost, st));
            }
        }
        UHIP(hipMemcpyAsync(hcnt.data(), d_cnt, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(hjc.data(), d_jc, nj * sizeof(int), hipMemcpyDeviceToHost, st));
        pool.release();
    }
    // (the host arrays above are read and written by the queued copies: they live until this wait)
    UHIP(hipStreamSynchronize(st));
    for (int k = 0; k < ng; k++)
        if (stats && hcnt[k] > 0) { stats[orig[k]].status = LFDMI_MASK_OK; stats[orig[k]].n_pix = hcnt[k]; }
    if (frame_counts)
        for (size_t j = 0; j < nj; j++) frame_counts[jframe[j]] = hjc[j];
    return 0;
}
