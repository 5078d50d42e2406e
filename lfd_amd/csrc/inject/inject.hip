// inject.hip -- host side of the trail injection (include/lfdmi.h: trail injection; kernels in k_inject.h).  Its own translation
// unit in its own directory, like sky/: the detection kernels' code object does not change with it.  The context's internals
// are reached through unit.h.  The call keeps no state: its device memory comes from the stream's
// pool (hipMallocAsync) and goes back before the call's one wait.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_inject.h"

static_assert(INJ_MAX_TABLE == LFDMI_INJECT_MAX_TABLE, "the LDS table holds the header's cap");

#define INJ_LIST_MAX (8u << 20)         // (job, tile) pairs listed at a time: 64 MB
#define INJ_STAGE_BYTES (512ull << 20)  // device staging of host frames at a time
#define INJ_RENDER_BLOCKS 2048          // twice what 256 CUs hold at once (4 blocks of 4 waves each at 112 VGPRs): blocks walk the list

extern "C" int lfdmi_inject_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_inject_trail *trails,
                                   int n_trails, const float *tables, int n_tables, int table_len, double table_step, int subsample) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if (dtype != LFDMI_F32) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails takes LFDMI_F32 frames");
    if ((rc = unit_loc(ctx, loc))) return rc;
    if (n < 0 || n_trails < 0 || h < 1 || w < 1 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: n, n_trails >= 0, h, w positive, h * w at most 1e9");
    if ((n > 0 && !frames) || (n_trails > 0 && (!trails || !tables))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if (n_tables < 0 || table_len < 1 || table_len % 2 == 0 || table_len > LFDMI_INJECT_MAX_TABLE)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: table_len must be odd, 1 .. LFDMI_INJECT_MAX_TABLE");
    if (!std::isfinite(table_step) || !(table_step > 0)) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: table_step must be positive");
    if (subsample < 1 || subsample > 8) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: subsample 1 .. 8");
    for (int i = 0; i < n_trails; i++) {
        const lfdmi_inject_trail &t = trails[i];
        if (t.frame < 0 || t.frame >= n) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: trail " + std::to_string(i) + ": frame outside [0, n)");
        if (t.table < 0 || t.table >= n_tables)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: trail " + std::to_string(i) + ": table outside [0, n_tables)");
        if (!std::isfinite(t.rho) || !std::isfinite(t.theta) || !std::isfinite(t.amplitude) || fabs(t.rho) > 1e9)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_inject_trails: trail " + std::to_string(i) + ": rho (|rho| <= 1e9), theta and amplitude must be finite");
    }
    if (n == 0 || n_trails == 0) return 0;

    // trails by frame, ascending index within a frame (a counting sort); one job per frame that carries a trail
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    std::vector<int> start(n + 1, 0);
    for (int i = 0; i < n_trails; i++) start[trails[i].frame + 1]++;
    for (int f = 0; f < n; f++) start[f + 1] += start[f];
    std::vector<InjTrail> ht(n_trails);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        const double inf = std::numeric_limits<double>::infinity();
        for (int i = 0; i < n_trails; i++) {
            const lfdmi_inject_trail &t = trails[i];
            InjTrail &o = ht[at[t.frame]++];
            o.c = cos(t.theta); o.s = sin(t.theta); o.rho = t.rho;
            o.fx = t.rho * o.c; o.fy = t.rho * o.s;
            o.t0 = std::isfinite(t.t0) ? t.t0 : -inf;
            o.t1 = std::isfinite(t.t1) ? t.t1 : inf;
            o.amp = t.amplitude; o.table = t.table;
            o.bounded = std::isfinite(t.t0) || std::isfinite(t.t1);
        }
    }
    InjDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.ntx = (w + INJ_TILE_W - 1) / INJ_TILE_W; p.nty = (h + INJ_TILE_H - 1) / INJ_TILE_H;
    p.ss = subsample; p.M = (table_len - 1) / 2; p.table_len = table_len;
    p.step = table_step; p.halfw = (double)p.M * table_step; p.ss2 = (double)(subsample * subsample);
    for (int m = 0; m < subsample; m++) p.off[m] = ((double)m + 0.5) / (double)subsample - 0.5;
    const size_t ntiles = (size_t)p.ntx * p.nty;

    // chunks of jobs: the list of a chunk holds at most INJ_LIST_MAX pairs, host frames of a chunk at most INJ_STAGE_BYTES
    const bool in_dev = loc == LFDMI_DEVICE;
    size_t CH = std::max<size_t>(1, unit->limit_of(LIM_LIST_PAIRS, INJ_LIST_MAX) / ntiles);
    if (!in_dev) CH = std::min(CH, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, INJ_STAGE_BYTES) / FB));
    const size_t walk_max = unit->limit_of(LIM_RENDER_BLOCKS, INJ_RENDER_BLOCKS);
    std::vector<InjJob> hj;
    std::vector<int> jframe;
    for (int f = 0; f < n; f++)
        if (start[f + 1] > start[f]) {
            InjJob j;
            j.off = (int64_t)((in_dev ? (size_t)f : hj.size() % CH) * N);
            j.tb = start[f]; j.te = start[f + 1];
            hj.push_back(j);
            jframe.push_back(f);
        }
    const size_t nj = hj.size();
    CH = std::min(CH, nj);

    hipStream_t st = ctx_stream(ctx);
    Pool pool(st);
    InjTrail *d_tr = nullptr;
    InjJob *d_job = nullptr;
    float *d_tab = nullptr, *d_buf = nullptr;
    int2 *d_list = nullptr;
    int *d_count = nullptr;
    UHIP(pool.get(&d_tr, (size_t)n_trails));
    UHIP(pool.get(&d_job, nj));
    UHIP(pool.get(&d_tab, (size_t)n_tables * table_len));
    UHIP(pool.get(&d_list, CH * ntiles));
    UHIP(pool.get(&d_count, 1));
    if (!in_dev) UHIP(pool.get(&d_buf, CH * N));
    UHIP(hipMemcpyAsync(d_tr, ht.data(), (size_t)n_trails * sizeof(InjTrail), hipMemcpyHostToDevice, st));
    UHIP(hipMemcpyAsync(d_job, hj.data(), nj * sizeof(InjJob), hipMemcpyHostToDevice, st));
    UHIP(hipMemcpyAsync(d_tab, tables, (size_t)n_tables * table_len * sizeof(float), hipMemcpyHostToDevice, st));
    float *base = in_dev ? (float *)frames : d_buf;
    for (size_t j0 = 0; j0 < nj; j0 += CH) {
        const size_t c = std::min(CH, nj - j0);
        if (!in_dev)
            for (size_t k = 0; k < c; k++)
                UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + (size_t)jframe[j0 + k] * FB, FB, hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_count, 0, sizeof(int), st));
        const size_t pairs = c * ntiles, walk = std::min(pairs, walk_max);
        split->chunks++;
        split->grid = std::max<int64_t>(split->grid, (int64_t)walk);
        k_inject_cull<<<(unsigned)((pairs + INJ_THREADS - 1) / INJ_THREADS), INJ_THREADS, 0, st>>>(d_job + j0, (int)c, d_tr, p, d_list, d_count);
        ULAUNCH("k_inject_cull");
        k_inject_render<<<(unsigned)walk, INJ_THREADS, 0, st>>>(base, d_job + j0, d_tr, d_tab, p, d_list, d_count);
        ULAUNCH("k_inject_render");
        if (!in_dev)
            for (size_t k = 0; k < c; k++)
                UHIP(hipMemcpyAsync((char *)frames + (size_t)jframe[j0 + k] * FB, d_buf + k * N, FB, hipMemcpyDeviceToHost, st));
    }
    pool.release();
    // (the host arrays above are read by the queued copies: they live until this wait)
    UHIP(hipStreamSynchronize(st));
    return 0;
}
