// streak.hip -- host side of the short-streak search (include/lfdmi.h: short-streak search; kernels in k_streak.h).  Its own
// translation unit in its own directory, like stars/ and radon/: the detection kernels' code object does not change with it.
// The context's internals are reached through unit.h.  The call keeps no state: its device memory comes from the stream's pool
// (hipMallocAsync) and goes back before it returns.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_streak.h"

#define STREAK_STAGE_BYTES (1ull << 30)   // device staging of host frames at a time
#define STREAK_CELL_BYTES (2ull << 30)    // binned cells of one chunk
#define STREAK_MAX_CHUNK 16384            // frames of one launch (frame and orientation go in grid.z)
#define STREAK_MAX_DEVICES 64             // devices whose LDS allowance is remembered as raised

static_assert(offsetof(lfdmi_streak, snr) + sizeof(float) == sizeof(StreakRec), "lfdmi_streak begins with StreakRec");
static_assert(sizeof(lfdmi_streak) == 88 && sizeof(lfdmi_streak_params) == 24, "lfdmi_streak layout");

extern "C" void lfdmi_default_streak_params(lfdmi_streak_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->bin = 2; o->length = 32; o->max_streaks = 4; o->peel_halfwidth = 8;
    o->clip = 0.125f; o->threshold = 8.0f;
}

static bool streak_params_ok(const lfdmi_streak_params &q) {
    if (q.bin != 1 && q.bin != 2 && q.bin != 4) return false;
    if (q.length != 8 && q.length != 16 && q.length != 32 && q.length != 64) return false;
    if (q.max_streaks < 1 || q.max_streaks > LFDMI_STREAK_MAX_STREAKS || q.peel_halfwidth < 0 || q.peel_halfwidth > 65536) return false;
    if (!std::isfinite(q.clip) || !(q.clip > 0) || !std::isfinite(q.threshold) || !(q.threshold > 0)) return false;
    // step 2's range rule (a clip beyond 2048 never passes it: the product is compared in doubles first)
    const double top = (double)q.clip * 1048576.0;
    if (!(top < 2147483648.0)) return false;
    return llrint(top) * q.bin * q.bin * q.length < 2147483648ll;
}

// dev: the context's device.  The kernel's LDS allowance is raised once per device and process (a second thread that gets here
// first sets the same value again)
template <int L> static hipError_t streak_launch(int dev, dim3 grid, hipStream_t st, const int2 *cells, const StreakDev &p, const int *idx,
                                                 const float *sigma, unsigned long long *part) {
    const size_t lds = (size_t)(STK_TC + L - 1) * (STK_TR + 2 * (L - 1)) * sizeof(int2);
    static std::atomic<bool> raised[STREAK_MAX_DEVICES];
    if (lds > 48 * 1024 && !(dev >= 0 && dev < STREAK_MAX_DEVICES && raised[dev].load())) {
        hipError_t e = hipFuncSetAttribute((const void *)k_streak_search<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < STREAK_MAX_DEVICES) raised[dev].store(true);
    }
    k_streak_search<L><<<grid, STK_THREADS, lds, st>>>(cells, p, idx, sigma, part);
    return hipGetLastError();
}

// step 6's doubles of a record that is LFDMI_STREAK_OK
static void streak_line(const StreakDev &p, lfdmi_streak &o) {
    const int c[2] = {o.c0, o.c0 + p.L - 1}, r[2] = {o.r0, o.r0 + o.s};
    double x[2], y[2];
    for (int k = 0; k < 2; k++) {
        const double i = o.q == 0 ? c[k] : r[k], j = o.q == 0 ? r[k] : c[k];
        x[k] = (double)p.b * i + (double)(p.b - 1) / 2.0;
        y[k] = (double)p.b * j + (double)(p.b - 1) / 2.0;
    }
    o.x1 = x[0]; o.y1 = y[0]; o.x2 = x[1]; o.y2 = y[1];
    double theta = atan2(-(o.x2 - o.x1), o.y2 - o.y1);
    const double pi = 3.141592653589793;
    if (theta < 0.0) theta += pi;
    if (theta >= pi) theta -= pi;
    o.theta = theta;
    o.rho = o.x1 * cos(theta) + o.y1 * sin(theta);
}

extern "C" int lfdmi_streak_search(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                                   const lfdmi_streak_params *pp, lfdmi_streak *out, int32_t *n_streaks) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_streak_search", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    lfdmi_streak_params q;
    if (pp) q = *pp; else lfdmi_default_streak_params(&q);
    if (!streak_params_ok(q)) return ctx_fail(ctx, LFDMI_ERR_ARG, "streak params out of range (include/lfdmi.h: lfdmi_streak_params)");
    if (n < 0 || h < 2 * q.bin || w < 2 * q.bin || h > STK_MAX_CELLS * q.bin || w > STK_MAX_CELLS * q.bin)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_streak_search: n >= 0, h and w 2 bin .. 4096 bin");
    if (n > 0 && (!frames || !out || !n_streaks)) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    std::vector<float> sg;
    if ((rc = unit_sigma(ctx, "lfdmi_streak_search", sigma, n, &sg))) return rc;
    if (n == 0) return 0;

    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE;
    const int K = q.max_streaks;
    StreakDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.b = q.bin; p.be = dtype == LFDMI_F32_BE; p.L = q.length;
    p.hb = (h + q.bin - 1) / q.bin; p.wb = (w + q.bin - 1) / q.bin;
    p.hw = (q.peel_halfwidth + q.bin - 1) / q.bin;
    p.clip = q.clip; p.threshold = q.threshold;
    // one grid for both orientations: anchors of R rows and C - L + 1 columns, R x C = hb x wb and wb x hb
    const int big = std::max(p.hb, p.wb);
    const dim3 sgrid((std::max(big - p.L + 1, 1) + STK_TC - 1) / STK_TC, (big + STK_TR - 1) / STK_TR, 1);
    p.nparts = (int)(sgrid.x * sgrid.y * 2);
    const size_t ncell = (size_t)p.hb * p.wb;

    size_t chunk = STREAK_MAX_CHUNK;
    if (!in_dev) chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, STREAK_STAGE_BYTES) / FB));
    chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_CELL_BYTES, STREAK_CELL_BYTES) / (ncell * sizeof(int2))));

    hipStream_t st = ctx_stream(ctx);
    const int dev = ctx_device(ctx);
    memset(out, 0, (size_t)n * K * sizeof(lfdmi_streak));
    memset(n_streaks, 0, (size_t)n * sizeof(int32_t));
    std::vector<StreakRec> hrec(std::min<size_t>(chunk, n));   // (the queued copies use these: declared ahead of the pools, which wait)
    std::vector<int> hidx(hrec.size()), next;
    for (int c0 = 0; c0 < n; c0 += (int)chunk) {
        const int nf = std::min<int>((int)chunk, n - c0);
        split->chunks++;
        Pool pool(st);
        uint32_t *d_buf = nullptr;
        int2 *d_cells = nullptr;
        unsigned long long *d_part = nullptr;
        StreakRec *d_rec = nullptr;
        int *d_idx = nullptr;
        float *d_sigma = nullptr;
        UHIP(pool.get(&d_cells, (size_t)nf * ncell));
        UHIP(pool.get(&d_part, (size_t)nf * p.nparts));
        UHIP(pool.get(&d_rec, (size_t)nf));
        UHIP(pool.get(&d_idx, (size_t)nf));
        UHIP(pool.get(&d_sigma, (size_t)nf));
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * N;
        if (!in_dev) {
            UHIP(pool.get(&d_buf, (size_t)nf * N));
            UHIP(hipMemcpyAsync(d_buf, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = d_buf;
        }
        UHIP(hipMemcpyAsync(d_sigma, sg.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        k_streak_prep<<<dim3((p.wb + STK_THREADS - 1) / STK_THREADS, p.hb, nf), STK_THREADS, 0, st>>>(src, p, d_cells);
        ULAUNCH("k_streak_prep");
        int ncur = nf;
        for (int i = 0; i < nf; i++) hidx[i] = i;
        for (int k = 0; k < K && ncur > 0; k++) {
            // the frames still going, compacted: slot z of this round's launches is frame hidx[z] of the chunk
            UHIP(hipMemcpyAsync(d_idx, hidx.data(), (size_t)ncur * sizeof(int), hipMemcpyHostToDevice, st));
            const dim3 g(sgrid.x, sgrid.y, (unsigned)ncur * 2);
            hipError_t e = hipSuccess;
            switch (p.L) {
                case 8: e = streak_launch<8>(dev, g, st, d_cells, p, d_idx, d_sigma, d_part); break;
                case 16: e = streak_launch<16>(dev, g, st, d_cells, p, d_idx, d_sigma, d_part); break;
                case 32: e = streak_launch<32>(dev, g, st, d_cells, p, d_idx, d_sigma, d_part); break;
                default: e = streak_launch<64>(dev, g, st, d_cells, p, d_idx, d_sigma, d_part); break;
            }
            if (e != hipSuccess) return ctx_fail(ctx, LFDMI_ERR_HIP, std::string("launch k_streak_search: ") + hipGetErrorString(e));
            k_streak_finish<<<ncur, STK_THREADS, 0, st>>>(d_cells, p, d_idx, d_sigma, d_part, d_rec);
            ULAUNCH("k_streak_finish");
            if (k + 1 < K) {   // (a frame whose record is not found is left alone: it stops here)
                k_streak_peel<<<dim3((p.wb + STK_THREADS - 1) / STK_THREADS, p.hb, ncur), STK_THREADS, 0, st>>>(d_cells, p, d_idx, d_rec);
                ULAUNCH("k_streak_peel");
            }
            UHIP(hipMemcpyAsync(hrec.data(), d_rec, (size_t)ncur * sizeof(StreakRec), hipMemcpyDeviceToHost, st));
            UHIP(hipStreamSynchronize(st));   // the host decides which frames continue
            next.clear();
            for (int z = 0; z < ncur; z++) {
                const int f = c0 + hidx[z];
                lfdmi_streak &o = out[(size_t)f * K + k];
                const StreakRec &r = hrec[z];
                o.status = r.status ? LFDMI_STREAK_NONE : LFDMI_STREAK_OK;
                if (r.status) continue;
                o.found = r.found; o.q = r.q; o.s = r.s; o.r0 = r.r0; o.c0 = r.c0; o.n_pix = r.n_pix; o.sum = r.sum; o.snr = r.snr;
                streak_line(p, o);
                if (r.found) {
                    n_streaks[f]++;
                    next.push_back(hidx[z]);
                }
            }
            ncur = (int)next.size();
            std::copy(next.begin(), next.end(), hidx.begin());
        }
        pool.release();
        UHIP(hipStreamSynchronize(st));
    }
    return 0;
}

// the tile of k_streak_search, for the tests that plant segments at its seams
extern "C" void lfdmi_streak_tile(int32_t *rows, int32_t *cols) {
    if (rows) *rows = STK_TR;
    if (cols) *cols = STK_TC;
}
