// preview.hip -- host side of the frame previews (include/lfdmi.h: frame previews; kernels in k_preview.h).  Its own translation
// unit in its own directory, like the other units: the detection kernels' code object does not change with it.  The context's
// internals are reached through unit.h, the limits of its chunks through limits/limits.h.  The call keeps no state: its device
// memory comes from the stream's pool (hipMallocAsync) and is queued for release behind each chunk's work; the stream is waited
// for once, at the end.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_preview.h"

#define PREVIEW_STAGE_BYTES (1ull << 30)   // device staging of host frames at a time
#define PREVIEW_CELL_BYTES (1ull << 30)    // the int64 cell plane of a chunk
#define PREVIEW_MAX_CHUNK 32768            // frames of one launch (they go in grid.y)
#define PREVIEW_RENDER_BLOCKS 256          // blocks per frame of k_preview_render at most

static_assert(PRV_OK == LFDMI_PREVIEW_OK && PRV_FLAT == LFDMI_PREVIEW_FLAT && PRV_EMPTY == LFDMI_PREVIEW_EMPTY, "lfdmi_preview_frame status");
static_assert(PRV_RANK == LFDMI_PREVIEW_RANK && PRV_GIVEN == LFDMI_PREVIEW_GIVEN, "lfdmi_preview_params mode");
static_assert(PRV_LUT == LFDMI_PREVIEW_LUT && PRV_LUT == 16 * PRV_THREADS, "k_preview_render loads the table with one 16 B access a thread");
static_assert(sizeof(lfdmi_preview_frame) == 48 && sizeof(lfdmi_preview_params) == 16, "frame previews ABI");

extern "C" void lfdmi_default_preview_params(lfdmi_preview_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->bin = 4; o->mode = LFDMI_PREVIEW_RANK; o->lo_ppm = 10000; o->hi_ppm = 995000;
}

// step 4 of the definition, GIVEN: a finite limit as the integer a pixel of that value enters as
static long long given_fix(double x) { return llrint(std::min(std::max(x, -16777216.0), 16777216.0) * 1073741824.0); }

extern "C" int lfdmi_frame_previews(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_preview_params *pp,
                                    const double *limits, const uint8_t *lut, uint8_t *out, int out_loc, int64_t *cells,
                                    lfdmi_preview_frame *records) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_frame_previews", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (out_loc != LFDMI_HOST && out_loc != LFDMI_DEVICE && out_loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad out_loc");
    if (n < 0 || h < 1 || w < 1 || h > 65536 || w > 65536 || (double)h * (double)w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: n >= 0, h and w 1 .. 65536, h * w <= 1e9");
    lfdmi_preview_params q;
    if (pp) q = *pp; else lfdmi_default_preview_params(&q);
    int lg = -1;
    for (int k = 0; k <= 4; k++)
        if (q.bin == (1 << k)) lg = k;
    if (lg < 0) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: bin is 1, 2, 4, 8 or 16");
    if (q.mode != LFDMI_PREVIEW_RANK && q.mode != LFDMI_PREVIEW_GIVEN) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: bad mode");
    if (q.lo_ppm < 0 || q.hi_ppm > 1000000 || q.lo_ppm > q.hi_ppm)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: 0 <= lo_ppm <= hi_ppm <= 1000000");
    if (!lut) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: NULL lut");
    if (n > 0 && (!frames || !out || !records)) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    const bool given = q.mode == LFDMI_PREVIEW_GIVEN;
    std::vector<long long> hgiven;                          // (the queued copies read it: declared ahead of the pools)
    if (given) {
        if (n > 0 && !limits) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: LFDMI_PREVIEW_GIVEN needs limits");
        hgiven.resize((size_t)2 * n);
        for (int i = 0; i < 2 * n; i++) {
            if (!std::isfinite(limits[i])) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_frame_previews: a limit is not finite");
            hgiven[i] = given_fix(limits[i]);
        }
    }
    if (n == 0) return 0;

    const int b = 1 << lg;
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE, out_dev = out_loc == LFDMI_DEVICE;
    PrevDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.be = dtype == LFDMI_F32_BE; p.lg = lg;
    p.hp = (h + b - 1) / b; p.wp = (w + b - 1) / b; p.nseg = (w + PRV_SEG - 1) / PRV_SEG;
    p.mode = q.mode; p.lo_ppm = q.lo_ppm; p.hi_ppm = q.hi_ppm;
    const size_t NC = (size_t)p.hp * p.wp;
    size_t chunk = std::min<size_t>(PREVIEW_MAX_CHUNK, std::max<size_t>(1, unit->limit_of(LIM_CELL_BYTES, PREVIEW_CELL_BYTES) / (NC * 8)));
    if (!in_dev) chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, PREVIEW_STAGE_BYTES) / FB));

    hipStream_t st = ctx_stream(ctx);
    std::vector<PrevFrameDev> hrec(n);                      // (the queued copies write it: declared ahead of the pools)
    Pool keep(st);                                          // the table, for the whole call
    uint8_t *d_lut = nullptr;
    UHIP(keep.get(&d_lut, (size_t)PRV_LUT));
    UHIP(hipMemcpyAsync(d_lut, lut, PRV_LUT, hipMemcpyHostToDevice, st));
    for (int c0 = 0; c0 < n; c0 += (int)chunk) {
        const int nf = std::min<int>((int)chunk, n - c0);
        split->chunks++;
        Pool pool(st);
        uint32_t *d_buf = nullptr;
        long long *d_cells = nullptr, *d_given = nullptr;
        uint8_t *d_out = nullptr;
        PrevFrameDev *d_rec = nullptr;
        UHIP(pool.get(&d_rec, (size_t)nf));
        if (cells && out_dev) d_cells = (long long *)cells + (size_t)c0 * NC;
        else UHIP(pool.get(&d_cells, (size_t)nf * NC));
        if (out_dev) d_out = out + (size_t)c0 * NC;
        else UHIP(pool.get(&d_out, (size_t)nf * NC));
        if (given) {
            UHIP(pool.get(&d_given, (size_t)2 * nf));
            UHIP(hipMemcpyAsync(d_given, hgiven.data() + (size_t)2 * c0, (size_t)2 * nf * sizeof(long long), hipMemcpyHostToDevice, st));
        }
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * N;
        if (!in_dev) {
            UHIP(pool.get(&d_buf, (size_t)nf * N));
            UHIP(hipMemcpyAsync(d_buf, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = d_buf;
        }
        // 16 B loads: every row of every frame of the chunk starts on a 16 B boundary
        p.vec = ((uintptr_t)src % 16 == 0 && w % 4 == 0) ? 1 : 0;
        const long long items = (long long)nf * p.hp * p.nseg;
        k_preview_bin<<<(unsigned)((items + PRV_WAVES - 1) / PRV_WAVES), PRV_THREADS, 0, st>>>(src, N, p, nf, d_cells);
        ULAUNCH("k_preview_bin");
        k_preview_limits<<<nf, PRV_SEL_THREADS, 0, st>>>(d_cells, p, d_given, d_rec);
        ULAUNCH("k_preview_limits");
        const unsigned rb = (unsigned)std::min<size_t>(PREVIEW_RENDER_BLOCKS, (NC + PRV_THREADS - 1) / PRV_THREADS);
        k_preview_render<<<dim3(rb, nf), PRV_THREADS, 0, st>>>(d_cells, p, d_rec, d_lut, d_out);
        ULAUNCH("k_preview_render");
        UHIP(hipMemcpyAsync(hrec.data() + c0, d_rec, (size_t)nf * sizeof(PrevFrameDev), hipMemcpyDeviceToHost, st));
        if (!out_dev) {
            UHIP(hipMemcpyAsync(out + (size_t)c0 * NC, d_out, (size_t)nf * NC, hipMemcpyDeviceToHost, st));
            if (cells) UHIP(hipMemcpyAsync(cells + (size_t)c0 * NC, d_cells, (size_t)nf * NC * sizeof(long long), hipMemcpyDeviceToHost, st));
        }
        pool.release();                                     // (stream-ordered: behind the chunk's work, without a wait)
    }
    keep.release();
    UHIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        lfdmi_preview_frame &o = records[i];
        memset(&o, 0, sizeof(o));
        o.status = hrec[i].status;
        o.n_cells = hrec[i].n_cells;
        o.n_empty = (int32_t)(NC - (size_t)hrec[i].n_cells);
        o.lo = hrec[i].lo; o.hi = hrec[i].hi;
        o.lo_f = ldexp((double)o.lo, -30);
        o.hi_f = ldexp((double)o.hi, -30);
    }
    return 0;
}
