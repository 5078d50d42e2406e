// stars.hip -- host side of the source finder (include/lfdmi.h: source finder; kernels in k_stars.h).  Its own translation unit in
// its own directory, like sky/, inject/, radon/ and stack/: the detection kernels' code object does not change with it.  The
// context's internals are reached through unit.h.  The calls keep no state: their device memory comes from the stream's pool
// (hipMallocAsync) and goes back before they return.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_stars.h"

#define STARS_STAGE_BYTES (1ull << 30)   // device staging of host frames at a time
#define STARS_REC_BYTES (256ull << 20)   // records of one chunk
#define STARS_MAX_CHUNK 32768            // frames of one launch (they go in grid.z / grid.y)

static_assert(sizeof(StarRec) == sizeof(lfdmi_star), "lfdmi_star layout");
static_assert(sizeof(StarsFrameDev) == sizeof(lfdmi_stars_frame), "lfdmi_stars_frame layout");
static_assert(STR_EXTENDED == LFDMI_STAR_EXTENDED && STR_EDGE == LFDMI_STAR_EDGE, "lfdmi_star flags");

extern "C" void lfdmi_default_stars_params(lfdmi_stars_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->k_det = 5.0; o->k_edge = 3.0; o->edge_frac = 0.02;
    o->sep = 3; o->r_max = 32; o->max_obj = 4096;
}

static bool stars_params_ok(const lfdmi_stars_params &q) {
    if (!std::isfinite(q.k_det) || !(q.k_det > 0) || !std::isfinite(q.k_edge) || !(q.k_edge > 0)) return false;
    if (!(q.edge_frac >= 0.0 && q.edge_frac <= 1.0)) return false;
    return q.sep >= 1 && q.sep <= STR_MAX_SEP && q.r_max >= 1 && q.r_max <= STR_MAX_R && q.max_obj >= 1 && q.max_obj <= LFDMI_STARS_MAX_OBJ;
}

extern "C" int lfdmi_find_stars(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                                const lfdmi_stars_params *pp, lfdmi_star *out_records, int out_loc, lfdmi_stars_frame *frame_records) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_find_stars", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (out_loc != LFDMI_HOST && out_loc != LFDMI_DEVICE && out_loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad out_loc");
    if (n < 0 || h < 1 || w < 1 || h > 65536 || w > 65536) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_find_stars: n >= 0, h and w 1 .. 65536");
    if (n > 0 && (!frames || !out_records || !frame_records)) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    lfdmi_stars_params q;
    if (pp) q = *pp; else lfdmi_default_stars_params(&q);
    if (!stars_params_ok(q)) return ctx_fail(ctx, LFDMI_ERR_ARG, "stars params out of range (include/lfdmi.h: lfdmi_stars_params)");
    std::vector<float> sg;
    if ((rc = unit_sigma(ctx, "lfdmi_find_stars", sigma, n, &sg))) return rc;
    if (n == 0) return 0;

    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE, out_dev = out_loc == LFDMI_DEVICE;
    StarsDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.be = dtype == LFDMI_F32_BE; p.sep = q.sep; p.r_max = q.r_max; p.max_obj = q.max_obj;
    p.wq = (w + 63) >> 6;
    p.edge_frac = q.edge_frac;
    // definition steps 2 and 4: the two thresholds that depend on the frame's sigma alone
    std::vector<float> hT(n), hE(n);
    for (int i = 0; i < n; i++) {
        hT[i] = (float)(q.k_det * 3.0 * (double)sg[i]);
        hE[i] = (float)(q.k_edge * 3.0 * (double)sg[i]);
    }
    size_t chunk = STARS_MAX_CHUNK;
    if (!in_dev) chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, STARS_STAGE_BYTES) / FB));
    if (!out_dev)
        chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_STARS_REC_BYTES, STARS_REC_BYTES) / ((size_t)q.max_obj * sizeof(StarRec))));

    hipStream_t st = ctx_stream(ctx);
    std::vector<StarsFrameDev> hrec(n);   // (the queued copies write it: declared ahead of the pools, which wait before they go)
    for (int c0 = 0; c0 < n; c0 += (int)chunk) {
        const int nf = std::min<int>((int)chunk, n - c0);
        split->chunks++;
        Pool pool(st);
        uint32_t *d_buf = nullptr;
        str_u64 *d_bits = nullptr;
        int *d_rs = nullptr;
        float *d_T = nullptr, *d_E = nullptr;
        StarsFrameDev *d_frec = nullptr;
        StarRec *d_rec = nullptr;
        UHIP(pool.get(&d_bits, (size_t)nf * h * p.wq));
        UHIP(pool.get(&d_rs, (size_t)nf * (h + 1)));
        UHIP(pool.get(&d_T, (size_t)nf));
        UHIP(pool.get(&d_E, (size_t)nf));
        UHIP(pool.get(&d_frec, (size_t)nf));
        const size_t nrec = (size_t)nf * q.max_obj;
        if (out_dev) d_rec = (StarRec *)out_records + (size_t)c0 * q.max_obj;
        else UHIP(pool.get(&d_rec, nrec));
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * N;
        if (!in_dev) {
            UHIP(pool.get(&d_buf, (size_t)nf * N));
            UHIP(hipMemcpyAsync(d_buf, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = d_buf;
        }
        UHIP(hipMemcpyAsync(d_T, hT.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_E, hE.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_rec, 0, nrec * sizeof(StarRec), st));   // rows past n_out are zero
        k_stars_detect<<<dim3(p.wq, (h + STR_TH - 1) / STR_TH, nf), STR_THREADS, 0, st>>>(src, N, p, d_T, d_bits);
        ULAUNCH("k_stars_detect");
        k_stars_rows<<<nf, STR_THREADS, 0, st>>>(p, d_bits, d_rs, d_frec);
        ULAUNCH("k_stars_rows");
        UHIP(hipMemcpyAsync(hrec.data() + c0, d_frec, (size_t)nf * sizeof(StarsFrameDev), hipMemcpyDeviceToHost, st));
        UHIP(hipStreamSynchronize(st));
        int slots = 0;
        for (int i = 0; i < nf; i++) slots = std::max(slots, hrec[c0 + i].n_out);
        if (slots > 0) {
            k_stars_measure<<<dim3(slots, nf), STR_THREADS, 0, st>>>(src, N, p, d_E, d_bits, d_rs, d_rec);
            ULAUNCH("k_stars_measure");
        }
        if (!out_dev) UHIP(hipMemcpyAsync((StarRec *)out_records + (size_t)c0 * q.max_obj, d_rec, nrec * sizeof(StarRec), hipMemcpyDeviceToHost, st));
        pool.release();
        UHIP(hipStreamSynchronize(st));
    }
    for (int i = 0; i < n; i++) {
        frame_records[i].status = hrec[i].status ? LFDMI_STARS_TRUNCATED : LFDMI_STARS_OK;
        frame_records[i].n_found = hrec[i].n_found;
        frame_records[i].n_out = hrec[i].n_out;
    }
    return 0;
}

extern "C" int lfdmi_stars_catalog(lfdmi_ctx *ctx, const lfdmi_star *records, int rec_loc, const lfdmi_stars_frame *frame_records, int n,
                                   int max_obj, double pixscale, const lfdmi_catalog *cat) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if ((rc = unit_loc(ctx, rec_loc))) return rc;
    if (n < 0 || max_obj < 1 || max_obj > LFDMI_STARS_MAX_OBJ || n > STARS_MAX_CHUNK)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stars_catalog: n 0 .. 32768, max_obj 1 .. LFDMI_STARS_MAX_OBJ");
    if (!std::isfinite(pixscale) || !(pixscale > 0)) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stars_catalog: pixscale must be positive");
    if (!cat || (n > 0 && (!records || !frame_records))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if ((rc = unit_loc(ctx, cat->loc))) return rc;
    if (cat->max_obj != max_obj) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stars_catalog: the catalogue's max_obj differs");
    if (n > 0 && (!cat->count || !cat->rowc || !cat->colc || !cat->psfmag || !cat->petro90 || !cat->nobserve || !cat->ndetect))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if (n == 0) return 0;
    for (int i = 0; i < n; i++)
        if (frame_records[i].n_out < 0 || frame_records[i].n_out > max_obj)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stars_catalog: frame " + std::to_string(i) + ": n_out outside [0, max_obj]");

    hipStream_t st = ctx_stream(ctx);
    const size_t rows = (size_t)n * max_obj;
    const bool cat_dev = cat->loc == LFDMI_DEVICE;
    std::vector<int> hn(n);   // (declared ahead of the pool: the queued copy reads it)
    for (int i = 0; i < n; i++) hn[i] = frame_records[i].n_out;
    Pool pool(st);
    int *d_n = nullptr;
    UHIP(pool.get(&d_n, (size_t)n));
    UHIP(hipMemcpyAsync(d_n, hn.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    const StarRec *d_rec = (const StarRec *)records;
    if (rec_loc != LFDMI_DEVICE) {
        StarRec *up = nullptr;
        UHIP(pool.get(&up, rows));
        UHIP(hipMemcpyAsync(up, records, rows * sizeof(StarRec), hipMemcpyHostToDevice, st));
        d_rec = up;
    }
    int *count = (int *)cat->count, *nob = (int *)cat->nobserve, *nde = (int *)cat->ndetect;
    float *f5[4] = {(float *)cat->rowc, (float *)cat->colc, (float *)cat->psfmag, (float *)cat->petro90};
    if (!cat_dev) {
        UHIP(pool.get(&count, (size_t)n));
        UHIP(pool.get(&nob, rows));
        UHIP(pool.get(&nde, rows));
        for (float *&a : f5) UHIP(pool.get(&a, rows * 5));
    }
    k_stars_catalog<<<dim3((max_obj + STR_THREADS - 1) / STR_THREADS, n), STR_THREADS, 0, st>>>(d_rec, d_n, max_obj, pixscale, count, f5[0], f5[1],
                                                                                           f5[2], f5[3], nob, nde);
    ULAUNCH("k_stars_catalog");
    if (!cat_dev) {
        UHIP(hipMemcpyAsync((void *)cat->count, count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync((void *)cat->nobserve, nob, rows * sizeof(int), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync((void *)cat->ndetect, nde, rows * sizeof(int), hipMemcpyDeviceToHost, st));
        const float *dst[4] = {cat->rowc, cat->colc, cat->psfmag, cat->petro90};
        for (int k = 0; k < 4; k++) UHIP(hipMemcpyAsync((void *)dst[k], f5[k], rows * 5 * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    pool.release();
    UHIP(hipStreamSynchronize(st));
    return 0;
}
