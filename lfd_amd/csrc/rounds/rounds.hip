// rounds.hip -- host side of the detection rounds (include/lfdmi.h: detection rounds; the kernel in k_rounds.h).  Its own
// translation unit in its own directory, like mask/: the detection kernels' code object does not change with it.  Round 0 and
// every later round are the public lfdmi_detect_batch_raw; what this unit adds between two rounds is the work copy of the frames
// that continue, with the bands of their lines so far set to +0, and the catalogue compacted to those frames.  The call keeps no
// state: the work buffer and the compacted device arrays of a round come from the stream's pool and go back after the round.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "../unit.h"
#include "k_rounds.h"

static_assert(RND_MAX_BANDS == LFDMI_ROUNDS_MAX_TRAILS - 1, "a frame's last round sees all lines but one");
static_assert(sizeof(lfdmi_rounds_params) == 24, "the header's layout");

#define FN "lfdmi_detect_rounds"

extern "C" void lfdmi_default_rounds_params(lfdmi_rounds_params *out) {
    if (!out) return;
    out->max_trails = 4;
    out->pad = 0;
    out->half = 10.0;
    out->dup_dist = 20.0;
}

static bool rec_found(const lfdmi_result &r) { return r.status == 0 && r.found != 0; }

// step 2 of the trail masks for a record's segment; false for what they call a bad segment (it has no band)
static bool rounds_geometry(const lfdmi_result &r, double half, RoundsBand &o) {
    const double x1 = (double)r.x1, y1 = (double)r.y1, x2 = (double)r.x2, y2 = (double)r.y2;
    const double c[4] = {x1, y1, x2, y2};
    for (double v : c)
        if (fabs(v) > 1e6) return false;
    const double dx = x2 - x1, dy = y2 - y1;
    const double L = sqrt(dx * dx + dy * dy);
    if (L == 0.0) return false;
    o.x1 = x1; o.y1 = y1;
    o.ex = dx / L; o.ey = dy / L;
    o.nx = -o.ey; o.ny = o.ex;
    o.half = half;
    return true;
}

// step 4: the smallest j < k whose line both end points of record k lie within dup_dist of, or -1
static int32_t rounds_dup_of(const lfdmi_result *rec, int k, double dup_dist) {
    if (!rec_found(rec[k])) return -1;
    const double px[2] = {(double)rec[k].x1, (double)rec[k].x2}, py[2] = {(double)rec[k].y1, (double)rec[k].y2};
    for (int j = 0; j < k; j++) {
        RoundsBand g;
        if (!rounds_geometry(rec[j], 0.0, g)) continue;
        bool near = true;
        for (int e = 0; e < 2; e++) {
            const double u = (px[e] - g.x1) * g.nx + (py[e] - g.y1) * g.ny;
            near = near && fabs(u) <= dup_dist;
        }
        if (near) return j;
    }
    return -1;
}

// the catalogue entries of the frames idx[0 .. m), in that order: host arrays gathered into `host`, device arrays copied
// into pool memory on the stream
struct CatHost {
    std::vector<int32_t> count, nobserve, ndetect;
    std::vector<float> rowc, colc, psfmag, petro90;
};
template <class T> static void gather_rows(std::vector<T> &dst, const T *src, const std::vector<int> &idx, size_t row) {
    dst.resize(idx.size() * row);
    for (size_t s = 0; s < idx.size(); s++) memcpy(dst.data() + s * row, src + (size_t)idx[s] * row, row * sizeof(T));
}
template <class T> static int gather_rows_dev(lfdmi_ctx *ctx, Pool &pool, hipStream_t st, const T **out, const T *src, const std::vector<int> &idx, size_t row) {
    T *d = nullptr;
    UHIP(pool.get(&d, idx.size() * row));
    for (size_t s = 0; s < idx.size() && row > 0; s++)
        UHIP(hipMemcpyAsync(d + s * row, src + (size_t)idx[s] * row, row * sizeof(T), hipMemcpyDeviceToDevice, st));
    *out = d;
    return 0;
}
static int compact_catalog(lfdmi_ctx *ctx, Pool &pool, hipStream_t st, const lfdmi_catalog *cat, const std::vector<int> &idx, CatHost &host, lfdmi_catalog *out) {
    *out = *cat;
    const size_t mo = cat->max_obj > 0 ? (size_t)cat->max_obj : 0;
    if (mo == 0) return 0;   // (remove_stars does nothing and reads nothing)
    int rc;
    if (cat->loc == LFDMI_DEVICE) {
        if ((rc = gather_rows_dev(ctx, pool, st, &out->count, cat->count, idx, 1))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->rowc, cat->rowc, idx, mo * 5))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->colc, cat->colc, idx, mo * 5))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->psfmag, cat->psfmag, idx, mo * 5))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->petro90, cat->petro90, idx, mo * 5))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->nobserve, cat->nobserve, idx, mo))) return rc;
        if ((rc = gather_rows_dev(ctx, pool, st, &out->ndetect, cat->ndetect, idx, mo))) return rc;
        return 0;
    }
    gather_rows(host.count, cat->count, idx, 1);
    gather_rows(host.rowc, cat->rowc, idx, mo * 5);
    gather_rows(host.colc, cat->colc, idx, mo * 5);
    gather_rows(host.psfmag, cat->psfmag, idx, mo * 5);
    gather_rows(host.petro90, cat->petro90, idx, mo * 5);
    gather_rows(host.nobserve, cat->nobserve, idx, mo);
    gather_rows(host.ndetect, cat->ndetect, idx, mo);
    out->count = host.count.data();
    out->rowc = host.rowc.data(); out->colc = host.colc.data(); out->psfmag = host.psfmag.data(); out->petro90 = host.petro90.data();
    out->nobserve = host.nobserve.data(); out->ndetect = host.ndetect.data();
    return 0;
}

// one later round: the frames idx[0 .. m) gathered into a work buffer with their bands blotted, detected there; tmp[s]: the record
// of frame idx[s]
static int rounds_round(lfdmi_ctx *ctx, const void *frames, int dtype, int h, int w, int loc, const lfdmi_catalog *cat,
                        const lfdmi_rs_params *rs, const lfdmi_params *bright, const lfdmi_params *dim, double half,
                        const lfdmi_result *records, int stride, int k, const std::vector<int> &idx, lfdmi_result *tmp) {
    const size_t m = idx.size(), N = (size_t)h * w;
    hipStream_t st = ctx_stream(ctx);
    std::vector<RoundsSlot> hs(m);
    const bool on_host = loc != LFDMI_DEVICE;
    for (size_t s = 0; s < m; s++) {
        RoundsSlot &sl = hs[s];
        memset(&sl, 0, sizeof(sl));
        sl.src = (int64_t)((on_host ? s : (size_t)idx[s]) * N);
        for (int j = 0; j < k; j++)
            if (rounds_geometry(records[(size_t)idx[s] * stride + j], half, sl.b[sl.nb])) sl.nb++;
    }
    Pool pool(st);
    CatHost cat_host;
    lfdmi_catalog cat_m;
    float *work = nullptr;
    RoundsSlot *d_slots = nullptr;
    UHIP(pool.get(&work, m * N));
    UHIP(pool.get(&d_slots, m));
    UHIP(hipMemcpyAsync(d_slots, hs.data(), m * sizeof(RoundsSlot), hipMemcpyHostToDevice, st));
    if (on_host)   // only the frames that continue travel, straight into their slots; the kernel then runs in place
        for (size_t s = 0; s < m; s++)
            UHIP(hipMemcpyAsync(work + s * N, (const char *)frames + (size_t)idx[s] * N * 4, N * 4, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((w + RND_TILE_W - 1) / RND_TILE_W), (unsigned)((h + RND_TILE_H - 1) / RND_TILE_H), (unsigned)m);
    k_rounds_gather<<<grid, RND_THREADS, 0, st>>>((const uint32_t *)(on_host ? (const void *)work : frames), (uint32_t *)work, d_slots, h, w,
                                                  dtype == LFDMI_F32_BE);
    ULAUNCH("k_rounds_gather");
    if (cat) {
        int rc = compact_catalog(ctx, pool, st, cat, idx, cat_host, &cat_m);
        if (rc) return rc;
    }
    // (the detect call runs on the same stream, behind the gather, and waits for it before it returns: hs and the pool's memory
    // live until then)
    int rc = lfdmi_detect_batch_raw(ctx, work, LFDMI_F32, (int)m, h, w, cat ? &cat_m : nullptr, rs, bright, dim, tmp, LFDMI_DEVICE);
    if (rc) return ctx_fail(ctx, rc, std::string(FN ": round ") + std::to_string(k) + ": " + lfdmi_last_error(ctx));
    pool.release();
    return 0;
}

extern "C" int lfdmi_detect_rounds(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, const lfdmi_catalog *cat,
                                   const lfdmi_rs_params *rs, const lfdmi_params *bright, const lfdmi_params *dim,
                                   const lfdmi_rounds_params *params, lfdmi_result *records, int32_t *n_found, int32_t *dup_of, int loc) {
    if (!ctx) return LFDMI_ERR_ARG;
    lfdmi_rounds_params rp;
    lfdmi_default_rounds_params(&rp);
    if (params) rp = *params;
    if (rp.max_trails < 1 || rp.max_trails > LFDMI_ROUNDS_MAX_TRAILS)
        return ctx_fail(ctx, LFDMI_ERR_ARG, FN ": max_trails must be 1 .. LFDMI_ROUNDS_MAX_TRAILS");
    if (!std::isfinite(rp.half) || rp.half < 0.0) return ctx_fail(ctx, LFDMI_ERR_ARG, FN ": half must be finite and >= 0");
    if (!std::isfinite(rp.dup_dist) || rp.dup_dist < 0.0) return ctx_fail(ctx, LFDMI_ERR_ARG, FN ": dup_dist must be finite and >= 0");
    if (!records || !n_found || !dup_of) return ctx_fail(ctx, LFDMI_ERR_ARG, FN ": NULL records, n_found or dup_of");
    int rc = unit_dtype(ctx, FN, dtype);
    if (rc) return rc;
    if (n < 0) return ctx_fail(ctx, LFDMI_ERR_ARG, FN ": bad shape");
    // (only now is the context touched: not while calls are in flight; its device; no stale error)
    if ((rc = ctx_begin(ctx))) return ctx_fail(ctx, rc, std::string(FN ": ") + lfdmi_last_error(ctx));
    const int K = rp.max_trails;

    // round 0: the plain call, which refuses what it refuses before it touches anything.  With K == 1 its records go straight
    // into the caller's array and nothing is allocated.
    std::vector<lfdmi_result> tmp(K > 1 && n > 0 ? (size_t)n : 0);
    rc = lfdmi_detect_batch_raw(ctx, frames, dtype, n, h, w, cat, rs, bright, dim, K > 1 ? tmp.data() : records, loc);
    if (rc) return ctx_fail(ctx, rc, std::string(FN ": ") + lfdmi_last_error(ctx));
    if (K == 1) {
        for (int i = 0; i < n; i++) { n_found[i] = rec_found(records[i]); dup_of[i] = -1; }
        return 0;
    }
    memset(records, 0, (size_t)n * K * sizeof(lfdmi_result));
    std::vector<int> alive;
    for (int i = 0; i < n; i++) {
        records[(size_t)i * K] = tmp[i];
        for (int k = 0; k < K; k++) dup_of[(size_t)i * K + k] = -1;
        n_found[i] = rec_found(tmp[i]);
        if (n_found[i]) alive.push_back(i);
    }
    // big-endian frames on the device were swapped in place by round 0 and are native from here on
    const int src_dtype = dtype == LFDMI_F32_BE && loc == LFDMI_DEVICE ? LFDMI_F32 : dtype;
    for (int k = 1; k < K && !alive.empty(); k++) {
        rc = rounds_round(ctx, frames, src_dtype, h, w, loc, cat, rs, bright, dim, rp.half, records, K, k, alive, tmp.data());
        if (rc) return rc;
        std::vector<int> next;
        for (size_t s = 0; s < alive.size(); s++) {
            const int i = alive[s];
            lfdmi_result *rec = records + (size_t)i * K;
            rec[k] = tmp[s];
            dup_of[(size_t)i * K + k] = rounds_dup_of(rec, k, rp.dup_dist);
            if (rec_found(rec[k])) { n_found[i] = k + 1; next.push_back(i); }
        }
        alive.swap(next);
    }
    return 0;
}
