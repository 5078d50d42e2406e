// psf.hip -- host side of the frame seeing (include/lfdmi.h: frame seeing; kernels in k_psf.h).  Its own translation unit in its
// own directory, like stars/: no other unit's code object changes with it.  The call keeps no state: its device memory comes
// from the stream's pool (hipMallocAsync) and goes back before it returns.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_psf.h"

#define PSF_STAGE_BYTES (1ull << 30)   // device staging of host frames at a time
#define PSF_REC_BYTES (256ull << 20)   // host records staged, and per-record sums, of one chunk
#define PSF_MAX_CHUNK 32768            // frames of one launch (they go in grid.y)
#define PSF_MAX_OBJ 1048576            // LFDMI_STARS_MAX_OBJ

static_assert(sizeof(PsfStarRec) == sizeof(lfdmi_star), "lfdmi_star layout");
static_assert(sizeof(PsfStarDev) == sizeof(lfdmi_psf_star) && sizeof(lfdmi_psf_star) == 64, "lfdmi_psf_star layout");
static_assert(sizeof(lfdmi_seeing_frame) == 64 && sizeof(lfdmi_psf_params) == 56, "frame seeing layouts");
static_assert(PSF_OK == LFDMI_PSF_OK && PSF_NOT_CANDIDATE == LFDMI_PSF_NOT_CANDIDATE && PSF_CLIPPED == LFDMI_PSF_CLIPPED &&
                  PSF_CROWDED == LFDMI_PSF_CROWDED && PSF_BAD_PIXEL == LFDMI_PSF_BAD_PIXEL && PSF_MAX_OBJ == LFDMI_STARS_MAX_OBJ,
              "LFDMI_PSF_* statuses");

extern "C" void lfdmi_default_psf_params(lfdmi_psf_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->k_peak = 50.0; o->e_max = 0.2; o->sat = LFDMI_PSF_MAX_SAT;
    o->win = 7; o->gap = 2; o->ring = 3; o->iso = 12; o->rad_max = 16; o->min_stars = 5; o->max_used = 256;
}

static bool psf_params_ok(const lfdmi_psf_params &q) {
    if (!std::isfinite(q.k_peak) || !(q.k_peak > 0)) return false;
    if (!(q.e_max >= 0.0 && q.e_max <= 1.0)) return false;
    if (!(q.sat > 0.0 && q.sat <= LFDMI_PSF_MAX_SAT)) return false;
    return q.win >= 1 && q.win <= 16 && q.gap >= 0 && q.gap <= 8 && q.ring >= 1 && q.ring <= 8 && q.iso >= 1 && q.iso <= 64 &&
           q.rad_max >= 1 && q.rad_max <= 32 && q.min_stars >= 1 && q.min_stars <= 1024 && q.max_used >= 1 && q.max_used <= 1024;
}

static double lower_median(std::vector<double> &v) {
    std::sort(v.begin(), v.end());
    return v[(v.size() - 1) / 2];
}

// step 5 of the definition for one frame: its packed stars -> the doubles and n_used of its record
static void psf_frame_seeing(const lfdmi_psf_star *s, int n_packed, const lfdmi_psf_params &q, lfdmi_seeing_frame *o) {
    std::vector<double> wd, el;
    for (int k = 0; k < n_packed; k++) {
        if (s[k].Q0 <= 0) continue;
        const double q0 = (double)s[k].Q0;
        const double mx = (double)s[k].Qx / q0, my = (double)s[k].Qy / q0;
        const double sxx = (double)s[k].Qxx / q0 - mx * mx, syy = (double)s[k].Qyy / q0 - my * my, sxy = (double)s[k].Qxy / q0 - mx * my;
        if (!(sxx > 0.0) || !(syy > 0.0)) continue;
        const double t = sxx + syy, d = sxx - syy;
        const double e = sqrt(d * d + 4.0 * (sxy * sxy)) / t;
        if (!(e <= q.e_max)) continue;
        wd.push_back(2.3548200450309493 * sqrt(t / 2.0));
        el.push_back(e);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    o->n_used = (int32_t)wd.size();
    o->fwhm_px = o->scatter = o->ell = nan;
    if (!wd.empty()) {
        const double med = lower_median(wd);
        for (double &x : wd) x = fabs(x - med);
        o->fwhm_px = med;
        o->scatter = 1.4826 * lower_median(wd);
        o->ell = lower_median(el);
    }
    o->status = o->n_used < q.min_stars ? LFDMI_SEEING_FEW : LFDMI_SEEING_OK;
}

extern "C" int lfdmi_measure_seeing(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                                    const lfdmi_star *records, int rec_loc, const lfdmi_stars_frame *frame_records, int max_obj,
                                    const lfdmi_psf_params *pp, lfdmi_psf_star *out_stars, lfdmi_seeing_frame *out_frames) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_measure_seeing", dtype)) || (rc = unit_loc(ctx, loc)) || (rc = unit_loc(ctx, rec_loc))) return rc;
    if (n < 0 || h < 1 || w < 1 || h > 65536 || w > 65536) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_measure_seeing: n >= 0, h and w 1 .. 65536");
    if (max_obj < 1 || max_obj > PSF_MAX_OBJ) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_measure_seeing: max_obj 1 .. LFDMI_STARS_MAX_OBJ");
    if (n > 0 && (!frames || !records || !frame_records || !out_stars || !out_frames)) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    lfdmi_psf_params q;
    if (pp) q = *pp; else lfdmi_default_psf_params(&q);
    if (!psf_params_ok(q)) return ctx_fail(ctx, LFDMI_ERR_ARG, "psf params out of range (include/lfdmi.h: lfdmi_psf_params)");
    std::vector<float> sg;
    if ((rc = unit_sigma(ctx, "lfdmi_measure_seeing", sigma, n, &sg))) return rc;
    for (int i = 0; i < n; i++)
        if (frame_records[i].n_out < 0 || frame_records[i].n_out > max_obj)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_measure_seeing: frame " + std::to_string(i) + ": n_out outside [0, max_obj]");
    if (n == 0) return 0;

    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE, rec_dev = rec_loc == LFDMI_DEVICE;
    PsfDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.be = dtype == LFDMI_F32_BE; p.max_obj = max_obj;
    p.win = q.win; p.gap = q.gap; p.ring = q.ring; p.iso = q.iso; p.rad_max = q.rad_max; p.max_used = q.max_used;
    const float satf = (float)q.sat;            // (positive and finite: its bits order as its value)
    memcpy(&p.sat_bits, &satf, sizeof(satf));
    std::vector<float> hfloor(n);
    std::vector<int> hn(n);
    for (int i = 0; i < n; i++) {
        hfloor[i] = (float)(q.k_peak * 3.0 * (double)sg[i]);
        hn[i] = frame_records[i].n_out;
    }
    const size_t rec_lim = unit->limit_of(LIM_STARS_REC_BYTES, PSF_REC_BYTES);
    size_t chunk = std::min<size_t>(PSF_MAX_CHUNK, std::max<size_t>(1, rec_lim / ((size_t)max_obj * sizeof(PsfStarDev))));
    if (!in_dev) chunk = std::min(chunk, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, PSF_STAGE_BYTES) / FB));

    hipStream_t st = ctx_stream(ctx);
    std::vector<PsfFrameDev> hrec(n);           // (the queued copies write it: declared ahead of the pools, which wait before they go)
    for (int c0 = 0; c0 < n; c0 += (int)chunk) {
        const int nf = std::min<int>((int)chunk, n - c0);
        split->chunks++;
        int slots = 0;
        for (int i = 0; i < nf; i++) slots = std::max(slots, hn[c0 + i]);
        Pool pool(st);
        uint32_t *d_buf = nullptr;
        PsfStarRec *d_up = nullptr;
        int *d_n = nullptr;
        float *d_floor = nullptr;
        uint8_t *d_status = nullptr;
        PsfStarDev *d_sums = nullptr, *d_out = nullptr;
        PsfFrameDev *d_frec = nullptr;
        const size_t nrec = (size_t)nf * max_obj, nout = (size_t)nf * q.max_used;
        UHIP(pool.get(&d_n, (size_t)nf));
        UHIP(pool.get(&d_floor, (size_t)nf));
        UHIP(pool.get(&d_status, nrec));
        UHIP(pool.get(&d_sums, nrec));
        UHIP(pool.get(&d_out, nout));
        UHIP(pool.get(&d_frec, (size_t)nf));
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * N;
        if (!in_dev) {
            UHIP(pool.get(&d_buf, (size_t)nf * N));
            UHIP(hipMemcpyAsync(d_buf, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = d_buf;
        }
        const PsfStarRec *d_rec = (const PsfStarRec *)records + (size_t)c0 * max_obj;
        if (!rec_dev) {
            UHIP(pool.get(&d_up, nrec));
            UHIP(hipMemcpyAsync(d_up, d_rec, nrec * sizeof(PsfStarRec), hipMemcpyHostToDevice, st));
            d_rec = d_up;
        }
        UHIP(hipMemcpyAsync(d_n, hn.data() + c0, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_floor, hfloor.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_out, 0, nout * sizeof(PsfStarDev), st));   // rows past n_packed are zero
        if (slots > 0) {
            k_psf_measure<<<dim3((slots + PSF_WAVES - 1) / PSF_WAVES, nf), PSF_THREADS, 0, st>>>(src, N, p, d_rec, d_n, d_floor, d_status, d_sums);
            ULAUNCH("k_psf_measure");
        }
        k_psf_pack<<<nf, PSF_THREADS, 0, st>>>(p, d_n, d_status, d_sums, d_out, d_frec);
        ULAUNCH("k_psf_pack");
        UHIP(hipMemcpyAsync(out_stars + (size_t)c0 * q.max_used, d_out, nout * sizeof(PsfStarDev), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(hrec.data() + c0, d_frec, (size_t)nf * sizeof(PsfFrameDev), hipMemcpyDeviceToHost, st));
        pool.release();
        UHIP(hipStreamSynchronize(st));
    }
    for (int i = 0; i < n; i++) {
        lfdmi_seeing_frame o;
        memset(&o, 0, sizeof(o));
        const PsfFrameDev &r = hrec[i];
        o.n_ok = r.n_ok; o.n_packed = r.n_packed;
        o.n_not_candidate = r.count[PSF_NOT_CANDIDATE]; o.n_clipped = r.count[PSF_CLIPPED];
        o.n_crowded = r.count[PSF_CROWDED]; o.n_bad_pixel = r.count[PSF_BAD_PIXEL];
        o.n_cand = hn[i] - o.n_not_candidate;
        psf_frame_seeing(out_stars + (size_t)i * q.max_used, o.n_packed, q, &o);
        out_frames[i] = o;
    }
    return 0;
}
