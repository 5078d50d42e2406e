// lc.hip -- host side of the light curves (include/lfdmi.h: light curves; kernels in k_lc.h).  Its own translation unit in its own
// directory, like mask/: the detection kernels' code object does not change with it.  The context's internals are reached
// through unit.h.  The call keeps no state: its device memory comes from the stream's pool (hipMallocAsync) and goes back before
// the call's one wait.  The device returns five integers per (segment, section); every double of a record is made here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_lc.h"

static_assert(sizeof(lfdmi_lc_segment) == 64 && sizeof(lfdmi_lc_params) == 24 && sizeof(lfdmi_lc) == 88 && sizeof(lfdmi_lc_section) == 112,
              "the header's layouts");
static_assert(sizeof(LcSeg) == 96, "a chunk of segments is 12 KB of LDS");

#define LC_LIST_MAX (8u << 20)         // (job, tile) pairs listed at a time: 64 MB
#define LC_STAGE_BYTES (512ull << 20)  // device staging of host frames and host planes at a time
#define LC_RENDER_BLOCKS 2048          // persistent blocks that walk the list

static const double kNaN = std::numeric_limits<double>::quiet_NaN();

extern "C" void lfdmi_default_lc_params(lfdmi_lc_params *out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->sec_len = 32.0;
    out->clip = 0.125f;
    out->min_core = 32;
    out->min_sky = 32;
}

// step 2 of the definition: LFDMI_LC_OK, LFDMI_LC_BAD_SEGMENT or LFDMI_LC_TOO_LONG
static int lc_geometry(const lfdmi_lc_segment &s, double inv, int max_sec, LcSeg &o) {
    const double c[4] = {s.x1, s.y1, s.x2, s.y2};
    for (double v : c)
        if (!std::isfinite(v) || fabs(v) > 1e6) return LFDMI_LC_BAD_SEGMENT;
    if (!std::isfinite(s.half) || !(s.half > 0.0)) return LFDMI_LC_BAD_SEGMENT;
    if (std::isnan(s.bg_in) || std::isnan(s.bg_out)) return LFDMI_LC_BAD_SEGMENT;
    if (s.bg_in < s.half || s.bg_out < s.bg_in || s.bg_out > LFDMI_LC_MAX_BG) return LFDMI_LC_BAD_SEGMENT;
    const double dx = s.x2 - s.x1, dy = s.y2 - s.y1;
    const double L = sqrt(dx * dx + dy * dy);
    if (L == 0.0) return LFDMI_LC_BAD_SEGMENT;
    const double ns = ceil(L * inv);
    if (ns > (double)max_sec) return LFDMI_LC_TOO_LONG;
    o.x1 = s.x1; o.y1 = s.y1;
    o.ex = dx / L; o.ey = dy / L;
    o.nx = -o.ey; o.ny = o.ex;
    o.half = s.half; o.bg_in = s.bg_in; o.bg_out = s.bg_out;
    o.L = L; o.inv = inv;
    o.n_sec = std::max(1, (int)ns);
    o.base = 0;
    return LFDMI_LC_OK;
}

// step 5 of the definition
static void lc_section(int j, const int32_t *c, const int64_t *q, const LcSeg &g, const lfdmi_lc_params &p, double sigma, lfdmi_lc_section &o) {
    memset(&o, 0, sizeof(o));
    o.n_geom = c[0]; o.n_core = c[1]; o.n_sky = c[2];
    o.q_core = q[0]; o.q_sky = q[1];
    o.t0 = (double)j * p.sec_len;
    o.t1 = std::min((double)(j + 1) * p.sec_len, g.L);
    o.mean = o.bkg = o.sb = o.flux = o.flux_err = o.rate = o.rate_err = o.coverage = kNaN;
    if (o.n_geom == 0) { o.status = LFDMI_LC_SEC_EMPTY; return; }
    if (o.n_core < p.min_core || o.n_sky < p.min_sky) { o.status = LFDMI_LC_SEC_LOW; return; }
    o.status = LFDMI_LC_SEC_OK;
    const double nc = (double)o.n_core, ns = (double)o.n_sky, width = 2.0 * g.half;
    const double s_core = (double)o.q_core * 9.313225746154785e-10, s_sky = (double)o.q_sky * 9.313225746154785e-10;   // 2^-30
    o.mean = s_core / nc;
    o.bkg = s_sky / ns;
    o.sb = o.mean - o.bkg;
    o.flux = o.sb * nc;
    o.flux_err = sigma * sqrt(nc + nc * nc / ns);
    o.rate = o.sb * width;
    o.rate_err = sigma * sqrt(1.0 / nc + 1.0 / ns) * width;
    o.coverage = nc / (double)o.n_geom;
}

// step 6 of the definition, from the segment's section records
static void lc_record(const lfdmi_lc_section *sec, int n_sec, lfdmi_lc &o) {
    memset(&o, 0, sizeof(o));
    o.n_sec = n_sec;
    o.first_ok = o.last_ok = o.peak_section = -1;
    o.mean_rate = o.mean_rate_err = o.chi2 = o.peak_rate = o.length = o.flux = o.flux_err = kNaN;
    double num = 0.0, den = 0.0, w = 0.0, len = 0.0;
    for (int j = 0; j < n_sec; j++) {
        const lfdmi_lc_section &s = sec[j];
        if (s.status != LFDMI_LC_SEC_OK) continue;
        if (o.n_ok == 0) o.first_ok = j;
        o.last_ok = j;
        o.n_ok++;
        num = num + (double)s.n_core * s.rate;
        den = den + (double)s.n_core;
        w = w + 1.0 / (s.rate_err * s.rate_err);
        len = len + (s.t1 - s.t0);
        if (o.peak_section < 0 || s.rate > o.peak_rate) { o.peak_section = j; o.peak_rate = s.rate; }
    }
    o.dof = o.n_ok - 1;
    if (o.n_ok == 0) { o.status = LFDMI_LC_EMPTY; return; }
    o.status = LFDMI_LC_OK;
    o.mean_rate = num / den;
    o.mean_rate_err = 1.0 / sqrt(w);
    double chi2 = 0.0;
    for (int j = 0; j < n_sec; j++) {
        const lfdmi_lc_section &s = sec[j];
        if (s.status != LFDMI_LC_SEC_OK) continue;
        const double d = (s.rate - o.mean_rate) / s.rate_err;
        chi2 = chi2 + d * d;
    }
    o.chi2 = chi2;
    o.length = len;
    o.flux = o.mean_rate * len;
    o.flux_err = o.mean_rate_err * len;
}

extern "C" int lfdmi_light_curves(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                                  const lfdmi_lc_segment *segs, int n_seg, const float *sigma, const lfdmi_lc_params *pp, lfdmi_lc *out,
                                  lfdmi_lc_section *sections, int max_sections_per_seg) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_light_curves", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (n < 0 || n_seg < 0 || h < 1 || w < 1 || h > 65536 || w > 65536 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: n, n_seg >= 0, h and w 1 .. 65536, h * w at most 1e9");
    if ((n > 0 && !frames) || (n_seg > 0 && (!segs || !out || !sections))) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: NULL argument");
    if (max_sections_per_seg < 1 || max_sections_per_seg > LFDMI_LC_MAX_SECTIONS)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: max_sections_per_seg 1 .. LFDMI_LC_MAX_SECTIONS");
    if (skip_bits < 0 || skip_bits > 255) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: skip_bits 0 .. 255");
    lfdmi_lc_params q;
    if (pp) q = *pp; else lfdmi_default_lc_params(&q);
    if (!(q.sec_len >= 8.0 && q.sec_len <= 4096.0) || !std::isfinite(q.clip) || !(q.clip > 0.0f && q.clip <= 1024.0f) || q.min_core < 1 ||
        q.min_sky < 1)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: params out of range (include/lfdmi.h: lfdmi_lc_params)");
    for (int i = 0; i < n_seg; i++)
        if (segs[i].frame < 0 || segs[i].frame >= n)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_light_curves: segment " + std::to_string(i) + ": frame outside [0, n)");
    std::vector<float> sig;
    if ((rc = unit_sigma(ctx, "lfdmi_light_curves", sigma, n, &sig))) return rc;
    if (n_seg == 0) return 0;

    // good segments by frame (a counting sort); one job per frame that carries one; the sections of the good segments in a row
    const size_t N = (size_t)h * w, FB = N * sizeof(float);
    const double inv = 1.0 / q.sec_len;
    std::vector<LcSeg> geo(n_seg);
    std::vector<int> status(n_seg);
    std::vector<int> start(n + 1, 0);
    for (int i = 0; i < n_seg; i++) {
        status[i] = lc_geometry(segs[i], inv, max_sections_per_seg, geo[i]);
        if (status[i] == LFDMI_LC_OK) start[segs[i].frame + 1]++;
    }
    for (int f = 0; f < n; f++) start[f + 1] += start[f];
    const int ng = start[n];
    std::vector<LcSeg> hs(ng);
    std::vector<int> place(n_seg, -1);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int i = 0; i < n_seg; i++)
            if (status[i] == LFDMI_LC_OK) {
                place[i] = at[segs[i].frame]++;
                hs[place[i]] = geo[i];
            }
    }
    size_t nsec = 0;
    for (int k = 0; k < ng; k++) { hs[k].base = (int32_t)nsec; nsec += (size_t)hs[k].n_sec; }
    if (nsec > (size_t)1 << 30) return ctx_fail(ctx, LFDMI_ERR_CAPACITY, "lfdmi_light_curves: more than 2^30 sections in one call");

    LcDev p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.ntx = (w + LC_TILE_W - 1) / LC_TILE_W; p.nty = (h + LC_TILE_H - 1) / LC_TILE_H;
    p.be = dtype == LFDMI_F32_BE;
    p.skip_bits = mask ? (uint32_t)skip_bits : 0u;
    memcpy(&p.clip_bits, &q.clip, sizeof(float));
    const size_t ntiles = (size_t)p.ntx * p.nty;

    // chunks of jobs: the list of a chunk holds at most LC_LIST_MAX pairs, what a chunk stages at most LC_STAGE_BYTES
    const bool stage = loc != LFDMI_DEVICE, m_stage = stage && mask;
    size_t CH = std::max<size_t>(1, unit->limit_of(LIM_LIST_PAIRS, LC_LIST_MAX) / ntiles);
    if (stage) CH = std::min(CH, std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, LC_STAGE_BYTES) / (FB + (m_stage ? N : 0))));
    const size_t walk_max = unit->limit_of(LIM_RENDER_BLOCKS, LC_RENDER_BLOCKS);
    std::vector<LcJob> hj;
    std::vector<int> jframe;
    for (int f = 0; f < n; f++)
        if (start[f + 1] > start[f]) {
            LcJob j;
            j.foff = j.moff = (int64_t)((stage ? hj.size() % CH : (size_t)f) * N);
            j.sb = start[f]; j.se = start[f + 1];
            hj.push_back(j);
            jframe.push_back(f);
        }
    const size_t nj = hj.size();
    CH = std::min(CH, std::max<size_t>(nj, 1));

    hipStream_t st = ctx_stream(ctx);
    std::vector<int32_t> hcnt(3 * nsec, 0);
    std::vector<int64_t> hq(2 * nsec, 0);
    if (nj > 0) {
        Pool pool(st);
        LcSeg *d_seg = nullptr;
        LcJob *d_job = nullptr;
        uint32_t *d_buf = nullptr;
        uint8_t *d_mbuf = nullptr;
        int2 *d_list = nullptr;
        int *d_count = nullptr, *d_cnt = nullptr;
        unsigned long long *d_q = nullptr;
        UHIP(pool.get(&d_seg, (size_t)ng));
        UHIP(pool.get(&d_job, nj));
        UHIP(pool.get(&d_list, CH * ntiles));
        UHIP(pool.get(&d_count, 1));
        UHIP(pool.get(&d_cnt, 3 * nsec));
        UHIP(pool.get(&d_q, 2 * nsec));
        if (stage) UHIP(pool.get(&d_buf, CH * N));
        if (m_stage) UHIP(pool.get(&d_mbuf, CH * N));
        UHIP(hipMemcpyAsync(d_seg, hs.data(), (size_t)ng * sizeof(LcSeg), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(d_job, hj.data(), nj * sizeof(LcJob), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(d_cnt, 0, 3 * nsec * sizeof(int), st));
        UHIP(hipMemsetAsync(d_q, 0, 2 * nsec * sizeof(unsigned long long), st));
        const uint32_t *fbase = stage ? d_buf : (const uint32_t *)frames;
        const uint8_t *mbase = !mask ? nullptr : m_stage ? d_mbuf : mask;
        p.vec = w % 4 == 0 && (uintptr_t)fbase % 16 == 0;
        p.mvec = mbase && w % 4 == 0 && (uintptr_t)mbase % 4 == 0;
        for (size_t j0 = 0; j0 < nj; j0 += CH) {
            const size_t c = std::min(CH, nj - j0);
            for (size_t k = 0; k < c; k++) {
                const size_t f = (size_t)jframe[j0 + k];
                if (stage) UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + f * FB, FB, hipMemcpyHostToDevice, st));
                if (m_stage) UHIP(hipMemcpyAsync(d_mbuf + k * N, mask + f * N, N, hipMemcpyHostToDevice, st));
            }
            UHIP(hipMemsetAsync(d_count, 0, sizeof(int), st));
            const size_t pairs = c * ntiles, walk = std::min(pairs, walk_max);
            split->chunks++;
            split->grid = std::max<int64_t>(split->grid, (int64_t)walk);
            k_lc_cull<<<(unsigned)((pairs + LC_THREADS - 1) / LC_THREADS), LC_THREADS, 0, st>>>(d_job + j0, (int)c, d_seg, p, d_list, d_count);
            ULAUNCH("k_lc_cull");
            k_lc_render<<<(unsigned)walk, LC_THREADS, 0, st>>>(fbase, mbase, d_job + j0, d_seg, p, d_list, d_count, d_cnt, d_q);
            ULAUNCH("k_lc_render");
        }
        UHIP(hipMemcpyAsync(hcnt.data(), d_cnt, 3 * nsec * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(hq.data(), d_q, 2 * nsec * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        pool.release();
    }
    // (the host arrays above are read and written by the queued copies: they live until this wait)
    UHIP(hipStreamSynchronize(st));

    for (int i = 0; i < n_seg; i++) {
        lfdmi_lc &o = out[i];
        lfdmi_lc_section *row = sections + (size_t)i * max_sections_per_seg;
        memset(row, 0, (size_t)max_sections_per_seg * sizeof(lfdmi_lc_section));
        if (status[i] != LFDMI_LC_OK) {
            memset(&o, 0, sizeof(o));
            o.status = status[i];
            o.mean_rate = o.mean_rate_err = o.chi2 = o.peak_rate = o.length = o.flux = o.flux_err = kNaN;
            continue;
        }
        const LcSeg &g = hs[place[i]];
        const double sg = (double)sig[segs[i].frame];
        for (int j = 0; j < g.n_sec; j++) lc_section(j, hcnt.data() + 3 * ((size_t)g.base + j), hq.data() + 2 * ((size_t)g.base + j), g, q, sg, row[j]);
        lc_record(row, g.n_sec, o);
    }
    return 0;
}
