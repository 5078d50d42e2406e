// radon.hip -- host side of the faint-trail search (include/lfdmi.h: faint-trail search; kernels in k_radon.h).  Its own
// translation unit in its own directory, like sky/ and inject/: the detection kernels' code object does not change with it.
// The context's internals are reached through unit.h; the handle owns every byte of device memory
// the search uses.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../unit.h"
#include "k_radon.h"
#include "k_radon_lines.h"
#include "k_radon_short.h"
#include "k_radon_wide.h"
#include "k_radon_null.h"

struct lfdmi_radon {
    lfdmi_ctx *ctx = nullptr;   // lfdmi_radon_search only: destroy does not touch the context (it may be gone by then)
    int device = 0, max_frames = 0;
    lfdmi_radon_params par;
    RadonDev p;
    int np[2] = {0, 0};         // partial records of the last level per orientation pair
    float *V = nullptr, *S[2] = {nullptr, nullptr}, *sigma = nullptr, *stage = nullptr;
    uint16_t *M = nullptr, *N[2] = {nullptr, nullptr};
    RadonPart *part = nullptr;
    RadonRec *rec = nullptr;
    // lfdmi_radon_search_lines only, allocated on its first call: the second V, M set the rounds alternate with, the found
    // lines of a round, their prefix arrays (max(Hb, Wb) + 1 values per line) and their segments
    float *V2 = nullptr, *pre = nullptr;
    uint16_t *M2 = nullptr;
    int *cnt = nullptr;
    RadonLineDev *lnd = nullptr;
    RadonExtDev *ext = nullptr;
    // lfdmi_radon_search_short only, allocated on its first call: the scoring levels' partial records (the layout for
    // min_strip = 64, which holds every other) and the frames' short records
    RadonShortPart *spart = nullptr;
    RadonShortRec *srec = nullptr;
    // lfdmi_radon_search_wide only, allocated on its first call: k_radon_wide's partial records (two per workgroup), the
    // frames' band records and the found bands' widths
    int nwp[2] = {0, 0}, wstride = 0;
    RadonWidePart *wpart = nullptr;
    RadonWideRec *wrec = nullptr;
    int *wid = nullptr;
    // lfdmi_radon_null only, allocated on its first call: the key and the frame of every slot; with peel records
    // (lfdmi_radon_null_scheme) a pass's line and width of every slot
    RadonNullSlot *nslot = nullptr;
    RadonLineDev *nline = nullptr;
    int *nwid = nullptr;
    int64_t bytes = 0;
};

static int pow2_at_least(int c) {
    int p = 1;
    while (p < c) p *= 2;
    return p;
}
static int ceil_div(int a, int b) { return (a + b - 1) / b; }

extern "C" void lfdmi_default_radon_params(lfdmi_radon_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->bin = 2; o->min_len = 256; o->clip = 0.125f; o->threshold = 8.0f;
}

extern "C" int lfdmi_radon_create(lfdmi_ctx *ctx, int h, int w, int max_frames, const lfdmi_radon_params *pp, lfdmi_radon **out) {
    if (!ctx) return LFDMI_ERR_ARG;
    if (!out) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    lfdmi_radon_params q;
    if (pp) q = *pp; else lfdmi_default_radon_params(&q);
    if ((q.bin != 1 && q.bin != 2 && q.bin != 4) || q.min_len < 1 || !std::isfinite(q.clip) || !(q.clip > 0) || std::isnan(q.threshold))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "radon params out of range (include/lfdmi.h: lfdmi_radon_params)");
    // (frames times orientations go in grid.z, at most 65535)
    if (h < 2 * q.bin || w < 2 * q.bin || max_frames < 1 || max_frames > 16383 || (double)h * w > 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_create: h, w at least 2 bin (h * w at most 1e9), max_frames 1 .. 16383");
    const int hb = ceil_div(h, q.bin), wb = ceil_div(w, q.bin);
    // a line of orientation q crosses all C columns of its working array, b x b pixels in each: N reaches max(Hb, Wb) b b
    if ((int64_t)std::max(hb, wb) * q.bin * q.bin > 65535)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_create: a line could count more than 65535 pixels, max(Hb, Wb) * bin * bin (the counts are 16-bit)");
    auto *s = new lfdmi_radon();
    s->ctx = ctx; s->device = ctx_device(ctx); s->max_frames = max_frames; s->par = q;
    RadonDev &p = s->p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.b = q.bin; p.hb = hb; p.wb = wb; p.min_len = q.min_len; p.clip = q.clip;
    p.R[0] = hb; p.C[0] = wb; p.R[1] = wb; p.C[1] = hb;
    long long off = 0;
    for (int k = 0; k < 4; k++) {
        const int o = k >> 1;
        if (!(k & 1)) p.P[o] = pow2_at_least(p.C[o]);
        p.off[k] = off;
        off += (((long long)p.R[o] + p.P[o] - 1) * p.P[o] + 63) / 64 * 64;   // (planes start on 256-byte boundaries)
    }
    p.frame_elems = off;
    for (int o = 0; o < 2; o++) {
        const int n = p.P[o] / 2, tt = std::min(RAD_TT, n);
        s->np[o] = ceil_div(p.R[o] + p.P[o] - 1, RAD_Y) * (p.P[o] / (2 * tt));
        s->nwp[o] = ceil_div(p.R[o] + p.P[o] - 1, RADW_Y) * (p.P[o] / std::min(RADW_S, p.P[o]));
    }
    s->wstride = std::max(s->nwp[0], s->nwp[1]);
    p.part_stride = std::max(s->np[0], s->np[1]);
    auto run = [&]() -> int {
        const size_t F = (size_t)max_frames, px = (size_t)hb * wb, E = (size_t)p.frame_elems;
        UHIP(hipMalloc(&s->V, F * px * sizeof(float)));
        UHIP(hipMalloc(&s->M, F * px * sizeof(uint16_t)));
        for (int k = 0; k < 2; k++) {
            UHIP(hipMalloc(&s->S[k], F * E * sizeof(float)));
            UHIP(hipMalloc(&s->N[k], F * E * sizeof(uint16_t)));
        }
        UHIP(hipMalloc(&s->sigma, F * sizeof(float)));
        UHIP(hipMalloc(&s->part, F * 4 * (size_t)p.part_stride * sizeof(RadonPart)));
        UHIP(hipMalloc(&s->rec, F * sizeof(RadonRec)));
        s->bytes = (int64_t)(F * px * 6 + F * E * 12 + F * 4 + F * 4 * (size_t)p.part_stride * sizeof(RadonPart) + F * sizeof(RadonRec));
        return 0;
    };
    rc = run();
    if (rc) { lfdmi_radon_destroy(s); return rc; }
    *out = s;
    return 0;
}

extern "C" void lfdmi_radon_destroy(lfdmi_radon *s) {
    if (!s) return;
    // lfdmi_radon_search returns after its stream has drained, so no work of the context still uses these buffers
    DeviceGuard on(s->device);   // the caller's current device stays what it was
    for (void *x : {(void *)s->V, (void *)s->M, (void *)s->S[0], (void *)s->S[1], (void *)s->N[0], (void *)s->N[1], (void *)s->sigma,
                    (void *)s->stage, (void *)s->part, (void *)s->rec, (void *)s->V2, (void *)s->M2, (void *)s->pre, (void *)s->cnt,
                    (void *)s->lnd, (void *)s->ext, (void *)s->spart, (void *)s->srec, (void *)s->wpart, (void *)s->wrec, (void *)s->wid,
                    (void *)s->nslot, (void *)s->nline, (void *)s->nwid})
        if (x) hipFree(x);
    delete s;
}

extern "C" int lfdmi_radon_dims(const lfdmi_radon *s, int32_t *p01, int32_t *p23, int64_t *bytes) {
    if (!s) return LFDMI_ERR_ARG;
    if (p01) *p01 = s->p.P[0];
    if (p23) *p23 = s->p.P[1];
    if (bytes) *bytes = s->bytes;
    return 0;
}

// the working point (c, r) of orientation q in pixels (step 6's mapping); r: a row, or the middle between two rows (a band's
// centre line, steps 15 and 16).  Every whole r is exact in a double, so a line's points do not depend on the route here
static void radon_point(const RadonDev &p, int q, int c, double r, double &x, double &y) {
    double i, j;
    if (q == 0) { i = c; j = r; }
    else if (q == 1) { i = c; j = (double)(p.hb - 1) - r; }
    else if (q == 2) { i = r; j = c; }
    else { i = (double)(p.wb - 1) - r; j = c; }
    x = (double)p.b * i + (double)(p.b - 1) / 2.0;
    y = (double)p.b * j + (double)(p.b - 1) / 2.0;
}
// the row offset of the centre line of a band `width` lines wide above its lowest line (0: a mode without widths)
static double radon_mid(int width) { return width > 1 ? (double)(width - 1) / 2.0 : 0.0; }

// definition step 6, `mid` rows above the line (o: an lfdmi_radon_result, or a record that begins with its fields)
template <class T> static void radon_line(const RadonDev &p, int q, int y0, int sl, double mid, T &o) {
    radon_point(p, q, 0, (double)y0 + mid, o.x1, o.y1);
    radon_point(p, q, p.P[q >> 1] - 1, (double)(y0 + sl) + mid, o.x2, o.y2);
    double theta = atan2(-(o.x2 - o.x1), o.y2 - o.y1);
    const double pi = 3.141592653589793;
    if (theta < 0.0) theta += pi;
    if (theta >= pi) theta -= pi;
    o.theta = theta;
    o.rho = o.x1 * cos(theta) + o.y1 * sin(theta);
}

// what every device record and every caller's record begin with (o zeroed before); false: no line, o stays as it is
template <class R, class T> static bool radon_fill_head(const R &r, float threshold, T &o) {
    o.status = r.status;
    if (o.status != LFDMI_RADON_OK) return false;
    o.q = r.q; o.y0 = r.y0; o.s = r.s; o.n_pix = r.n_pix;
    o.sum = r.sum; o.snr = r.snr;
    o.found = o.snr >= threshold;
    return true;
}

// the record of a frame's best line as the caller gets it (o zeroed before)
template <class T> static void radon_fill(const lfdmi_radon *s, const RadonDev &p, const RadonRec &r, T &o) {
    if (radon_fill_head(r, s->par.threshold, o)) radon_line(p, o.q, o.y0, o.s, 0.0, o);
}

// where the scoring levels of strip widths min_strip .. P/2 put their partial records (k_radon_short.h): the grids are
// radon_transform's
static RadonShortDev radon_short_layout(const RadonDev &p, int min_strip) {
    RadonShortDev d;
    memset(&d, 0, sizeof(d));
    for (int o = 0; o < 2; o++) {
        const int P = p.P[o], R = p.R[o];
        for (int lv = std::min(RAD_G, P / 2); 2 * lv < P; lv *= 2) {
            if (2 * lv < min_strip) continue;
            const int e = d.ne++;
            d.L[e] = 2 * lv; d.o[e] = o;
            d.cnt[e] = ceil_div(R + 2 * lv - 1, RAD_Y) * (P / (2 * RAD_TT));
            d.off[e] = d.total;
            d.total += 2LL * d.cnt[e];
        }
    }
    return d;
}

// definition steps 3 - 6 of the nf frames in V, M (sigma in s->sigma): their records in s->rec.  sd: the short search's mode --
// the levels it lists score what they store (step 10) and the frames' short records go to s->srec; `last` false then leaves
// the last level and s->rec out (a peel round of the short search has no use for them).  max_width > 0: the wide search's mode --
// the last level is stored by the non-scoring instance into the plane set that does not hold its input, k_radon_wide scores
// its bands (steps 13, 14), and k_radon_wide_finish writes the frames' band records to s->wrec and the plain ones to s->rec
static int radon_transform(lfdmi_ctx *ctx, lfdmi_radon *s, const RadonDev &p, const float *V, const uint16_t *M, int nf, hipStream_t st,
                           const RadonShortDev *sd = nullptr, bool last = true, int max_width = 0) {
    {
        int gx = 0, gy = 0;
        for (int o = 0; o < 2; o++) {
            const int G = std::min(RAD_G, p.P[o] / 2);
            gx = std::max(gx, ceil_div(p.R[o] + G - 1, RAD_BAND));
            gy = std::max(gy, p.P[o] / G);
        }
        k_radon_first<<<dim3(gx, gy, nf * 4), RAD_THREADS, 0, st>>>(V, M, p, s->S[0], s->N[0]);
        ULAUNCH("k_radon_first");
    }
    for (int o = 0; o < 2; o++) {
        const int P = p.P[o], R = p.R[o];
        int cur = 0, lv = std::min(RAD_G, P / 2);
        for (; 2 * lv < P; lv *= 2, cur ^= 1) {   // (only reached with lv >= RAD_G)
            const dim3 grid(ceil_div(R + 2 * lv - 1, RAD_Y), P / (2 * RAD_TT), nf * 2);
            int e = -1;
            for (int k = 0; sd && k < sd->ne; k++)
                if (sd->o[k] == o && sd->L[k] == 2 * lv) e = k;
            if (e >= 0)
                k_radon_level<4, false, true><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], s->S[cur ^ 1], s->N[cur ^ 1], p, o, lv, s->sigma,
                                                                            nullptr, s->spart, sd->off[e], sd->total);
            else
                k_radon_level<4, false><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], s->S[cur ^ 1], s->N[cur ^ 1], p, o, lv, nullptr, nullptr,
                                                                      nullptr, 0, 0);
            ULAUNCH("k_radon_level");
        }
        if (!last) continue;
        const int tt = std::min(RAD_TT, lv);
        const dim3 grid(ceil_div(R + P - 1, RAD_Y), P / (2 * tt), nf * 2);
        if (max_width > 0) {
            // (a level n writes rows -(2n-1) .. R-1 of width 2n: the last one fills its whole (R + P - 1) x P plane, [y][s])
            if (lv >= RAD_TT)
                k_radon_level<4, false><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], s->S[cur ^ 1], s->N[cur ^ 1], p, o, lv, nullptr, nullptr,
                                                                      nullptr, 0, 0);
            else
                k_radon_level<1, false><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], s->S[cur ^ 1], s->N[cur ^ 1], p, o, lv, nullptr, nullptr,
                                                                      nullptr, 0, 0);
            ULAUNCH("k_radon_level (last, stored)");
            const dim3 wgrid(ceil_div(R + P - 1, RADW_Y), P / std::min(RADW_S, P), nf * 2);
            k_radon_wide<<<wgrid, RAD_THREADS, 0, st>>>(s->S[cur ^ 1], s->N[cur ^ 1], p, o, max_width, s->sigma, s->wpart, s->wstride);
            ULAUNCH("k_radon_wide");
            continue;
        }
        if (lv >= RAD_TT)
            k_radon_level<4, true><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], nullptr, nullptr, p, o, lv, s->sigma, s->part, nullptr, 0, 0);
        else
            k_radon_level<1, true><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], nullptr, nullptr, p, o, lv, s->sigma, s->part, nullptr, 0, 0);
        ULAUNCH("k_radon_level (last)");
    }
    if (last && max_width > 0) {
        k_radon_wide_finish<<<nf, RAD_THREADS, 0, st>>>(s->wpart, s->wstride, s->nwp[0], s->nwp[1], s->wrec, s->rec);
        ULAUNCH("k_radon_wide_finish");
    } else if (last) {
        k_radon_finish<<<nf, RAD_THREADS, 0, st>>>(s->part, p, s->np[0], s->np[1], s->rec);
        ULAUNCH("k_radon_finish");
    }
    if (sd) {
        k_radon_short_finish<<<nf, RAD_THREADS, 0, st>>>(s->spart, p, *sd, s->srec);
        ULAUNCH("k_radon_short_finish");
    }
    return 0;
}

// every buffer a handle allocates after its creation goes through here: `count` values for *slot unless it has them.  Into a
// local first: a failed hipMalloc leaves *slot null and uncounted, so the next call tries again and destroy frees nothing twice
template <class T> static int radon_lazy(lfdmi_ctx *ctx, lfdmi_radon *s, T **slot, size_t count) {
    if (*slot) return 0;
    void *m = nullptr;
    UHIP(hipMalloc(&m, count * sizeof(T)));
    *slot = (T *)m;
    s->bytes += (int64_t)(count * sizeof(T));
    return 0;
}

// what the searches do alike: the checks of the handle and of the arguments, the frames' sigma on the host, the staging
// buffer of host frames, and the front of every chunk
struct LFD_HIDDEN RadonCall {
    lfdmi_ctx *ctx;
    lfdmi_radon *s;
    const char *fn;
    const void *frames = nullptr;
    RadonDev p;
    std::vector<float> hsig;
    size_t PX = 0, FB = 0;
    bool in_dev = false;
    int n = 0, CH = 0;
    hipStream_t st = nullptr;

    int begin() {
        if (!ctx) return LFDMI_ERR_ARG;
        int rc = ctx_begin(ctx);
        if (rc) return rc;
        if (!s || s->ctx != ctx) return ctx_fail(ctx, LFDMI_ERR_ARG, std::string(fn) + ": the handle belongs to another context");
        return 0;
    }
    // (outs: every output array of the call is there)
    int args(const void *fr, bool outs, int dtype, int nfr, int loc, const float *sigma) {
        int rc;
        if (nfr < 0 || (nfr > 0 && (!fr || !outs))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
        if ((rc = unit_dtype(ctx, fn, dtype)) || (rc = unit_loc(ctx, loc)) || (rc = unit_sigma(ctx, fn, sigma, nfr, &hsig))) return rc;
        frames = fr; n = nfr;
        p = s->p;
        p.be = dtype == LFDMI_F32_BE;
        PX = (size_t)p.h * p.w; FB = PX * sizeof(float);
        in_dev = loc == LFDMI_DEVICE;
        CH = s->max_frames;
        return 0;
    }
    // the staging buffer, allocated by the first call with host frames
    int stage() {
        int rc;
        if (!in_dev && (rc = radon_lazy(ctx, s, &s->stage, (size_t)CH * PX))) return rc;
        st = ctx_stream(ctx);
        return 0;
    }
    // frames c0 .. c0 + nf - 1 and their sigma on the device, steps 1 and 2 into s->V, s->M
    int chunk(int c0, int nf) {
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * PX;
        if (!in_dev) {
            UHIP(hipMemcpyAsync(s->stage, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = (const uint32_t *)s->stage;
        }
        UHIP(hipMemcpyAsync(s->sigma, hsig.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        k_radon_prep<<<dim3(ceil_div(p.wb, RAD_THREADS), p.hb, nf), RAD_THREADS, 0, st>>>(src, p, s->V, s->M);
        ULAUNCH("k_radon_prep");
        return 0;
    }
};

extern "C" int lfdmi_radon_search(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                  lfdmi_radon_result *results) {
    RadonCall c{ctx, s, "lfdmi_radon_search"};
    int rc;
    if ((rc = c.begin()) || (rc = c.args(frames, results, dtype, n, loc, sigma))) return rc;
    if (n == 0) return 0;
    if ((rc = c.stage())) return rc;
    const RadonDev &p = c.p;
    hipStream_t st = c.st;
    std::vector<RadonRec> hrec(n);
    for (int c0 = 0; c0 < n; c0 += c.CH) {
        const int nf = std::min(c.CH, n - c0);
        if ((rc = c.chunk(c0, nf)) || (rc = radon_transform(ctx, s, p, s->V, s->M, nf, st))) return rc;
        UHIP(hipMemcpyAsync(hrec.data() + c0, s->rec, (size_t)nf * sizeof(RadonRec), hipMemcpyDeviceToHost, st));
    }
    UHIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        memset(&results[i], 0, sizeof(results[i]));
        radon_fill(s, p, hrec[i], results[i]);
    }
    return 0;
}

extern "C" void lfdmi_default_radon_lines_params(lfdmi_radon_lines_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->max_lines = 4; o->peel_halfwidth = 8; o->min_seg = 64;
}

// definition step 7 on the host
static int radon_path(int c, int sl, int P) {
    int d = 0;
    for (int n = P >> 1; n > 0; n >>= 1, sl >>= 1)
        if (c & n) d += (sl + 1) >> 1;
    return d;
}

// what the rounds of every peeling search need, allocated by the first call of any (pstride: a line's prefix values)
static int radon_pstride(const RadonDev &p) { return std::max(p.hb, p.wb) + 1; }
static int radon_rounds_alloc(lfdmi_ctx *ctx, lfdmi_radon *s) {
    const size_t F = (size_t)s->max_frames, px = (size_t)s->p.hb * s->p.wb, ps = (size_t)radon_pstride(s->p);
    int rc;
    if ((rc = radon_lazy(ctx, s, &s->V2, F * px)) || (rc = radon_lazy(ctx, s, &s->M2, F * px)) || (rc = radon_lazy(ctx, s, &s->pre, F * ps)) ||
        (rc = radon_lazy(ctx, s, &s->cnt, F * ps)) || (rc = radon_lazy(ctx, s, &s->lnd, F)) || (rc = radon_lazy(ctx, s, &s->ext, F)))
        return rc;
    return 0;
}

// ---- the peeling searches ------------------------------------------------------------------------------------------------------------
// A Mode is what one of them adds to radon_rounds: Out, the caller's record; Rec, the device's, and where a round leaves them
// (rec()); q, its parameters (max_lines, peel_halfwidth and min_seg among them); transform(), radon_transform with the mode's
// arguments for round k; fill(), Rec -> Out (o zeroed before); width(), the found band's lines, 0 where lines have no width.
struct LFD_HIDDEN RadonLinesMode {
    typedef lfdmi_radon_line Out;
    typedef RadonRec Rec;
    lfdmi_radon *s;
    lfdmi_radon_lines_params q;
    const Rec *rec() const { return s->rec; }
    int transform(const RadonCall &c, const float *V, const uint16_t *M, int nf, int) const { return radon_transform(c.ctx, s, c.p, V, M, nf, c.st); }
    void fill(const RadonDev &p, const Rec &r, Out &o) const { radon_fill(s, p, r, o); }
    static int width(const Out &) { return 0; }
};

struct LFD_HIDDEN RadonShortMode {
    static constexpr int null_wfield = -1;      // (lfdmi_radon_null: a found record has a segment, and no width)
    float threshold() const { return q.short_threshold; }
    typedef lfdmi_radon_short Out;
    typedef RadonShortRec Rec;
    lfdmi_radon *s;
    lfdmi_radon_short_params q;
    RadonShortDev sd;
    const Rec *rec() const { return s->srec; }
    // round 0 runs the last level too: the plain search's record comes with it
    int transform(const RadonCall &c, const float *V, const uint16_t *M, int nf, int k) const {
        return radon_transform(c.ctx, s, c.p, V, M, nf, c.st, &sd, k == 0);
    }
    // the parent line's geometry by step 6
    void fill(const RadonDev &p, const Rec &r, Out &o) const {
        if (!radon_fill_head(r, q.short_threshold, o)) return;
        o.level = r.level; o.strip = r.strip; o.ys = r.ys; o.ss = r.ss;
        radon_line(p, o.q, o.y0, o.s, 0.0, o);
    }
    static int width(const Out &) { return 0; }
};

struct LFD_HIDDEN RadonWideMode {
    static constexpr int null_wfield = 7;       // (lfdmi_radon_null: a found record has a segment; RadonWideRec.k in ints, asserted below)
    float threshold() const { return q.wide_threshold; }
    typedef lfdmi_radon_wide Out;
    typedef RadonWideRec Rec;
    lfdmi_radon *s;
    lfdmi_radon_wide_params q;
    const Rec *rec() const { return s->wrec; }
    // every round's width-1 pass is step 5: round 0's is the plain search's record
    int transform(const RadonCall &c, const float *V, const uint16_t *M, int nf, int) const {
        return radon_transform(c.ctx, s, c.p, V, M, nf, c.st, nullptr, true, q.max_width);
    }
    // steps 14 and 15
    void fill(const RadonDev &p, const Rec &r, Out &o) const {
        if (!radon_fill_head(r, q.wide_threshold, o)) return;
        o.width = r.k;
        radon_line(p, o.q, o.y0, o.s, radon_mid(o.width), o);
        const long long run = p.P[o.q >> 1] - 1, rise = o.s;
        o.width_px = (double)(o.width * p.b) * ((double)run / sqrt((double)(run * run + rise * rise)));
    }
    static int width(const Out &o) { return o.width; }
};

// definition step 9's fields of a found record from its line's (width 0) or band's extent
template <class T> static void radon_fill_segment(const RadonDev &p, const RadonExtDev &x, int width, T &o) {
    const int P = p.P[o.q >> 1];
    const double mid = radon_mid(width);
    o.c1 = x.c1; o.c2 = x.c2; o.seg_n_pix = x.n; o.seg_sum = x.sum; o.seg_snr = x.snr;
    radon_point(p, o.q, o.c1, (double)(o.y0 + radon_path(o.c1, o.s, P)) + mid, o.ex1, o.ey1);
    radon_point(p, o.q, o.c2, (double)(o.y0 + radon_path(o.c2, o.s, P)) + mid, o.ex2, o.ey2);
}

// The chunks and the rounds of a peeling search, after the entry point's checks, c.stage() and the lazy allocations: lines
// [n * max_lines] and n_lines [n], and with `plain` the plain search's records, which round 0 leaves in s->rec.  A round queues
// the transform and the records' copy, waits for the stream (the call's one wait per round of a chunk, but for the last one of a
// pending segment copy), and then queues the found lines' extents, the copy of their segments, which the next round's wait
// covers, the peel into the other V, M set and the found frames' sigma.
template <class Mode>
static int radon_rounds(RadonCall &c, const Mode &m, typename Mode::Out *lines, int32_t *n_lines, lfdmi_radon_result *plain) {
    typedef typename Mode::Out Out;
    lfdmi_ctx *ctx = c.ctx;
    lfdmi_radon *s = c.s;
    const RadonDev &p = c.p;
    hipStream_t st = c.st;
    const int n = c.n, CH = c.CH, K = m.q.max_lines, pstride = radon_pstride(p);
    const int hw = (int)(((int64_t)m.q.peel_halfwidth + p.b - 1) / p.b);
    int rc;
    memset(lines, 0, (size_t)n * K * sizeof(*lines));
    memset(n_lines, 0, (size_t)n * sizeof(*n_lines));
    float *Vs[2] = {s->V, s->V2};
    uint16_t *Ms[2] = {s->M, s->M2};
    std::vector<typename Mode::Rec> hrec(CH);
    std::vector<RadonRec> hplain(plain ? n : 0);
    // (round k's host buffers are read or written by copies that finish with round k + 1's wait: two of each alternate)
    std::vector<RadonLineDev> hl[2];
    std::vector<RadonExtDev> hx[2];
    std::vector<float> hs[2];
    std::vector<int> alive, found_frames[2], hwid[2];
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int nf = std::min(CH, n - c0);
        if ((rc = c.chunk(c0, nf))) return rc;
        alive.resize(nf);
        for (int a = 0; a < nf; a++) alive[a] = c0 + a;     // slot -> frame
        int cur = 0, pending = -1;                          // pending: the round whose segments are on their way to hx[round & 1]
        // the segments of round k's found lines, once their copy has been waited for
        auto segments = [&](int k) {
            const int b = k & 1;
            for (size_t e = 0; e < found_frames[b].size(); e++) {
                Out &o = lines[(size_t)found_frames[b][e] * K + k];
                radon_fill_segment(p, hx[b][e], m.width(o), o);
            }
        };
        for (int k = 0; k < K && !alive.empty(); k++) {
            const int na = (int)alive.size(), b = k & 1;
            if ((rc = m.transform(c, Vs[cur], Ms[cur], na, k))) return rc;
            UHIP(hipMemcpyAsync(hrec.data(), m.rec(), (size_t)na * sizeof(hrec[0]), hipMemcpyDeviceToHost, st));
            if (k == 0 && plain) UHIP(hipMemcpyAsync(hplain.data() + c0, s->rec, (size_t)na * sizeof(RadonRec), hipMemcpyDeviceToHost, st));
            UHIP(hipStreamSynchronize(st));
            if (pending >= 0) { segments(pending); pending = -1; }
            hl[b].clear(); found_frames[b].clear(); hs[b].clear(); hwid[b].clear();
            for (int a = 0; a < na; a++) {
                Out &o = lines[(size_t)alive[a] * K + k];
                m.fill(p, hrec[a], o);
                if (!o.found) continue;
                n_lines[alive[a]] = k + 1;
                hl[b].push_back(RadonLineDev{a, o.q, o.y0, o.s});
                if (m.width(o)) hwid[b].push_back(m.width(o));
                found_frames[b].push_back(alive[a]);
                hs[b].push_back(c.hsig[alive[a]]);
            }
            const int nl = (int)hl[b].size();
            if (!nl) break;
            hx[b].resize(nl);
            // (a mode with widths has one for every found line; the others pass none and upload nothing)
            const int *wid = (int)hwid[b].size() == nl ? s->wid : nullptr;
            UHIP(hipMemcpyAsync(s->lnd, hl[b].data(), (size_t)nl * sizeof(RadonLineDev), hipMemcpyHostToDevice, st));
            if (wid) UHIP(hipMemcpyAsync(s->wid, hwid[b].data(), (size_t)nl * sizeof(int), hipMemcpyHostToDevice, st));
            k_radon_extent<<<nl, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, s->sigma, m.q.min_seg, s->pre, s->cnt, pstride, s->ext, wid);
            ULAUNCH("k_radon_extent");
            UHIP(hipMemcpyAsync(hx[b].data(), s->ext, (size_t)nl * sizeof(RadonExtDev), hipMemcpyDeviceToHost, st));
            pending = k;
            if (k + 1 == K) break;
            // the found frames go on: slot e of the other set is the frame of line e
            if (p.wb % 8 == 0) {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS * 8), ceil_div(p.hb, RADL_ROWS), nl);
                k_radon_peel<8><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, hw, Vs[cur ^ 1], Ms[cur ^ 1], wid);
            } else {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS), ceil_div(p.hb, RADL_ROWS), nl);
                k_radon_peel<1><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, hw, Vs[cur ^ 1], Ms[cur ^ 1], wid);
            }
            ULAUNCH("k_radon_peel");
            UHIP(hipMemcpyAsync(s->sigma, hs[b].data(), (size_t)nl * sizeof(float), hipMemcpyHostToDevice, st));
            alive = found_frames[b];
            cur ^= 1;
        }
        if (pending >= 0) {
            UHIP(hipStreamSynchronize(st));
            segments(pending);
        }
    }
    if (plain)
        for (int i = 0; i < n; i++) {
            memset(&plain[i], 0, sizeof(plain[i]));
            radon_fill(s, p, hplain[i], plain[i]);
        }
    return 0;
}

// the rules of lfdmi_radon_short_params and lfdmi_radon_wide_params for handle s
static int radon_short_check(lfdmi_ctx *ctx, const lfdmi_radon *s, const lfdmi_radon_short_params &sq) {
    const int bb = s->p.b * s->p.b;
    if (sq.min_strip < 64 || (sq.min_strip & (sq.min_strip - 1)) || sq.max_lines < 1 || sq.max_lines > LFDMI_RADON_MAX_LINES ||
        sq.peel_halfwidth < 0 || sq.min_seg < 1 || (int64_t)sq.min_seg > (int64_t)sq.min_strip * bb / 2 ||
        !std::isfinite(sq.short_threshold) || !(sq.short_threshold > 0))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "radon short params out of range (include/lfdmi.h: lfdmi_radon_short_params)");
    return 0;
}
static int radon_lines_check(lfdmi_ctx *ctx, const lfdmi_radon *s, const lfdmi_radon_lines_params &lq) {
    if (lq.max_lines < 1 || lq.max_lines > LFDMI_RADON_MAX_LINES || lq.peel_halfwidth < 0 || lq.min_seg < 1 || lq.min_seg > s->par.min_len)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "radon lines params out of range (include/lfdmi.h: lfdmi_radon_lines_params)");
    return 0;
}
static int radon_wide_check(lfdmi_ctx *ctx, const lfdmi_radon *s, const lfdmi_radon_wide_params &wq) {
    if (wq.max_width < 1 || wq.max_width > LFDMI_RADON_MAX_WIDTH || (wq.max_width & (wq.max_width - 1)) || wq.max_lines < 1 ||
        wq.max_lines > LFDMI_RADON_MAX_LINES || wq.peel_halfwidth < 0 || wq.min_seg < 1 || wq.min_seg > s->par.min_len ||
        !std::isfinite(wq.wide_threshold) || !(wq.wide_threshold > 0))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "radon wide params out of range (include/lfdmi.h: lfdmi_radon_wide_params)");
    return 0;
}

// what the short and the wide search allocate on their first call
static int radon_short_alloc(lfdmi_ctx *ctx, lfdmi_radon *s) {
    // (the partial records in the layout for min_strip = 64, which holds every other)
    const size_t F = (size_t)s->max_frames, total = (size_t)std::max(1LL, radon_short_layout(s->p, 64).total);
    int rc;
    if ((rc = radon_rounds_alloc(ctx, s)) || (rc = radon_lazy(ctx, s, &s->spart, F * total)) || (rc = radon_lazy(ctx, s, &s->srec, F))) return rc;
    return 0;
}
static int radon_wide_alloc(lfdmi_ctx *ctx, lfdmi_radon *s) {
    const size_t F = (size_t)s->max_frames;
    int rc;
    if ((rc = radon_rounds_alloc(ctx, s)) || (rc = radon_lazy(ctx, s, &s->wpart, F * 4 * s->wstride * 2)) ||
        (rc = radon_lazy(ctx, s, &s->wrec, F)) || (rc = radon_lazy(ctx, s, &s->wid, F)))
        return rc;
    return 0;
}

extern "C" int lfdmi_radon_search_lines(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                        const lfdmi_radon_lines_params *lp, lfdmi_radon_line *lines, int32_t *n_lines) {
    RadonCall c{ctx, s, "lfdmi_radon_search_lines"};
    int rc = c.begin();
    if (rc) return rc;
    RadonLinesMode m{s};
    if (lp) m.q = *lp; else lfdmi_default_radon_lines_params(&m.q);
    if ((rc = radon_lines_check(ctx, s, m.q))) return rc;
    if ((rc = c.args(frames, lines && n_lines, dtype, n, loc, sigma))) return rc;
    if (n == 0) return 0;
    if ((rc = c.stage()) || (rc = radon_rounds_alloc(ctx, s))) return rc;
    return radon_rounds(c, m, lines, n_lines, nullptr);
}

extern "C" void lfdmi_default_radon_short_params(lfdmi_radon_short_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->min_strip = 64; o->max_lines = 4; o->peel_halfwidth = 8; o->min_seg = 32; o->short_threshold = 8.5f;
}

extern "C" int lfdmi_radon_search_short(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                        const lfdmi_radon_short_params *sp, lfdmi_radon_short *lines, int32_t *n_lines,
                                        lfdmi_radon_result *plain) {
    RadonCall c{ctx, s, "lfdmi_radon_search_short"};
    int rc = c.begin();
    if (rc) return rc;
    RadonShortMode m{s};
    lfdmi_radon_short_params &sq = m.q;
    if (sp) sq = *sp; else lfdmi_default_radon_short_params(&sq);
    if ((rc = radon_short_check(ctx, s, sq))) return rc;
    if ((rc = c.args(frames, lines && n_lines, dtype, n, loc, sigma))) return rc;
    if (n == 0) return 0;
    if ((rc = c.stage()) || (rc = radon_short_alloc(ctx, s))) return rc;
    m.sd = radon_short_layout(c.p, sq.min_strip);
    return radon_rounds(c, m, lines, n_lines, plain);
}

extern "C" void lfdmi_default_radon_wide_params(lfdmi_radon_wide_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->max_width = 8; o->max_lines = 4; o->peel_halfwidth = 8; o->min_seg = 64; o->wide_threshold = 8.0f;
}

extern "C" int lfdmi_radon_search_wide(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                       const lfdmi_radon_wide_params *wp, lfdmi_radon_wide *lines, int32_t *n_lines,
                                       lfdmi_radon_result *plain) {
    RadonCall c{ctx, s, "lfdmi_radon_search_wide"};
    int rc = c.begin();
    if (rc) return rc;
    RadonWideMode m{s};
    lfdmi_radon_wide_params &wq = m.q;
    if (wp) wq = *wp; else lfdmi_default_radon_wide_params(&wq);
    if ((rc = radon_wide_check(ctx, s, wq))) return rc;
    if ((rc = c.args(frames, lines && n_lines, dtype, n, loc, sigma))) return rc;
    if (n == 0) return 0;
    if ((rc = c.stage()) || (rc = radon_wide_alloc(ctx, s))) return rc;
    return radon_rounds(c, m, lines, n_lines, plain);
}

// ---- null peaks (definition steps 17 - 22) ----------------------------------------------------------------------------------------------
// The plain search as a Mode: what lfdmi_radon_null needs of one
struct LFD_HIDDEN RadonPlainMode {
    static constexpr int null_wfield = -2;      // (no segment: lfdmi_radon_result has none)
    typedef lfdmi_radon_result Out;
    typedef RadonRec Rec;
    lfdmi_radon *s;
    const Rec *rec() const { return s->rec; }
    int transform(const RadonCall &c, const float *V, const uint16_t *M, int nf, int) const { return radon_transform(c.ctx, s, c.p, V, M, nf, c.st); }
    void fill(const RadonDev &p, const Rec &r, Out &o) const { radon_fill(s, p, r, o); }
};

// k_radon_null_lines reads every kind's record as ints: the fields it names, where it expects them
#define RADON_NULL_PREFIX(T)                                                                                                      \
    static_assert(offsetof(T, status) == 0 && offsetof(T, q) == 4 && offsetof(T, y0) == 8 && offsetof(T, s) == 12 &&               \
                      offsetof(T, n_pix) == 16 && offsetof(T, sum) == 20 && offsetof(T, snr) == 4 * RADN_SNR,                       \
                  #T ": k_radon_null_lines expects status, q, y0, s, n_pix, sum, snr first")
RADON_NULL_PREFIX(RadonRec);
RADON_NULL_PREFIX(RadonShortRec);
RADON_NULL_PREFIX(RadonWideRec);
static_assert(offsetof(RadonWideRec, k) == 4 * RadonWideMode::null_wfield, "RadonWideMode::null_wfield is RadonWideRec.k");

static uint64_t radon_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The chunks of lfdmi_radon_null and lfdmi_radon_null_scheme after the entry point's checks, c.stage() and the lazy allocations.
// Slot g = f K + r is realisation r of frame f; a chunk is max_frames consecutive slots, so it reads at most that many frames
// (which fit the staging buffer) and a frame's realisations may continue in the next chunk, which then uploads the frame again.
// scheme: how the slots' V', M' are made (step 21).  peel, n_peel (step 22; checked by the caller): pass j blots record j of
// every slot's frame from one V, M set into the other with k_radon_peel, slot a to slot a; a slot whose frame has no line in
// that place (width 0) gets a line whose band lies outside every frame, so it is copied as it is.  A chunk runs as many passes
// as its longest list.  Everything is queued; the host buffers live until the one wait at the end.
static_assert(LFDMI_RADON_NULL_SIGNFLIP == RADN_SIGNFLIP && LFDMI_RADON_NULL_ROWSHIFT == RADN_ROWSHIFT &&
                  LFDMI_RADON_NULL_COLSHIFT == RADN_COLSHIFT, "k_radon_null.h names the schemes by the header's values");
#define RADN_HW_MAX (1 << 20)     // a half-width beyond any frame (a working row is below 2^18 in magnitude) blots what this one does
#define RADN_NO_LINE (1 << 28)    // y0 of the line that blots nothing: farther from every cell than RADN_HW_MAX + LFDMI_RADON_MAX_WIDTH
template <class Mode>
static int radon_null(RadonCall &c, const Mode &m, const uint64_t *seeds, int K, typename Mode::Out *records,
                      int scheme = LFDMI_RADON_NULL_SCRAMBLE, const lfdmi_radon_peel *peel = nullptr, int n_peel = 0) {
    typedef typename Mode::Rec Rec;
    static_assert(sizeof(Rec) % sizeof(int) == 0, "k_radon_null_lines reads records as ints");
    constexpr bool SEG = Mode::null_wfield >= -1;
    lfdmi_ctx *ctx = c.ctx;
    lfdmi_radon *s = c.s;
    const RadonDev &p = c.p;
    hipStream_t st = c.st;
    const int64_t total = (int64_t)c.n * K;
    const int CH = c.CH;
    int rc;
    if ((rc = radon_lazy(ctx, s, &s->nslot, (size_t)CH))) return rc;
    // the frames' peel passes: a frame's records of width >= 1, in their order
    int passes = 0;
    std::vector<int> npeel(peel ? c.n : 0, 0);
    for (int f = 0; f < (int)npeel.size(); f++) {
        for (int e = 0; e < n_peel; e++) npeel[f] += peel[(size_t)f * n_peel + e].width >= 1;
        passes = std::max(passes, npeel[f]);
    }
    if (passes) {
        const size_t F = (size_t)CH, px = (size_t)p.hb * p.wb;
        if ((rc = radon_lazy(ctx, s, &s->V2, F * px)) || (rc = radon_lazy(ctx, s, &s->M2, F * px)) || (rc = radon_lazy(ctx, s, &s->nline, F)) ||
            (rc = radon_lazy(ctx, s, &s->nwid, F)))
            return rc;
    }
    const int hw = (int)std::min<int64_t>(((int64_t)m.q.peel_halfwidth + p.b - 1) / p.b, RADN_HW_MAX);
    std::vector<RadonNullSlot> hslot((size_t)total);
    std::vector<float> hsg((size_t)total);
    std::vector<Rec> hrec((size_t)total);
    std::vector<RadonExtDev> hext(SEG ? (size_t)total : 0);
    std::vector<RadonLineDev> hline((size_t)total * passes);     // [chunk][pass][slot], filled as the chunks are queued
    std::vector<int> hwid((size_t)total * passes);
    size_t lused = 0;
    float *Vs[2] = {s->V, s->V2};
    uint16_t *Ms[2] = {s->M, s->M2};
    for (int64_t g0 = 0; g0 < total; g0 += CH) {
        const int ns = (int)std::min<int64_t>(CH, total - g0), f0 = (int)(g0 / K), nfr = (int)((g0 + ns - 1) / K) - f0 + 1;
        for (int a = 0; a < ns; a++) {
            const int f = (int)((g0 + a) / K), r = (int)((g0 + a) % K);
            const uint64_t k = radon_splitmix64((seeds ? seeds[f] : (uint64_t)f) + 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1));
            hslot[g0 + a] = RadonNullSlot{(uint32_t)k, (uint32_t)(k >> 32), f - f0, 0};
            hsg[g0 + a] = c.hsig[f];
        }
        const uint32_t *src = (const uint32_t *)c.frames + (size_t)f0 * c.PX;
        if (!c.in_dev) {
            UHIP(hipMemcpyAsync(s->stage, (const char *)c.frames + (size_t)f0 * c.FB, (size_t)nfr * c.FB, hipMemcpyHostToDevice, st));
            src = (const uint32_t *)s->stage;
        }
        UHIP(hipMemcpyAsync(s->sigma, hsg.data() + g0, (size_t)ns * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(s->nslot, hslot.data() + g0, (size_t)ns * sizeof(RadonNullSlot), hipMemcpyHostToDevice, st));
        const dim3 pgrid(ceil_div(p.wb, RAD_THREADS), p.hb, ns);
        if (scheme == LFDMI_RADON_NULL_SIGNFLIP)
            k_radon_prep_scheme<RADN_SIGNFLIP><<<pgrid, RAD_THREADS, 0, st>>>(src, p, s->nslot, s->V, s->M);
        else if (scheme == LFDMI_RADON_NULL_ROWSHIFT)
            k_radon_prep_scheme<RADN_ROWSHIFT><<<pgrid, RAD_THREADS, 0, st>>>(src, p, s->nslot, s->V, s->M);
        else if (scheme == LFDMI_RADON_NULL_COLSHIFT)
            k_radon_prep_scheme<RADN_COLSHIFT><<<pgrid, RAD_THREADS, 0, st>>>(src, p, s->nslot, s->V, s->M);
        else
            k_radon_prep_null<<<pgrid, RAD_THREADS, 0, st>>>(src, p, s->nslot, s->V, s->M);
        ULAUNCH("k_radon_prep_null");
        int cur = 0, cpass = 0;
        for (int f = f0; f < f0 + nfr && passes; f++) cpass = std::max(cpass, npeel[f]);
        for (int j = 0; j < cpass; j++, cur ^= 1) {
            RadonLineDev *hl = hline.data() + lused;
            int *hwd = hwid.data() + lused;
            lused += (size_t)ns;
            for (int a = 0; a < ns; a++) {
                const int f = (int)((g0 + a) / K);
                hl[a] = RadonLineDev{a, 0, RADN_NO_LINE, 0};
                hwd[a] = 1;
                for (int e = 0, seen = 0; e < n_peel; e++) {
                    const lfdmi_radon_peel &r = peel[(size_t)f * n_peel + e];
                    if (r.width >= 1 && seen++ == j) {
                        hl[a] = RadonLineDev{a, r.q, r.y0, r.s};
                        hwd[a] = r.width;
                        break;
                    }
                }
            }
            UHIP(hipMemcpyAsync(s->nline, hl, (size_t)ns * sizeof(RadonLineDev), hipMemcpyHostToDevice, st));
            UHIP(hipMemcpyAsync(s->nwid, hwd, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
            if (p.wb % 8 == 0) {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS * 8), ceil_div(p.hb, RADL_ROWS), ns);
                k_radon_peel<8><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->nline, hw, Vs[cur ^ 1], Ms[cur ^ 1], s->nwid);
            } else {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS), ceil_div(p.hb, RADL_ROWS), ns);
                k_radon_peel<1><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->nline, hw, Vs[cur ^ 1], Ms[cur ^ 1], s->nwid);
            }
            ULAUNCH("k_radon_peel");
        }
        if ((rc = m.transform(c, Vs[cur], Ms[cur], ns, 0))) return rc;
        UHIP(hipMemcpyAsync(hrec.data() + g0, m.rec(), (size_t)ns * sizeof(Rec), hipMemcpyDeviceToHost, st));
        if constexpr (SEG) {
            int *wid = Mode::null_wfield >= 0 ? s->wid : nullptr;
            k_radon_null_lines<<<ceil_div(ns, RAD_THREADS), RAD_THREADS, 0, st>>>((const int *)m.rec(), (int)(sizeof(Rec) / sizeof(int)),
                                                                                  Mode::null_wfield, m.threshold(), ns, s->lnd, wid);
            ULAUNCH("k_radon_null_lines");
            k_radon_extent<<<ns, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, s->sigma, m.q.min_seg, s->pre, s->cnt, radon_pstride(p), s->ext, wid);
            ULAUNCH("k_radon_extent");
            UHIP(hipMemcpyAsync(hext.data() + g0, s->ext, (size_t)ns * sizeof(RadonExtDev), hipMemcpyDeviceToHost, st));
        }
    }
    UHIP(hipStreamSynchronize(st));
    for (int64_t g = 0; g < total; g++) {
        typename Mode::Out &o = records[g];
        memset(&o, 0, sizeof(o));
        m.fill(p, hrec[g], o);
        if constexpr (SEG)
            if (o.found) radon_fill_segment(p, hext[g], Mode::width(o), o);
    }
    return 0;
}

// step 22's rules for the peel records of a call on handle s
static int radon_peel_check(lfdmi_ctx *ctx, const lfdmi_radon *s, int scheme, const lfdmi_radon_peel *peel, int n, int n_peel) {
    if (scheme < LFDMI_RADON_NULL_SCRAMBLE || scheme > LFDMI_RADON_NULL_COLSHIFT || n_peel < 0 || n_peel > LFDMI_RADON_MAX_LINES ||
        (n_peel > 0 && (!peel || scheme != LFDMI_RADON_NULL_SIGNFLIP)))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_null_scheme: scheme LFDMI_RADON_NULL_SCRAMBLE .. COLSHIFT, n_peel 0 .. "
                                            "LFDMI_RADON_MAX_LINES, and peel records with LFDMI_RADON_NULL_SIGNFLIP only");
    for (int64_t e = 0; e < (int64_t)std::max(n, 0) * n_peel; e++) {
        const lfdmi_radon_peel &r = peel[e];
        if (r.width == 0) continue;
        if (r.width < 1 || r.width > LFDMI_RADON_MAX_WIDTH || (r.width & (r.width - 1)) || r.q < 0 || r.q > 3)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_null_scheme: a peel record's width is 0 or a power of two up to 16, its q 0 .. 3");
        const int P = s->p.P[r.q >> 1], R = s->p.R[r.q >> 1];
        if (r.s < 0 || r.s > P - 1 || r.y0 < -(P - 1) || r.y0 > R - 1)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_null_scheme: a peel record's s is 0 .. P-1, its y0 -(P-1) .. R-1");
    }
    return 0;
}

// the plain search as the LINES kind of lfdmi_radon_null_scheme: its peel_halfwidth comes from an lfdmi_radon_lines_params
struct LFD_HIDDEN RadonPlainPeelMode : RadonPlainMode {
    lfdmi_radon_lines_params q;
};

// what both entry points do; `scheme_call`: lfdmi_radon_null_scheme, whose LINES kind takes an lfdmi_radon_lines_params
static int radon_null_call(lfdmi_ctx *ctx, lfdmi_radon *s, const char *fn, bool scheme_call, const void *frames, int dtype, int n, int loc,
                           const float *sigma, const uint64_t *seeds, int K, int kind, const void *kind_params, int scheme,
                           const lfdmi_radon_peel *peel, int n_peel, void *records) {
    RadonCall c{ctx, s, fn};
    int rc = c.begin();
    if (rc) return rc;
    if (K < 1 || K > LFDMI_RADON_NULL_MAX || kind < LFDMI_RADON_NULL_LINES || kind > LFDMI_RADON_NULL_WIDE ||
        (kind == LFDMI_RADON_NULL_LINES && kind_params && !scheme_call))
        return ctx_fail(ctx, LFDMI_ERR_ARG, std::string(fn) + ": K 1 .. LFDMI_RADON_NULL_MAX, kind LFDMI_RADON_NULL_*, and no kind_params for LINES");
    if ((uint64_t)s->p.h * (uint64_t)s->p.w >= (1ull << 32))     // (lfdmi_radon_create holds H W to 1e9)
        return ctx_fail(ctx, LFDMI_ERR_ARG, std::string(fn) + ": H * W must be below 2^32");
    if ((rc = radon_peel_check(ctx, s, scheme, peel, n, n_peel))) return rc;
    if (kind == LFDMI_RADON_NULL_SHORT) {
        RadonShortMode m{s};
        if (kind_params) m.q = *(const lfdmi_radon_short_params *)kind_params; else lfdmi_default_radon_short_params(&m.q);
        if ((rc = radon_short_check(ctx, s, m.q)) || (rc = c.args(frames, records, dtype, n, loc, sigma))) return rc;
        if (n == 0) return 0;
        if ((rc = c.stage()) || (rc = radon_short_alloc(ctx, s))) return rc;
        m.sd = radon_short_layout(c.p, m.q.min_strip);
        return radon_null(c, m, seeds, K, (lfdmi_radon_short *)records, scheme, peel, n_peel);
    }
    if (kind == LFDMI_RADON_NULL_WIDE) {
        RadonWideMode m{s};
        if (kind_params) m.q = *(const lfdmi_radon_wide_params *)kind_params; else lfdmi_default_radon_wide_params(&m.q);
        if ((rc = radon_wide_check(ctx, s, m.q)) || (rc = c.args(frames, records, dtype, n, loc, sigma))) return rc;
        if (n == 0) return 0;
        if ((rc = c.stage()) || (rc = radon_wide_alloc(ctx, s))) return rc;
        return radon_null(c, m, seeds, K, (lfdmi_radon_wide *)records, scheme, peel, n_peel);
    }
    RadonPlainPeelMode m{{s}};
    // (without parameters only the default peel_halfwidth is used: a handle whose min_len is below the default min_seg is served)
    lfdmi_default_radon_lines_params(&m.q);
    if (kind_params) {
        m.q = *(const lfdmi_radon_lines_params *)kind_params;
        if ((rc = radon_lines_check(ctx, s, m.q))) return rc;
    }
    if ((rc = c.args(frames, records, dtype, n, loc, sigma))) return rc;
    if (n == 0) return 0;
    if ((rc = c.stage())) return rc;
    return radon_null(c, m, seeds, K, (lfdmi_radon_result *)records, scheme, peel, n_peel);
}

extern "C" int lfdmi_radon_null(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                const uint64_t *seeds, int K, int kind, const void *kind_params, void *records) {
    return radon_null_call(ctx, s, "lfdmi_radon_null", false, frames, dtype, n, loc, sigma, seeds, K, kind, kind_params,
                           LFDMI_RADON_NULL_SCRAMBLE, nullptr, 0, records);
}

extern "C" int lfdmi_radon_null_scheme(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                       const uint64_t *seeds, int K, int kind, const void *kind_params, int scheme,
                                       const lfdmi_radon_peel *peel, int n_peel, void *records) {
    return radon_null_call(ctx, s, "lfdmi_radon_null_scheme", true, frames, dtype, n, loc, sigma, seeds, K, kind, kind_params, scheme, peel,
                           n_peel, records);
}
