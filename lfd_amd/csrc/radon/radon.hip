// radon.hip -- host side of the faint-trail search (include/lfdmi.h: faint-trail search; kernels in k_radon.h).  Its own
// translation unit in its own directory, like sky/ and inject/: the detection kernels' code object does not change with it.
// The context's internals are reached through the ctx_* functions of lfdmi.hip; the handle owns every byte of device memory
// the search uses.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/lfdmi.h"
#include "k_radon.h"
#include "k_radon_lines.h"

int ctx_begin(lfdmi_ctx *ctx);
int ctx_fail(lfdmi_ctx *ctx, int code, const std::string &msg);
hipStream_t ctx_stream(lfdmi_ctx *ctx);
int ctx_device(lfdmi_ctx *ctx);

#define RHIP(expr)                                                                                      \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return ctx_fail(ctx, LFDMI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define RKCHK(name)                                                                                     \
    do {                                                                                                \
        hipError_t e_ = hipGetLastError();                                                              \
        if (e_ != hipSuccess) return ctx_fail(ctx, LFDMI_ERR_HIP, std::string("launch ") + name + ": " + hipGetErrorString(e_)); \
    } while (0)

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
    }
    p.part_stride = std::max(s->np[0], s->np[1]);
    auto run = [&]() -> int {
        const size_t F = (size_t)max_frames, px = (size_t)hb * wb, E = (size_t)p.frame_elems;
        RHIP(hipMalloc(&s->V, F * px * sizeof(float)));
        RHIP(hipMalloc(&s->M, F * px * sizeof(uint16_t)));
        for (int k = 0; k < 2; k++) {
            RHIP(hipMalloc(&s->S[k], F * E * sizeof(float)));
            RHIP(hipMalloc(&s->N[k], F * E * sizeof(uint16_t)));
        }
        RHIP(hipMalloc(&s->sigma, F * sizeof(float)));
        RHIP(hipMalloc(&s->part, F * 4 * (size_t)p.part_stride * sizeof(RadonPart)));
        RHIP(hipMalloc(&s->rec, F * sizeof(RadonRec)));
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
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    hipSetDevice(s->device);
    for (void *x : {(void *)s->V, (void *)s->M, (void *)s->S[0], (void *)s->S[1], (void *)s->N[0], (void *)s->N[1], (void *)s->sigma,
                    (void *)s->stage, (void *)s->part, (void *)s->rec, (void *)s->V2, (void *)s->M2, (void *)s->pre, (void *)s->cnt,
                    (void *)s->lnd, (void *)s->ext})
        if (x) hipFree(x);
    if (cur >= 0 && cur != s->device) hipSetDevice(cur);   // the caller's current device stays what it was
    delete s;
}

extern "C" int lfdmi_radon_dims(const lfdmi_radon *s, int32_t *p01, int32_t *p23, int64_t *bytes) {
    if (!s) return LFDMI_ERR_ARG;
    if (p01) *p01 = s->p.P[0];
    if (p23) *p23 = s->p.P[1];
    if (bytes) *bytes = s->bytes;
    return 0;
}

// definition step 6
static void radon_line(const RadonDev &p, int q, int y0, int sl, lfdmi_radon_result &o) {
    const int P = p.P[q >> 1], b = p.b;
    double px[2], py[2];
    for (int k = 0; k < 2; k++) {
        const int c = k ? P - 1 : 0, r = k ? y0 + sl : y0;
        int i, j;
        if (q == 0) { i = c; j = r; }
        else if (q == 1) { i = c; j = p.hb - 1 - r; }
        else if (q == 2) { i = r; j = c; }
        else { i = p.wb - 1 - r; j = c; }
        px[k] = (double)b * i + (double)(b - 1) / 2.0;
        py[k] = (double)b * j + (double)(b - 1) / 2.0;
    }
    double theta = atan2(-(px[1] - px[0]), py[1] - py[0]);
    const double pi = 3.141592653589793;
    if (theta < 0.0) theta += pi;
    if (theta >= pi) theta -= pi;
    o.x1 = px[0]; o.y1 = py[0]; o.x2 = px[1]; o.y2 = py[1];
    o.theta = theta;
    o.rho = px[0] * cos(theta) + py[0] * sin(theta);
}

// definition steps 3 - 6 of the nf frames in V, M (sigma in s->sigma): their records in s->rec
static int radon_transform(lfdmi_ctx *ctx, lfdmi_radon *s, const RadonDev &p, const float *V, const uint16_t *M, int nf, hipStream_t st) {
    {
        int gx = 0, gy = 0;
        for (int o = 0; o < 2; o++) {
            const int G = std::min(RAD_G, p.P[o] / 2);
            gx = std::max(gx, ceil_div(p.R[o] + G - 1, RAD_BAND));
            gy = std::max(gy, p.P[o] / G);
        }
        k_radon_first<<<dim3(gx, gy, nf * 4), RAD_THREADS, 0, st>>>(V, M, p, s->S[0], s->N[0]);
        RKCHK("k_radon_first");
    }
    for (int o = 0; o < 2; o++) {
        const int P = p.P[o], R = p.R[o];
        int cur = 0, lv = std::min(RAD_G, P / 2);
        for (; 2 * lv < P; lv *= 2, cur ^= 1) {   // (only reached with lv >= RAD_G)
            const dim3 grid(ceil_div(R + 2 * lv - 1, RAD_Y), P / (2 * RAD_TT), nf * 2);
            k_radon_level<4, false><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], s->S[cur ^ 1], s->N[cur ^ 1], p, o, lv, nullptr, nullptr);
            RKCHK("k_radon_level");
        }
        const int tt = std::min(RAD_TT, lv);
        const dim3 grid(ceil_div(R + P - 1, RAD_Y), P / (2 * tt), nf * 2);
        if (lv >= RAD_TT) k_radon_level<4, true><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], nullptr, nullptr, p, o, lv, s->sigma, s->part);
        else k_radon_level<1, true><<<grid, RAD_THREADS, 0, st>>>(s->S[cur], s->N[cur], nullptr, nullptr, p, o, lv, s->sigma, s->part);
        RKCHK("k_radon_level (last)");
    }
    k_radon_finish<<<nf, RAD_THREADS, 0, st>>>(s->part, p, s->np[0], s->np[1], s->rec);
    RKCHK("k_radon_finish");
    return 0;
}

extern "C" int lfdmi_radon_search(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                  lfdmi_radon_result *results) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!s || s->ctx != ctx) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search: the handle belongs to another context");
    if (n < 0 || (n > 0 && (!frames || !results))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if (dtype != LFDMI_F32 && dtype != LFDMI_F32_BE) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search takes LFDMI_F32 / LFDMI_F32_BE frames");
    if (loc != LFDMI_HOST && loc != LFDMI_DEVICE && loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad loc");
    std::vector<float> hsig(n, 0.025f);
    if (sigma)
        for (int i = 0; i < n; i++) {
            if (!std::isfinite(sigma[i]) || !(sigma[i] > 0)) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search: sigma must be positive");
            hsig[i] = sigma[i];
        }
    if (n == 0) return 0;
    RadonDev p = s->p;
    p.be = dtype == LFDMI_F32_BE;
    const size_t PX = (size_t)p.h * p.w, FB = PX * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE;
    const int CH = s->max_frames;
    if (!in_dev && !s->stage) {
        RHIP(hipMalloc(&s->stage, (size_t)CH * FB));
        s->bytes += (int64_t)((size_t)CH * FB);
    }
    hipStream_t st = ctx_stream(ctx);
    std::vector<RadonRec> hrec(n);
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int nf = std::min(CH, n - c0);
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * PX;
        if (!in_dev) {
            RHIP(hipMemcpyAsync(s->stage, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = (const uint32_t *)s->stage;
        }
        RHIP(hipMemcpyAsync(s->sigma, hsig.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        k_radon_prep<<<dim3(ceil_div(p.wb, RAD_THREADS), p.hb, nf), RAD_THREADS, 0, st>>>(src, p, s->V, s->M);
        RKCHK("k_radon_prep");
        rc = radon_transform(ctx, s, p, s->V, s->M, nf, st);
        if (rc) return rc;
        RHIP(hipMemcpyAsync(hrec.data() + c0, s->rec, (size_t)nf * sizeof(RadonRec), hipMemcpyDeviceToHost, st));
    }
    RHIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        lfdmi_radon_result &o = results[i];
        memset(&o, 0, sizeof(o));
        o.status = hrec[i].status;
        if (o.status != LFDMI_RADON_OK) continue;
        o.q = hrec[i].q; o.y0 = hrec[i].y0; o.s = hrec[i].s; o.n_pix = hrec[i].n_pix;
        o.sum = hrec[i].sum; o.snr = hrec[i].snr;
        o.found = o.snr >= s->par.threshold;
        radon_line(p, o.q, o.y0, o.s, o);
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

// the working point (c, r) of orientation q in pixels (step 6's mapping)
static void radon_point(const RadonDev &p, int q, int c, int r, double &x, double &y) {
    int i, j;
    if (q == 0) { i = c; j = r; }
    else if (q == 1) { i = c; j = p.hb - 1 - r; }
    else if (q == 2) { i = r; j = c; }
    else { i = p.wb - 1 - r; j = c; }
    x = (double)p.b * i + (double)(p.b - 1) / 2.0;
    y = (double)p.b * j + (double)(p.b - 1) / 2.0;
}

extern "C" int lfdmi_radon_search_lines(lfdmi_ctx *ctx, lfdmi_radon *s, const void *frames, int dtype, int n, int loc, const float *sigma,
                                        const lfdmi_radon_lines_params *lp, lfdmi_radon_line *lines, int32_t *n_lines) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!s || s->ctx != ctx) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search_lines: the handle belongs to another context");
    lfdmi_radon_lines_params lq;
    if (lp) lq = *lp; else lfdmi_default_radon_lines_params(&lq);
    if (lq.max_lines < 1 || lq.max_lines > LFDMI_RADON_MAX_LINES || lq.peel_halfwidth < 0 || lq.min_seg < 1 || lq.min_seg > s->par.min_len)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "radon lines params out of range (include/lfdmi.h: lfdmi_radon_lines_params)");
    if (n < 0 || (n > 0 && (!frames || !lines || !n_lines))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if (dtype != LFDMI_F32 && dtype != LFDMI_F32_BE) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search_lines takes LFDMI_F32 / LFDMI_F32_BE frames");
    if (loc != LFDMI_HOST && loc != LFDMI_DEVICE && loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad loc");
    std::vector<float> hsig(n, 0.025f);
    if (sigma)
        for (int i = 0; i < n; i++) {
            if (!std::isfinite(sigma[i]) || !(sigma[i] > 0)) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_radon_search_lines: sigma must be positive");
            hsig[i] = sigma[i];
        }
    if (n == 0) return 0;
    RadonDev p = s->p;
    p.be = dtype == LFDMI_F32_BE;
    const size_t PX = (size_t)p.h * p.w, FB = PX * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE;
    const int CH = s->max_frames, K = lq.max_lines;
    const int hw = (int)(((int64_t)lq.peel_halfwidth + p.b - 1) / p.b);
    const int pstride = std::max(p.hb, p.wb) + 1;
    if (!in_dev && !s->stage) {
        RHIP(hipMalloc(&s->stage, (size_t)CH * FB));
        s->bytes += (int64_t)((size_t)CH * FB);
    }
    if (!s->V2) {
        const size_t F = (size_t)CH, px = (size_t)p.hb * p.wb;
        RHIP(hipMalloc(&s->V2, F * px * sizeof(float)));
        RHIP(hipMalloc(&s->M2, F * px * sizeof(uint16_t)));
        RHIP(hipMalloc(&s->pre, F * pstride * sizeof(float)));
        RHIP(hipMalloc(&s->cnt, F * pstride * sizeof(int)));
        RHIP(hipMalloc(&s->lnd, F * sizeof(RadonLineDev)));
        RHIP(hipMalloc(&s->ext, F * sizeof(RadonExtDev)));
        s->bytes += (int64_t)(F * px * 6 + F * pstride * 8 + F * (sizeof(RadonLineDev) + sizeof(RadonExtDev)));
    }
    hipStream_t st = ctx_stream(ctx);
    memset(lines, 0, (size_t)n * K * sizeof(*lines));
    memset(n_lines, 0, (size_t)n * sizeof(*n_lines));
    float *Vs[2] = {s->V, s->V2};
    uint16_t *Ms[2] = {s->M, s->M2};
    std::vector<RadonRec> hrec(CH);
    // (round k's host buffers are read or written by copies that finish with round k + 1's wait: two of each alternate)
    std::vector<RadonLineDev> hl[2];
    std::vector<RadonExtDev> hx[2];
    std::vector<float> hs[2];
    std::vector<int> alive, found_frames[2];
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int nf = std::min(CH, n - c0);
        const uint32_t *src = (const uint32_t *)frames + (size_t)c0 * PX;
        if (!in_dev) {
            RHIP(hipMemcpyAsync(s->stage, (const char *)frames + (size_t)c0 * FB, (size_t)nf * FB, hipMemcpyHostToDevice, st));
            src = (const uint32_t *)s->stage;
        }
        RHIP(hipMemcpyAsync(s->sigma, hsig.data() + c0, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st));
        k_radon_prep<<<dim3(ceil_div(p.wb, RAD_THREADS), p.hb, nf), RAD_THREADS, 0, st>>>(src, p, s->V, s->M);
        RKCHK("k_radon_prep");
        alive.resize(nf);
        for (int a = 0; a < nf; a++) alive[a] = c0 + a;     // slot -> frame
        int cur = 0, pending = -1;                          // pending: the round whose segments are on their way to hx[round & 1]
        // the segments of round k's found lines, once their copy has been waited for
        auto segments = [&](int k) {
            const int b = k & 1;
            for (size_t e = 0; e < found_frames[b].size(); e++) {
                lfdmi_radon_line &o = lines[(size_t)found_frames[b][e] * K + k];
                const RadonExtDev &x = hx[b][e];
                const int P = p.P[o.q >> 1];
                o.c1 = x.c1; o.c2 = x.c2; o.seg_n_pix = x.n; o.seg_sum = x.sum; o.seg_snr = x.snr;
                radon_point(p, o.q, o.c1, o.y0 + radon_path(o.c1, o.s, P), o.ex1, o.ey1);
                radon_point(p, o.q, o.c2, o.y0 + radon_path(o.c2, o.s, P), o.ex2, o.ey2);
            }
        };
        for (int k = 0; k < K && !alive.empty(); k++) {
            const int na = (int)alive.size(), b = k & 1;
            rc = radon_transform(ctx, s, p, Vs[cur], Ms[cur], na, st);
            if (rc) return rc;
            RHIP(hipMemcpyAsync(hrec.data(), s->rec, (size_t)na * sizeof(RadonRec), hipMemcpyDeviceToHost, st));
            RHIP(hipStreamSynchronize(st));
            if (pending >= 0) { segments(pending); pending = -1; }
            hl[b].clear(); found_frames[b].clear(); hs[b].clear();
            for (int a = 0; a < na; a++) {
                lfdmi_radon_line &o = lines[(size_t)alive[a] * K + k];
                o.status = hrec[a].status;
                if (o.status != LFDMI_RADON_OK) continue;
                o.q = hrec[a].q; o.y0 = hrec[a].y0; o.s = hrec[a].s; o.n_pix = hrec[a].n_pix;
                o.sum = hrec[a].sum; o.snr = hrec[a].snr;
                o.found = o.snr >= s->par.threshold;
                lfdmi_radon_result r;
                radon_line(p, o.q, o.y0, o.s, r);
                o.x1 = r.x1; o.y1 = r.y1; o.x2 = r.x2; o.y2 = r.y2; o.rho = r.rho; o.theta = r.theta;
                if (!o.found) continue;
                n_lines[alive[a]] = k + 1;
                hl[b].push_back(RadonLineDev{a, o.q, o.y0, o.s});
                found_frames[b].push_back(alive[a]);
                hs[b].push_back(hsig[alive[a]]);
            }
            const int nl = (int)hl[b].size();
            if (!nl) break;
            hx[b].resize(nl);
            RHIP(hipMemcpyAsync(s->lnd, hl[b].data(), (size_t)nl * sizeof(RadonLineDev), hipMemcpyHostToDevice, st));
            k_radon_extent<<<nl, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, s->sigma, lq.min_seg, s->pre, s->cnt, pstride, s->ext);
            RKCHK("k_radon_extent");
            RHIP(hipMemcpyAsync(hx[b].data(), s->ext, (size_t)nl * sizeof(RadonExtDev), hipMemcpyDeviceToHost, st));
            pending = k;
            if (k + 1 == K) break;
            // the found frames go on: slot e of the other set is the frame of line e
            if (p.wb % 8 == 0) {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS * 8), ceil_div(p.hb, RADL_ROWS), nl);
                k_radon_peel<8><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, hw, Vs[cur ^ 1], Ms[cur ^ 1]);
            } else {
                const dim3 grid(ceil_div(p.wb, RAD_THREADS), ceil_div(p.hb, RADL_ROWS), nl);
                k_radon_peel<1><<<grid, RAD_THREADS, 0, st>>>(Vs[cur], Ms[cur], p, s->lnd, hw, Vs[cur ^ 1], Ms[cur ^ 1]);
            }
            RKCHK("k_radon_peel");
            RHIP(hipMemcpyAsync(s->sigma, hs[b].data(), (size_t)nl * sizeof(float), hipMemcpyHostToDevice, st));
            alive = found_frames[b];
            cur ^= 1;
        }
        if (pending >= 0) {
            RHIP(hipStreamSynchronize(st));
            segments(pending);
        }
    }
    return 0;
}
