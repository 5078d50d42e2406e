// defocus.hip -- host side of the defocus bank and fit (include/lfdmi.h: defocus fit; kernels in k_defocus.h).  Its own translation
// unit: the detection kernels' code object does not change with it.  The context's internals are reached through unit.h.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "k_defocus.h"
#include "unit.h"

struct lfdmi_defocus_bank {
    lfdmi_ctx *ctx = nullptr;  // read and fit only: destroy does not touch the context (it may be gone by then)
    int device = 0;
    DefDev p;
    double delta_chi2 = 0;
    std::vector<double> heights, radii, seeings;
    std::vector<int> gvalid;   // per (seeing, height) group: any valid model
    std::vector<double> dfwhm; // per OD model ((n_h + 1) n_r)
    std::vector<double> gridv_h; // n_models x {ofwhm, depth}, the device's gridv
    double *d_grid = nullptr;  // heights, radii, seeings back to back
    float *cols = nullptr;     // ncol x nbp
    double *samp = nullptr;    // n_models x nq
    double *gridv = nullptr;   // n_models x {ofwhm, depth}
    int *valid = nullptr, *d_gvalid = nullptr;
    size_t bytes = 0;
};

// the fit's workspace, one per context (released with it)
struct DefocusWs {
    float *V = nullptr, *prof = nullptr;
    double *noise = nullptr, *res = nullptr, *cbh = nullptr;
    int *slice = nullptr;
    unsigned *gmax = nullptr;
    size_t cap_rows = 0, cap_groups = 0, cap_nbp = 0, cap_h = 0;
};
static void ws_free(DefocusWs *w) {
    for (void *q : {(void *)w->V, (void *)w->prof, (void *)w->noise, (void *)w->res, (void *)w->cbh, (void *)w->slice, (void *)w->gmax})
        if (q) hipFree(q);
    *w = DefocusWs();
}
static void ws_release(lfdmi_ctx *ctx) {
    void **slot = ctx_defocus(ctx, nullptr);
    if (*slot) {
        DeviceGuard on(ctx_device(ctx));
        hipStreamSynchronize(ctx_stream(ctx));
        ws_free((DefocusWs *)*slot);
        delete (DefocusWs *)*slot;
        *slot = nullptr;
    }
}

static const double *default_heights() {
    static const std::vector<double> h = [] {
        std::vector<double> v(128);
        for (int i = 0; i < 128; i++) v[i] = 60.0 * pow(300.0 / 60.0, i / 127.0);
        return v;
    }();
    return h.data();
}
static const double DEFAULT_RADII[7] = {0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0};
static const double *default_seeings() {
    static const std::vector<double> s = [] {
        std::vector<double> v(29);
        for (int i = 0; i < 29; i++) v[i] = 0.8 + 0.05 * i;
        return v;
    }();
    return s.data();
}

extern "C" void lfdmi_default_defocus_params(lfdmi_defocus_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->Ro = 1250.0; o->Ri = 585.0;
    o->pixscale = 0.396; o->prof_half = 24.0; o->prof_step = 0.1; o->wing = 8;
    o->ovs = 8; o->max_shift = 5;
    o->n_h = 128; o->n_r = 7; o->n_seeing = 29;
    o->heights = default_heights(); o->radii = DEFAULT_RADII; o->seeings = default_seeings();
    o->delta_chi2 = 1.0 / o->prof_step;
}

static bool all_finite(const double *v, int n, double lo, bool lo_open) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i]) || (lo_open ? !(v[i] > lo) : !(v[i] >= lo))) return false;
    return true;
}

extern "C" int lfdmi_defocus_bank_create(lfdmi_ctx *ctx, const lfdmi_defocus_params *pp, lfdmi_defocus_bank **out) {
    if (!ctx) return LFDMI_ERR_ARG;
    if (!out) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    lfdmi_defocus_params q;
    if (pp) q = *pp; else lfdmi_default_defocus_params(&q);
    const double kd = q.prof_half / q.prof_step;
    const int K = (std::isfinite(kd) && kd >= 1 && kd <= 512) ? (int)llround(kd) : 0;
    if (K == 0 || fabs((double)K * q.prof_step - q.prof_half) > 1e-9 * q.prof_half || !(q.pixscale > 0) || !std::isfinite(q.pixscale) ||
        !(q.Ri >= 0) || !(q.Ro > q.Ri) || !std::isfinite(q.Ro) || q.wing < 1 || q.wing >= q.prof_half || q.ovs < 1 || q.ovs > 64 ||
        q.max_shift < 0 || q.max_shift > 64 || q.max_shift >= K || q.n_h < 1 || q.n_r < 1 || q.n_seeing < 1 ||
        q.n_h > 4096 || q.n_r > 64 || q.n_seeing > 1024 || !q.heights || !q.radii || !q.seeings || !std::isfinite(q.delta_chi2) ||
        !(q.delta_chi2 >= 0))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "defocus params out of range (include/lfdmi.h: lfdmi_defocus_params)");
    if (!all_finite(q.heights, q.n_h, 0.0, true) || !all_finite(q.radii, q.n_r, 0.0, false) || !all_finite(q.seeings, q.n_seeing, 0.0, true))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "defocus grid: heights and seeings must be > 0, radii >= 0, all finite");
    DefDev p;
    memset(&p, 0, sizeof(p));
    p.n_h = q.n_h; p.n_r = q.n_r; p.n_se = q.n_seeing; p.S = q.max_shift; p.K = K; p.ovs = q.ovs;
    p.nb = 2 * K + 1; p.nbp = (p.nb + 15) / 16 * 16; p.nq = 2 * K + 2 * p.S + 1;
    p.jcap = K * q.ovs;
    p.Ro = q.Ro; p.Ri = q.Ri; p.pixscale = q.pixscale; p.step = q.prof_step; p.P = q.prof_half; p.wing = q.wing;
    p.delta = q.prof_step * q.pixscale / q.ovs; p.F = q.ovs / q.prof_step;
    double smax = 0;
    for (int i = 0; i < q.n_seeing; i++) smax = std::max(smax, q.seeings[i]);
    const double nkd = floor(4.0 * (1.035 / DEF_FWHM2SIGMA * smax) / p.delta) + ceil(p.F / 2 - 0.5) + ceil(p.F) - 1;
    if (nkd > 1 << 20) return ctx_fail(ctx, LFDMI_ERR_ARG, "defocus params: seeing too wide for the fine grid");
    p.nkcap = (int)nkd;
    p.group = p.n_r * (2 * p.S + 1);
    p.n_groups = p.n_se * (p.n_h + 1);
    p.n_models = p.n_groups * p.n_r;
    p.ncol = (int64_t)p.n_models * (2 * p.S + 1);
    if ((double)p.ncol * p.nbp * 4 > 64e9 || p.ncol >= (1ll << 31))
        return ctx_fail(ctx, LFDMI_ERR_CAPACITY, "defocus bank larger than 64 GB");

    auto *b = new lfdmi_defocus_bank();
    b->ctx = ctx; b->device = ctx_device(ctx); b->p = p; b->delta_chi2 = q.delta_chi2;
    b->heights.assign(q.heights, q.heights + q.n_h);
    b->radii.assign(q.radii, q.radii + q.n_r);
    b->seeings.assign(q.seeings, q.seeings + q.n_seeing);
    const int n_od = (p.n_h + 1) * p.n_r;
    const size_t L = 2 * (size_t)p.jcap + 1, LK = 2 * (size_t)p.nkcap + 1;
    double *od = nullptr, *o = nullptr, *d = nullptr, *odf = nullptr, *ks = nullptr, *s = nullptr, *sb = nullptr;
    int *odhw = nullptr, *kshw = nullptr;
    auto cleanup = [&]() {
        for (void *x : {(void *)od, (void *)o, (void *)d, (void *)odf, (void *)ks, (void *)s, (void *)sb, (void *)odhw, (void *)kshw})
            if (x) hipFree(x);
    };
    auto run = [&]() -> int {
        hipStream_t st = ctx_stream(ctx);
        const size_t ng = (size_t)p.n_h + p.n_r + p.n_se;
        UHIP(hipMalloc(&b->d_grid, ng * sizeof(double)));
        UHIP(hipMalloc(&b->cols, (size_t)p.ncol * p.nbp * sizeof(float)));
        UHIP(hipMalloc(&b->samp, (size_t)p.n_models * p.nq * sizeof(double)));
        UHIP(hipMalloc(&b->gridv, (size_t)p.n_models * 2 * sizeof(double)));
        UHIP(hipMalloc(&b->valid, (size_t)p.n_models * sizeof(int)));
        UHIP(hipMalloc(&b->d_gvalid, (size_t)p.n_groups * sizeof(int)));
        b->bytes = ng * 8 + (size_t)p.ncol * p.nbp * 4 + (size_t)p.n_models * (p.nq * 8 + 16 + 4) + (size_t)p.n_groups * 4;
        UHIP(hipMalloc(&od, n_od * L * sizeof(double)));
        UHIP(hipMalloc(&o, n_od * L * sizeof(double)));
        UHIP(hipMalloc(&d, n_od * L * sizeof(double)));
        UHIP(hipMalloc(&odf, n_od * sizeof(double)));
        UHIP(hipMalloc(&odhw, n_od * sizeof(int)));
        UHIP(hipMalloc(&ks, p.n_se * LK * sizeof(double)));
        UHIP(hipMalloc(&s, p.n_se * LK * sizeof(double)));
        UHIP(hipMalloc(&sb, p.n_se * LK * sizeof(double)));
        UHIP(hipMalloc(&kshw, p.n_se * sizeof(int)));
        std::vector<double> g(b->heights);
        g.insert(g.end(), b->radii.begin(), b->radii.end());
        g.insert(g.end(), b->seeings.begin(), b->seeings.end());
        UHIP(hipMemcpyAsync(b->d_grid, g.data(), ng * sizeof(double), hipMemcpyHostToDevice, st));
        const double *dh = b->d_grid, *dr = dh + p.n_h, *ds = dr + p.n_r;
        k_def_od<<<n_od, 256, 0, st>>>(dh, dr, p, od, o, d, odhw, odf);
        ULAUNCH("k_def_od");
        k_def_kernel<<<p.n_se, 256, 0, st>>>(ds, p, ks, s, sb, kshw);
        ULAUNCH("k_def_kernel");
        k_def_sample<<<p.n_models, 256, 0, st>>>(dh, dr, ds, p, od, odhw, ks, kshw, b->samp, b->gridv, b->valid, b->cols);
        ULAUNCH("k_def_sample");
        std::vector<int> valid(p.n_models);
        b->dfwhm.resize(n_od);
        UHIP(hipMemcpyAsync(valid.data(), b->valid, valid.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(b->dfwhm.data(), odf, n_od * sizeof(double), hipMemcpyDeviceToHost, st));
        b->gridv_h.resize((size_t)p.n_models * 2);
        UHIP(hipMemcpyAsync(b->gridv_h.data(), b->gridv, b->gridv_h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        UHIP(hipStreamSynchronize(st));
        b->gvalid.assign(p.n_groups, 0);
        for (int m = 0; m < p.n_models; m++)
            if (valid[m]) b->gvalid[m / p.n_r] = 1;
        UHIP(hipMemcpy(b->d_gvalid, b->gvalid.data(), p.n_groups * sizeof(int), hipMemcpyHostToDevice));
        return 0;
    };
    rc = run();
    cleanup();
    if (rc) { lfdmi_defocus_bank_destroy(b); return rc; }
    *out = b;
    return 0;
}

extern "C" void lfdmi_defocus_bank_destroy(lfdmi_defocus_bank *b) {
    if (!b) return;
    // every bank call returns after its stream has drained, so no work of the context still reads these buffers; hipFree
    // needs no stream
    hipSetDevice(b->device);
    for (void *x : {(void *)b->d_grid, (void *)b->cols, (void *)b->samp, (void *)b->gridv, (void *)b->valid, (void *)b->d_gvalid})
        if (x) hipFree(x);
    delete b;
}

extern "C" int lfdmi_defocus_bank_dims(const lfdmi_defocus_bank *b, int64_t *n_columns, int64_t *n_models, int32_t *n_bins) {
    if (!b) return LFDMI_ERR_ARG;
    if (n_columns) *n_columns = b->p.ncol;
    if (n_models) *n_models = b->p.n_models;
    if (n_bins) *n_bins = b->p.nb;
    return 0;
}

extern "C" int lfdmi_defocus_bank_read(const lfdmi_defocus_bank *b, float *columns, lfdmi_defocus_model *grid) {
    if (!b) return LFDMI_ERR_ARG;
    lfdmi_ctx *ctx = b->ctx;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    const DefDev &p = b->p;
    if (columns)
        UHIP(hipMemcpy2D(columns, p.nb * sizeof(float), b->cols, p.nbp * sizeof(float), p.nb * sizeof(float), p.ncol, hipMemcpyDeviceToHost));
    if (grid) {
        const std::vector<double> &gv = b->gridv_h;
        std::vector<int> valid(p.n_models);
        UHIP(hipMemcpy(valid.data(), b->valid, valid.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int m = 0; m < p.n_models; m++) {
            const int ir = m % p.n_r, ih = (m / p.n_r) % (p.n_h + 1), ise = m / (p.n_r * (p.n_h + 1));
            lfdmi_defocus_model &g = grid[m];
            g.h_km = ih == p.n_h ? INFINITY : b->heights[ih];
            g.radius_m = b->radii[ir];
            g.sfwhm = b->seeings[ise];
            g.dfwhm = b->dfwhm[ih * p.n_r + ir];
            g.ofwhm = gv[(size_t)m * 2];
            g.depth = gv[(size_t)m * 2 + 1];
            g.valid = valid[m];
            g.pad = 0;
        }
    }
    return 0;
}

static void fit_blank(lfdmi_defocus_fit *o, int status) {
    const double nan = NAN;
    o->status = status; o->shift = 0; o->dof = 0; o->column = -1;
    o->h_km = o->radius_m = o->seeing_arcsec = o->amplitude = o->offset = o->chi2 = nan;
    o->h_lo = o->h_hi = o->chi2_focus = o->model_ofwhm = o->model_depth = nan;
}

template <class T> static int ws_buf(lfdmi_ctx *ctx, T **ptr, size_t count) {
    if (*ptr) { UHIP(hipFree(*ptr)); *ptr = nullptr; }
    UHIP(hipMalloc((void **)ptr, std::max<size_t>(count, 1) * sizeof(T)));
    return 0;
}

#define FIT_CHUNK 4096 // trails per GEMM

extern "C" int lfdmi_fit_defocus(lfdmi_ctx *ctx, const lfdmi_defocus_bank *b, const lfdmi_trail *trails, const float *profiles, int n,
                                 const float *seeing, lfdmi_defocus_fit *out, float *chi2_by_height) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!b || b->ctx != ctx) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_fit_defocus: the bank belongs to another context");
    if (n < 0 || (n > 0 && (!trails || !profiles || !out))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    const DefDev &p = b->p;
    const int nb = p.nb, nh1 = p.n_h + 1;
    // which trails are fitted, and in which seeing slice
    std::vector<int> slice(n, -2);
    for (int i = 0; i < n; i++) {
        const float *v = profiles + (size_t)i * nb;
        int st = LFDMI_DEFOCUS_OK;
        if (trails[i].status != LFDMI_TRAIL_OK) st = LFDMI_DEFOCUS_NOT_MEASURED;
        else {
            for (int k = 0; k < nb; k++)
                if (std::isnan(v[k])) { st = LFDMI_DEFOCUS_GAPS; break; }
            if (st == LFDMI_DEFOCUS_OK && !(trails[i].noise > 0)) st = LFDMI_DEFOCUS_NO_NOISE;
        }
        fit_blank(&out[i], st);
        if (chi2_by_height) for (int h = 0; h < nh1; h++) chi2_by_height[(size_t)i * nh1 + h] = NAN;
        if (st != LFDMI_DEFOCUS_OK) continue;
        slice[i] = -1;
        if (seeing && !std::isnan(seeing[i])) {
            int best = 0;
            for (int j = 1; j < p.n_se; j++) {
                const double dj = fabs(b->seeings[j] - (double)seeing[i]), db = fabs(b->seeings[best] - (double)seeing[i]);
                if (dj < db || (dj == db && b->seeings[j] < b->seeings[best])) best = j;
            }
            slice[i] = best;
        }
    }
    std::vector<int> act;
    for (int i = 0; i < n; i++)
        if (slice[i] >= -1) act.push_back(i);
    if (act.empty()) return 0;

    void **slot = ctx_defocus(ctx, ws_release);
    if (!*slot) *slot = new DefocusWs();
    DefocusWs &W = *(DefocusWs *)*slot;
    hipStream_t st = ctx_stream(ctx);
    const size_t rows = std::min<size_t>(act.size(), FIT_CHUNK), rows_pad = (rows + DEF_BM - 1) / DEF_BM * DEF_BM;
    if (W.cap_rows < rows_pad || W.cap_nbp < (size_t)p.nbp || W.cap_groups < (size_t)p.n_groups || W.cap_h < (size_t)nh1) {
        UHIP(hipStreamSynchronize(st));
        const size_t R = std::max(rows_pad, W.cap_rows), NBP = std::max<size_t>(p.nbp, W.cap_nbp),
                     G = std::max<size_t>(p.n_groups, W.cap_groups), H = std::max<size_t>(nh1, W.cap_h);
        if ((rc = ws_buf(ctx, &W.V, R * NBP)) || (rc = ws_buf(ctx, &W.prof, R * NBP)) || (rc = ws_buf(ctx, &W.noise, R)) ||
            (rc = ws_buf(ctx, &W.res, R * 5)) || (rc = ws_buf(ctx, &W.cbh, R * H)) || (rc = ws_buf(ctx, &W.slice, R)) ||
            (rc = ws_buf(ctx, &W.gmax, R * G))) {
            ws_free(&W);
            return rc;
        }
        W.cap_rows = R; W.cap_nbp = NBP; W.cap_groups = G; W.cap_h = H;
    }
    std::vector<float> hv, hp;
    std::vector<double> hn, hres, hcbh;
    std::vector<int> hs;
    for (size_t a0 = 0; a0 < act.size(); a0 += FIT_CHUNK) {
        const int na = (int)std::min<size_t>(FIT_CHUNK, act.size() - a0);
        const int na_pad = (na + DEF_BM - 1) / DEF_BM * DEF_BM;
        hv.assign((size_t)na_pad * p.nbp, 0.0f);
        hp.assign((size_t)na * nb, 0.0f);
        hn.assign(na, 0.0);
        hs.assign(na_pad, -2);
        for (int r = 0; r < na; r++) {
            const int i = act[a0 + r];
            const float *v = profiles + (size_t)i * nb;
            double s = 0.0;
            for (int k = 0; k < nb; k++) s += v[k];
            const double mean = s / nb;
            for (int k = 0; k < nb; k++) hv[(size_t)r * p.nbp + k] = (float)((double)v[k] - mean);
            memcpy(&hp[(size_t)r * nb], v, nb * sizeof(float));
            hn[r] = trails[i].noise;
            hs[r] = slice[i];
        }
        UHIP(hipMemcpyAsync(W.V, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(W.prof, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(W.noise, hn.data(), hn.size() * sizeof(double), hipMemcpyHostToDevice, st));
        UHIP(hipMemcpyAsync(W.slice, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice, st));
        UHIP(hipMemsetAsync(W.gmax, 0, (size_t)na * p.n_groups * sizeof(unsigned), st));
        const dim3 grid((unsigned)((p.ncol + DEF_BN - 1) / DEF_BN), (unsigned)(na_pad / DEF_BM));
        k_def_gemm<<<grid, 256, 0, st>>>(W.V, na, b->cols, p, W.slice, b->valid, W.gmax);
        ULAUNCH("k_def_gemm");
        k_def_pick<<<na, 64, 0, st>>>(W.V, W.prof, W.noise, b->cols, b->samp, p, W.slice, b->valid, b->d_gvalid, W.gmax, W.res, W.cbh);
        ULAUNCH("k_def_pick");
        hres.resize((size_t)na * 5);
        hcbh.resize((size_t)na * nh1);
        UHIP(hipMemcpyAsync(hres.data(), W.res, hres.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(hcbh.data(), W.cbh, hcbh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        UHIP(hipStreamSynchronize(st));
        for (int r = 0; r < na; r++) {
            const int i = act[a0 + r];
            const double *rs = &hres[(size_t)r * 5], *cb = &hcbh[(size_t)r * nh1];
            lfdmi_defocus_fit *o = &out[i];
            if (chi2_by_height) for (int h = 0; h < nh1; h++) chi2_by_height[(size_t)i * nh1 + h] = (float)cb[h];
            if (!(rs[0] >= 0)) { fit_blank(o, LFDMI_DEFOCUS_NO_MODEL); continue; }
            const int64_t col = (int64_t)rs[0];
            const int ns = 2 * p.S + 1, m = (int)(col / ns);
            const int ir = m % p.n_r, ih = (m / p.n_r) % nh1, ise = m / (p.n_r * nh1);
            o->status = LFDMI_DEFOCUS_OK;
            o->column = (int32_t)col;
            o->shift = (int)(col % ns) - p.S;
            o->dof = 2 * p.K - 1;
            o->h_km = ih == p.n_h ? INFINITY : b->heights[ih];
            o->radius_m = b->radii[ir];
            o->seeing_arcsec = b->seeings[ise];
            o->amplitude = rs[1]; o->offset = rs[2]; o->chi2 = rs[3];
            o->chi2_focus = cb[p.n_h];
            double cmin = INFINITY;
            for (int h = 0; h < nh1; h++)
                if (cb[h] < cmin) cmin = cb[h];
            double lo = INFINITY, hi = -INFINITY;
            for (int h = 0; h < nh1; h++)
                if (cb[h] <= cmin + b->delta_chi2) {
                    const double hk = h == p.n_h ? INFINITY : b->heights[h];
                    lo = std::min(lo, hk); hi = std::max(hi, hk);
                }
            o->h_lo = lo; o->h_hi = hi;
            o->model_ofwhm = b->gridv_h[(size_t)m * 2]; o->model_depth = b->gridv_h[(size_t)m * 2 + 1];
        }
    }
    return 0;
}
