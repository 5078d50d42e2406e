// stack.hip -- host side of the stacked cross-sections (include/lfdmi.h: stacked cross-sections; kernels in k_stack.h).  Its own
// translation unit in its own directory, like sky/, inject/ and radon/: the detection kernels' code object does not change with
// it.  The context's internals are reached through unit.h.  The call keeps no state: its device
// memory comes from the stream's pool (hipMallocAsync) and goes back before the call returns.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../unit.h"
#include "../limits/limits.h"
#include "k_stack.h"

#define STK_STAGE_BYTES (1ull << 30)   // device staging of host frames at a time
#define STK_PART_BYTES (128ull << 20)  // block sums and counts of one launch

namespace {
struct Line {
    double a1, b1, g, cosphi;
    double bc(double a) const { return b1 + g * (a - a1); }
};
struct Seg {
    int status = LFDMI_STACK_OK, xmajor = 0, a_first = 0, a_last = -1, amid = 0, n_pass = 0;
    Line l0, l;
};

const double kNaN = std::numeric_limits<double>::quiet_NaN();

double lowmed(std::vector<double> &v) {   // rank floor((m-1)/2) of the ascending values; NaN for none
    if (v.empty()) return kNaN;
    std::sort(v.begin(), v.end());
    return v[(v.size() - 1) / 2];
}

double cosphi_of(double g) { return 1.0 / sqrt(1.0 + g * g); }

// definition step 2
void geometry(const lfdmi_stack_segment &s, int h, int w, int min_cols, Seg &o) {
    const double c[4] = {s.x1, s.y1, s.x2, s.y2};
    for (double v : c)
        if (!std::isfinite(v) || fabs(v) > 1e6) { o.status = LFDMI_STACK_BAD_SEGMENT; return; }
    const double dx = s.x2 - s.x1, dy = s.y2 - s.y1;
    if (dx == 0.0 && dy == 0.0) { o.status = LFDMI_STACK_BAD_SEGMENT; return; }
    o.xmajor = fabs(dx) >= fabs(dy);
    const double a1 = o.xmajor ? s.x1 : s.y1, b1 = o.xmajor ? s.y1 : s.x1, a2 = o.xmajor ? s.x2 : s.y2, b2 = o.xmajor ? s.y2 : s.x2;
    const int A = o.xmajor ? w : h;
    o.l.a1 = a1; o.l.b1 = b1;
    o.l.g = (b2 - b1) / (a2 - a1);
    o.l.cosphi = cosphi_of(o.l.g);
    o.l0 = o.l;
    o.a_first = (int)std::max(ceil(std::min(a1, a2)), 0.0);
    o.a_last = (int)std::min(floor(std::max(a1, a2)), (double)(A - 1));
    o.amid = (o.a_first + o.a_last + 1) >> 1;
    if (o.a_last - o.a_first + 1 < min_cols) o.status = LFDMI_STACK_TOO_SHORT;
}

// definition step 5 for one half: its centre's shift and score; false: no wing bin or no scored bin
bool half_centre(const float *A, const int32_t *N, int K, const lfdmi_stack_params &p, double &shift, double &score) {
    const int nb = 2 * K + 1;
    std::vector<double> wing;
    for (int k = 0; k < nb; k++)
        if (fabs((double)(k - K) * p.step) >= p.prof_half - (double)p.wing && N[k] > 0) wing.push_back((double)A[k] / (double)N[k]);
    if (wing.empty()) return false;
    const double bkg = lowmed(wing);
    const int hb = (int)floor(p.box / (2.0 * p.step));
    int best = -1;
    for (int k = 0; k < nb; k++) {
        if (!(fabs((double)(k - K) * p.step) <= p.max_shift)) continue;
        double SA = 0.0, SN = 0.0;
        for (int j = std::max(k - hb, 0); j <= std::min(k + hb, 2 * K); j++) { SA = SA + (double)A[j]; SN = SN + (double)N[j]; }
        if (!(SN > 0.0)) continue;
        const double sc = (SA - bkg * SN) / sqrt(SN);
        if (best < 0 || sc > score) { best = k; score = sc; }
    }
    if (best < 0) return false;
    shift = (double)(best - K) * p.step;
    return true;
}

// definition step 5: the line of the next pass; false: refinement stops
bool refine(Seg &s, const float *A, const int32_t *N, int K, const lfdmi_stack_params &p, double sigma) {
    const int nb = 2 * K + 1;
    double uL = 0, uR = 0, sL = 0, sR = 0;
    if (!half_centre(A, N, K, p, uL, sL) || !half_centre(A + nb, N + nb, K, p, uR, sR)) return false;
    const double thr = p.k_ref * sigma;
    if (!(sL >= thr) || !(sR >= thr)) return false;
    const double aL = ((double)s.a_first + (double)(s.amid - 1)) * 0.5, aR = ((double)s.amid + (double)s.a_last) * 0.5;
    const double bL = s.l.bc(aL) + uL / s.l.cosphi, bR = s.l.bc(aR) + uR / s.l.cosphi;
    const double g = (bR - bL) / (aR - aL);
    if (!(fabs(g) <= 2.0)) return false;
    s.l.a1 = aL; s.l.b1 = bL; s.l.g = g; s.l.cosphi = cosphi_of(g);
    return true;
}

// definition step 6
void finalize(const Seg &s, const float *A, const int32_t *N, int K, const lfdmi_stack_params &p, lfdmi_stack &o, float *row) {
    const int nb = 2 * K + 1;
    std::vector<float> m(nb), v(nb);
    std::vector<double> ub(nb), tmp;
    int min_valid = std::numeric_limits<int>::max();
    for (int k = 0; k < nb; k++) {
        const float a = A[k] + A[nb + k];
        const int n = N[k] + N[nb + k];
        m[k] = n > 0 ? a / (float)n : std::numeric_limits<float>::quiet_NaN();
        ub[k] = (double)(k - K) * p.step;
        min_valid = std::min(min_valid, n);
    }
    const double edge = p.prof_half - (double)p.wing;
    for (int k = 0; k < nb; k++)
        if (fabs(ub[k]) >= edge && !std::isnan(m[k])) tmp.push_back((double)m[k]);
    const bool wings = !tmp.empty();
    const float bg = wings ? (float)lowmed(tmp) : std::numeric_limits<float>::quiet_NaN();
    tmp.clear();
    float peak = -std::numeric_limits<float>::infinity();
    for (int k = 0; k < nb; k++) {
        v[k] = m[k] - bg;
        if (!std::isnan(v[k])) {
            peak = std::max(peak, v[k]);
            if (fabs(ub[k]) >= edge) tmp.push_back(fabs((double)v[k]));
        }
    }
    const double noise = wings ? 1.4826 * lowmed(tmp) : kNaN;
    o.n_col = s.a_last - s.a_first + 1;
    o.min_valid = min_valid;
    o.n_pass = s.n_pass;
    o.background = (double)bg; o.noise = noise; o.peak = (double)peak;
    o.fwhm = o.fwhm_arcsec = o.depth = kNaN;
    if (peak > 0.0f) {
        const float half = peak / 2.0f;
        int left = -1, right = -1;
        for (int k = 0; k < nb; k++)
            if (v[k] >= half) { if (left < 0) left = k; right = k; }
        o.fwhm = left == right ? 0.0 : fabs(ub[right]) + fabs(ub[left]);
        o.fwhm_arcsec = o.fwhm * p.pixscale;
        o.depth = ((double)peak - (double)v[K]) / (double)peak * 100.0;
    }
    double sum = 0.0;
    int ncore = 0;
    for (int k = 0; k < nb; k++)
        if (fabs(ub[k]) < edge) { sum = sum + (double)v[k]; ncore++; }
    o.flux = p.step * sum;
    o.flux_err = p.step * noise * sqrt((double)ncore);
    o.snr = o.flux / o.flux_err;
    o.status = (peak > 0.0f && (double)peak >= p.k_sig * noise) ? LFDMI_STACK_OK : LFDMI_STACK_TOO_FAINT;
    const double af = (double)s.a_first, al = (double)s.a_last;
    const double bf = s.l.bc(af), bl = s.l.bc(al);
    o.x1 = s.xmajor ? af : bf; o.y1 = s.xmajor ? bf : af;
    o.x2 = s.xmajor ? al : bl; o.y2 = s.xmajor ? bl : al;
    const double dx = o.x2 - o.x1, dy = o.y2 - o.y1, len = sqrt(dx * dx + dy * dy);
    line_rho_theta(o.x1, o.y1, dx / len, dy / len, &o.rho, &o.theta);
    const double am = (af + al) * 0.5;
    o.shift = (s.l.bc(am) - s.l0.bc(am)) * s.l0.cosphi;
    o.tilt = atan(s.l.g) - atan(s.l0.g);
    if (row) memcpy(row, v.data(), (size_t)nb * sizeof(float));
}

bool params_ok(const lfdmi_stack_params &q, int &K) {
    if (!std::isfinite(q.prof_half) || !std::isfinite(q.step) || !(q.step > 0) || !(q.prof_half > 0)) return false;
    const double kk = q.prof_half / q.step;
    K = (int)floor(kk + 0.5);
    if (K < 1 || K > 512 || fabs(kk - (double)K) > 1e-9 * kk) return false;
    if (!(q.prof_half + q.step / 2.0 <= LFDMI_STACK_MAX_HALF)) return false;
    if (q.wing < 1 || !((double)q.wing < q.prof_half) || q.n_iter < 0 || q.n_iter > 16 || q.min_cols < 2) return false;
    if (std::isnan(q.clip) || !(q.clip > 0)) return false;
    if (!std::isfinite(q.box) || q.box < 0 || !std::isfinite(q.max_shift) || q.max_shift < 0) return false;
    if (std::isnan(q.k_sig) || std::isnan(q.k_ref) || !std::isfinite(q.pixscale)) return false;
    return true;
}
}   // namespace

extern "C" void lfdmi_default_stack_params(lfdmi_stack_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->wing = 8; o->n_iter = 2; o->min_cols = 64; o->clip = 0.125f;
    o->prof_half = 24.0; o->step = 0.5; o->box = 4.0; o->max_shift = 8.0;
    o->k_sig = 6.0; o->k_ref = 4.0; o->pixscale = 0.396;
}

extern "C" int lfdmi_stack_profiles(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_stack_segment *segs,
                                    int n_seg, const float *sigma, const lfdmi_stack_params *pp, lfdmi_stack *out, float *profiles, float *sums,
                                    int32_t *counts) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    UnitState *unit = ctx_unit(ctx);   // (one look-up a call: the limits and the split it records)
    UnitSplit *split = &unit->split;
    if ((rc = unit_dtype(ctx, "lfdmi_stack_profiles", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (n < 0 || n_seg < 0 || h < 1 || w < 1 || h > 65536 || w > 65536)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stack_profiles: n, n_seg >= 0, h and w 1 .. 65536");
    if ((n > 0 && !frames) || (n_seg > 0 && (!segs || !out))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    lfdmi_stack_params q;
    if (pp) q = *pp; else lfdmi_default_stack_params(&q);
    int K = 0;
    if (!params_ok(q, K)) return ctx_fail(ctx, LFDMI_ERR_ARG, "stack params out of range (include/lfdmi.h: lfdmi_stack_params)");
    for (int i = 0; i < n_seg; i++)
        if (segs[i].frame < 0 || segs[i].frame >= n)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_stack_profiles: segment " + std::to_string(i) + ": frame outside [0, n)");
    if ((rc = unit_sigma(ctx, "lfdmi_stack_profiles", sigma, n, nullptr))) return rc;
    if (n_seg == 0) return 0;

    const int nb = 2 * K + 1;
    const size_t N = (size_t)h * w, FB = N * sizeof(float), row2 = (size_t)2 * nb;
    std::vector<Seg> sg(n_seg);
    std::vector<float> hA((size_t)n_seg * row2, 0.0f);      // A_L, A_R of every segment's last pass
    std::vector<int32_t> hN((size_t)n_seg * row2, 0);
    for (int i = 0; i < n_seg; i++) geometry(segs[i], h, w, q.min_cols, sg[i]);

    // groups of frames: device frames are used where they are, host frames that carry a segment are staged STK_STAGE_BYTES at a time
    const bool in_dev = loc == LFDMI_DEVICE;
    std::vector<int> slot(n, -1), group_of(n, -1);
    std::vector<std::vector<int>> gframes;
    {
        std::vector<char> used(n, 0);
        for (int i = 0; i < n_seg; i++)
            if (sg[i].status == LFDMI_STACK_OK) used[segs[i].frame] = 1;
        const size_t per = in_dev ? (size_t)n : std::max<size_t>(1, unit->limit_of(LIM_STAGE_BYTES, STK_STAGE_BYTES) / FB);
        for (int f = 0; f < n; f++) {
            if (!used[f]) continue;
            if (gframes.empty() || gframes.back().size() >= per) gframes.emplace_back();
            slot[f] = in_dev ? f : (int)gframes.back().size();
            group_of[f] = (int)gframes.size() - 1;
            gframes.back().push_back(f);
        }
    }

    StkDev dp;
    memset(&dp, 0, sizeof(dp));
    dp.h = h; dp.w = w; dp.be = dtype == LFDMI_F32_BE; dp.K = K; dp.nb = nb; dp.clip = q.clip;
    dp.inv = 1.0 / q.step; dp.kc = (double)K + 0.5;
    const double reach = q.prof_half + q.step / 2.0;
    const size_t items_max = std::max<size_t>(1, unit->limit_of(LIM_STACK_PART_BYTES, STK_PART_BYTES) / (8 * (size_t)nb));

    hipStream_t st = ctx_stream(ctx);
    for (size_t gi = 0; gi < gframes.size(); gi++) {
        std::vector<int> active;
        for (int i = 0; i < n_seg; i++)
            if (sg[i].status == LFDMI_STACK_OK && group_of[segs[i].frame] == (int)gi) active.push_back(i);
        if (active.empty()) continue;
        split->chunks++;
        // the largest launch of this group: whole segments up to items_max blocks
        size_t cap_items = 0;
        for (int i : active) cap_items = std::max<size_t>(cap_items, (size_t)((sg[i].a_last >> 5) - (sg[i].a_first >> 5) + 2));
        cap_items = std::max(cap_items, items_max);
        const size_t na0 = active.size();

        // (host arrays the queued copies read are declared ahead of the pool: it waits before they go)
        std::vector<StkSeg> hs;
        std::vector<std::vector<StkItem>> litems;
        std::vector<std::vector<StkHalf>> lhalves;
        std::vector<float> pA(na0 * row2);
        std::vector<int32_t> pN(na0 * row2);
        Pool pool(st);
        uint32_t *d_buf = nullptr;
        StkSeg *d_seg = nullptr;
        StkItem *d_item = nullptr;
        StkHalf *d_half = nullptr;
        float *d_ps = nullptr, *d_sum = nullptr;
        int *d_pc = nullptr, *d_cnt = nullptr;
        size_t total_items = 0;
        for (int i : active) total_items += (size_t)((sg[i].a_last >> 5) - (sg[i].a_first >> 5) + 2);
        cap_items = std::min(cap_items, total_items);
        UHIP(pool.get(&d_seg, na0));
        UHIP(pool.get(&d_item, cap_items));
        UHIP(pool.get(&d_half, 2 * na0));
        UHIP(pool.get(&d_ps, cap_items * nb));
        UHIP(pool.get(&d_pc, cap_items * nb));
        UHIP(pool.get(&d_sum, na0 * row2));
        UHIP(pool.get(&d_cnt, na0 * row2));
        const uint32_t *base = (const uint32_t *)frames;
        if (!in_dev) {
            UHIP(pool.get(&d_buf, gframes[gi].size() * N));
            for (size_t k = 0; k < gframes[gi].size(); k++)
                UHIP(hipMemcpyAsync(d_buf + k * N, (const char *)frames + (size_t)gframes[gi][k] * FB, FB, hipMemcpyHostToDevice, st));
            base = d_buf;
        }
        for (int pass = 0; pass <= q.n_iter && !active.empty(); pass++) {
            const size_t na = active.size();
            hs.assign(na, StkSeg());
            litems.clear();
            lhalves.clear();
            int S = 1;
            for (size_t e = 0; e < na; e++) {
                const Seg &s = sg[active[e]];
                StkSeg &o = hs[e];
                o.a1 = s.l.a1; o.b1 = s.l.b1; o.g = s.l.g; o.cosphi = s.l.cosphi;
                o.halfband = reach / s.l.cosphi;
                o.wb = q.step / s.l.cosphi;
                o.frame_off = (long long)((size_t)slot[segs[active[e]].frame] * N);
                o.xmajor = s.xmajor;
                o.E = (int)ceil(2.0 * o.halfband + fabs(s.l.g) * (double)(STK_COLS - 1)) + 6;
                S = std::max(S, o.E);
            }
            S |= 1;
            if (S > STK_MAX_STRIDE) return ctx_fail(ctx, LFDMI_ERR_CAPACITY, "lfdmi_stack_profiles: the band does not fit the LDS tile");
            dp.S = S;
            UHIP(hipMemcpyAsync(d_seg, hs.data(), na * sizeof(StkSeg), hipMemcpyHostToDevice, st));
            // launches of whole segments; the item and half lists of every launch live until the pass's wait
            for (size_t e0 = 0; e0 < na;) {
                litems.emplace_back();
                lhalves.emplace_back();
                std::vector<StkItem> &it = litems.back();
                std::vector<StkHalf> &hv = lhalves.back();
                size_t e = e0;
                for (; e < na; e++) {
                    const Seg &s = sg[active[e]];
                    const size_t need = (size_t)((s.a_last >> 5) - (s.a_first >> 5) + 2);
                    if (e > e0 && it.size() + need > cap_items) break;
                    const int lo[2] = {s.a_first, s.amid}, hi[2] = {s.amid - 1, s.a_last};
                    for (int hf = 0; hf < 2; hf++) {
                        StkHalf H;
                        H.item0 = (int)it.size(); H.out = (int)(2 * e + hf); H.pad = 0;
                        for (int a = lo[hf]; a <= hi[hf];) {
                            const int end = std::min(hi[hf], (a | (STK_COLS - 1)));
                            it.push_back(StkItem{(int)e, a, end, 0});
                            a = end + 1;
                        }
                        H.n_items = (int)it.size() - H.item0;
                        hv.push_back(H);
                    }
                }
                if (it.size() > cap_items) return ctx_fail(ctx, LFDMI_ERR_CAPACITY, "lfdmi_stack_profiles: block list overflow");
                UHIP(hipMemcpyAsync(d_item, it.data(), it.size() * sizeof(StkItem), hipMemcpyHostToDevice, st));
                UHIP(hipMemcpyAsync(d_half + 2 * e0, hv.data(), hv.size() * sizeof(StkHalf), hipMemcpyHostToDevice, st));
                if (!it.empty()) {
                    k_stack_block<<<(unsigned)it.size(), STK_THREADS, (size_t)STK_COLS * S * 8, st>>>(base, d_seg, d_item, dp, d_ps, d_pc);
                    ULAUNCH("k_stack_block");
                }
                k_stack_combine<<<(unsigned)hv.size(), STK_THREADS, 0, st>>>(d_half + 2 * e0, nb, d_ps, d_pc, d_sum, d_cnt);
                ULAUNCH("k_stack_combine");
                if (split->chunks == 1 && pass == 0) split->launches++;
                e0 = e;
            }
            UHIP(hipMemcpyAsync(pA.data(), d_sum, na * row2 * sizeof(float), hipMemcpyDeviceToHost, st));
            UHIP(hipMemcpyAsync(pN.data(), d_cnt, na * row2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            UHIP(hipStreamSynchronize(st));
            std::vector<int> next;
            for (size_t e = 0; e < na; e++) {
                const int i = active[e];
                Seg &s = sg[i];
                s.n_pass = pass + 1;
                const double sgm = sigma ? (double)sigma[segs[i].frame] : (double)0.025f;
                if (pass < q.n_iter && refine(s, pA.data() + e * row2, pN.data() + e * row2, K, q, sgm)) { next.push_back(i); continue; }
                memcpy(hA.data() + (size_t)i * row2, pA.data() + e * row2, row2 * sizeof(float));
                memcpy(hN.data() + (size_t)i * row2, pN.data() + e * row2, row2 * sizeof(int32_t));
            }
            active.swap(next);
        }
        pool.release();
    }

    for (int i = 0; i < n_seg; i++) {
        lfdmi_stack &o = out[i];
        float *row = profiles ? profiles + (size_t)i * nb : nullptr;
        if (sg[i].status != LFDMI_STACK_OK) {
            memset(&o, 0, sizeof(o));
            o.status = sg[i].status;
            o.rho = o.theta = o.x1 = o.y1 = o.x2 = o.y2 = o.background = o.noise = o.peak = o.fwhm = o.fwhm_arcsec = o.depth = kNaN;
            o.flux = o.flux_err = o.snr = o.shift = o.tilt = kNaN;
            if (sg[i].status == LFDMI_STACK_TOO_SHORT) o.n_col = std::max(0, sg[i].a_last - sg[i].a_first + 1);
            if (row)
                for (int k = 0; k < nb; k++) row[k] = std::numeric_limits<float>::quiet_NaN();
            continue;
        }
        memset(&o, 0, sizeof(o));
        finalize(sg[i], hA.data() + (size_t)i * row2, hN.data() + (size_t)i * row2, K, q, o, row);
    }
    if (sums) memcpy(sums, hA.data(), hA.size() * sizeof(float));
    if (counts) memcpy(counts, hN.data(), hN.size() * sizeof(int32_t));
    return 0;
}
