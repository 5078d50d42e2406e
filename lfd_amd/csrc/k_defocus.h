// k_defocus.h -- defocus bank and fit (include/lfdmi.h: defocus fit).  Bank: double precision on the fine grid, one block per
// model; fit: a float32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32) whose epilogue keeps, per trail, the largest score of
// every (seeing, height) group, then one block per trail picks the column and fits it in double.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define DEF_RAD2ARCSEC 206264.806247
#define DEF_PI 3.14159265358979323846
#define DEF_FWHM2SIGMA 2.436

struct DefDev {
    int n_h, n_r, n_se;     // grid lengths (height index n_h: the focus model)
    int S, K, ovs;          // max shift, profile half-width in bins, fine steps per bin
    int nb, nbp, nq;        // 2K+1 bins, the padded row length (multiple of 16), 2K+2S+1 samples per model
    int jcap;               // half-width of an OD row: K ovs (the profile's half-width)
    int nkcap;              // half-width of a KS row
    int n_models, group;    // n_se (n_h+1) n_r; columns per (seeing, height) group: n_r (2S+1)
    int n_groups;           // n_se (n_h+1)
    int64_t ncol;
    double Ro, Ri, pixscale, step, delta, F, P, wing;
};

__device__ inline void def_angles(const DefDev &p, const double *heights, const double *radii, int ih, int ir, double *to, double *ti,
                                  double *rho) {
    *to = *ti = *rho = 0.0;
    if (ih == p.n_h) return; // focus: no D, a point
    const double h = heights[ih];
    *to = p.Ro / (h * 1e6) * DEF_RAD2ARCSEC;
    *ti = p.Ri / (h * 1e6) * DEF_RAD2ARCSEC;
    *rho = radii[ir] / (2.0 * h * 1000.0) * DEF_RAD2ARCSEC;
}

// calc_fwhm's rule over n samples y at positions (j - c) * dx: first / last >= peak / 2, |x_right| + |x_left|
__device__ inline double def_fwhm(const double *y, int n, int c, double dx) {
    double peak = y[0];
    for (int j = 1; j < n; j++) peak = y[j] > peak ? y[j] : peak;
    int l = -1, r = -1;
    for (int j = 0; j < n; j++)
        if (y[j] >= peak / 2) { if (l < 0) l = j; r = j; }
    if (l == r) return 0.0;
    return fabs((r - c) * dx) + fabs((l - c) * dx);
}

// O (x) D of model (ih, ir) on the fine grid: od row [2 jcap + 1] (centre jcap); scratch o / d rows of the same length.
// od_hw: the half-width, -1 when it exceeds jcap (the model does not fit the profile); dfwhm: its FWHM in arcsec.
__global__ void k_def_od(const double *heights, const double *radii, DefDev p, double *od, double *o, double *d, int *od_hw,
                         double *dfwhm) {
    const int m = blockIdx.x, ih = m / p.n_r, ir = m % p.n_r, L = 2 * p.jcap + 1, c = p.jcap;
    double to, ti, rho;
    def_angles(p, heights, radii, ih, ir, &to, &ti, &rho);
    const bool point = ih == p.n_h || radii[ir] == 0.0;
    const double nDd = floor(to / p.delta), nOd = point ? 0.0 : floor(rho / p.delta);
    double *O = od + (size_t)m * L, *so = o + (size_t)m * L, *sd = d + (size_t)m * L;
    if (nDd + nOd > p.jcap) {
        if (threadIdx.x == 0) { od_hw[m] = -1; dfwhm[m] = NAN; }
        return;
    }
    const int nD = (int)nDd, nO = (int)nOd, hw = nD + nO;
    const double dn = 2.0 / (DEF_PI * (to * to - ti * ti)), on = point ? 0.0 : 2.0 / (DEF_PI * rho * rho);
    for (int j = -nD + (int)threadIdx.x; j <= nD; j += blockDim.x) {
        if (ih == p.n_h) { sd[c + j] = 1.0; continue; }
        const double x = j * p.delta, a = to * to - x * x, b = ti * ti - x * x;
        sd[c + j] = dn * ((a > 0 ? sqrt(a) : 0.0) - (fabs(x) < ti && b > 0 ? sqrt(b) : 0.0));
    }
    for (int j = -nO + (int)threadIdx.x; j <= nO; j += blockDim.x) {
        if (point) { so[c + j] = 1.0; continue; }
        const double x = j * p.delta, a = rho * rho - x * x;
        so[c + j] = on * (a > 0 ? sqrt(a) : 0.0);
    }
    __syncthreads();
    __shared__ double sums[2];
    if (threadIdx.x == 0) { // unit sums, ascending index
        double s = 0.0;
        for (int j = -nD; j <= nD; j++) s += sd[c + j];
        sums[0] = s;
        s = 0.0;
        for (int j = -nO; j <= nO; j++) s += so[c + j];
        sums[1] = s;
    }
    __syncthreads();
    for (int j = -nD + (int)threadIdx.x; j <= nD; j += blockDim.x) sd[c + j] /= sums[0];
    for (int j = -nO + (int)threadIdx.x; j <= nO; j += blockDim.x) so[c + j] /= sums[1];
    __syncthreads();
    for (int j = -p.jcap + (int)threadIdx.x; j <= p.jcap; j += blockDim.x) {
        double acc = 0.0;
        if (j >= -hw && j <= hw) {
            const int i0 = max(-nO, j - nD), i1 = min(nO, j + nD);
            for (int i = i0; i <= i1; i++) acc += so[c + i] * sd[c + j - i];
        }
        O[c + j] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        od_hw[m] = hw;
        dfwhm[m] = def_fwhm(O + c - hw, 2 * hw + 1, hw, p.delta);
    }
}

// KS = (S (x) B) (x) T for seeing ise: ks row [2 nkcap + 1] (centre nkcap), scratch rows s / sb of the same length
__global__ void k_def_kernel(const double *seeings, DefDev p, double *ks, double *s, double *sb, int *ks_hw) {
    const int ise = blockIdx.x, L = 2 * p.nkcap + 1, c = p.nkcap;
    const double sigma = 1.035 / DEF_FWHM2SIGMA * seeings[ise];
    const int nS = (int)floor(4.0 * sigma / p.delta), nB = (int)ceil(p.F / 2 - 0.5), nT = (int)ceil(p.F) - 1;
    double *K = ks + (size_t)ise * L, *sS = s + (size_t)ise * L, *sSB = sb + (size_t)ise * L;
    __shared__ double sums[3];
    for (int j = -nS + (int)threadIdx.x; j <= nS; j += blockDim.x) {
        const double x = j * p.delta;
        sS[c + j] = exp(-(x * x) / (2.0 * sigma * sigma));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, t = 0.0;
        for (int j = -nS; j <= nS; j++) a += sS[c + j];
        for (int j = -nB; j <= nB; j++) b += fmax(0.0, fmin(j + 0.5, p.F / 2) - fmax(j - 0.5, -p.F / 2));
        for (int j = -nT; j <= nT; j++) t += 1.0 - fabs((double)j) / p.F;
        sums[0] = a; sums[1] = b; sums[2] = t;
    }
    __syncthreads();
    for (int j = -nS + (int)threadIdx.x; j <= nS; j += blockDim.x) sS[c + j] /= sums[0];
    __syncthreads();
    const int nSB = nS + nB, nK = nSB + nT;
    for (int j = -nSB + (int)threadIdx.x; j <= nSB; j += blockDim.x) {
        double acc = 0.0;
        for (int i = max(-nS, j - nB); i <= min(nS, j + nB); i++)
            acc += sS[c + i] * (fmax(0.0, fmin((j - i) + 0.5, p.F / 2) - fmax((j - i) - 0.5, -p.F / 2)) / sums[1]);
        sSB[c + j] = acc;
    }
    __syncthreads();
    for (int j = -p.nkcap + (int)threadIdx.x; j <= p.nkcap; j += blockDim.x) {
        double acc = 0.0;
        if (j >= -nK && j <= nK)
            for (int i = max(-nSB, j - nT); i <= min(nSB, j + nT); i++)
                acc += sSB[c + i] * ((1.0 - fabs((double)(j - i)) / p.F) / sums[2]);
        K[c + j] = acc;
    }
    if (threadIdx.x == 0) ks_hw[ise] = nK;
}

// one model per block: samp (nq doubles), validity, ofwhm / depth, and its 2S+1 columns (float32, rows of nbp)
__global__ void k_def_sample(const double *heights, const double *radii, const double *seeings, DefDev p, const double *od,
                             const int *od_hw, const double *ks, const int *ks_hw, double *samp, double *gridv, int *valid,
                             float *cols) {
    const int m = blockIdx.x, ir = m % p.n_r, ih = (m / p.n_r) % (p.n_h + 1), ise = m / (p.n_r * (p.n_h + 1));
    const int odm = ih * p.n_r + ir, hw = od_hw[odm], nk = ks_hw[ise], ns = 2 * p.S + 1;
    const double *O = od + (size_t)odm * (2 * p.jcap + 1) + p.jcap, *Kr = ks + (size_t)ise * (2 * p.nkcap + 1) + p.nkcap;
    double *sm = samp + (size_t)m * p.nq;
    float *col = cols + (size_t)m * ns * p.nbp;
    __shared__ double mean_s[129], inv_s[129];
    __shared__ int ok;
    double to, ti, rho;
    def_angles(p, heights, radii, ih, ir, &to, &ti, &rho);
    const double sigma = 1.035 / DEF_FWHM2SIGMA * seeings[ise];
    if (threadIdx.x == 0)
        ok = hw >= 0 && (to + rho) / p.pixscale + 4.0 * sigma / p.pixscale + 1.0 + p.S * p.step <= p.P - p.wing;
    for (int q = threadIdx.x; q < p.nq; q += blockDim.x) {
        double acc = 0.0;
        if (hw >= 0) {
            const int cq = (q - p.K - p.S) * p.ovs;
            for (int i = max(-hw, cq - nk); i <= min(hw, cq + nk); i++) acc += O[i] * Kr[cq - i];
        }
        sm[q] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        valid[m] = ok;
        if (hw < 0) {
            gridv[(size_t)m * 2] = NAN; gridv[(size_t)m * 2 + 1] = NAN;
        } else {
            const double *v = sm + p.S;
            double peak = v[0];
            for (int k = 1; k < p.nb; k++) peak = v[k] > peak ? v[k] : peak;
            gridv[(size_t)m * 2] = def_fwhm(v, p.nb, p.K, p.step * p.pixscale);
            gridv[(size_t)m * 2 + 1] = (peak - v[p.K]) / peak * 100.0;
        }
    }
    if ((int)threadIdx.x < ns) { // column s = threadIdx.x - S: t_k = samp[k - s + S]
        const double *t = sm + 2 * p.S - threadIdx.x;
        double sum = 0.0;
        for (int k = 0; k < p.nb; k++) sum += t[k];
        const double mean = sum / p.nb;
        double ss = 0.0;
        for (int k = 0; k < p.nb; k++) ss += (t[k] - mean) * (t[k] - mean);
        mean_s[threadIdx.x] = mean;
        inv_s[threadIdx.x] = ss > 0 ? sqrt(ss) : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ns * p.nbp; e += blockDim.x) {
        const int s = e / p.nbp, k = e % p.nbp;
        float v = 0.0f;
        if (ok && k < p.nb && inv_s[s] > 0) v = (float)((sm[2 * p.S - s + k] - mean_s[s]) / inv_s[s]);
        col[e] = v;
    }
}

// ---- fit ----
typedef float def_f32x16 __attribute__((ext_vector_type(16)));
#define DEF_BM 128
#define DEF_BN 128
#define DEF_BK 16
#define DEF_LDA (DEF_BM + 32) // the two k rows an MFMA operand read spans sit 32 banks apart

// scores c = V . cols^T for a tile of 128 trails x 128 columns; per (trail, group) the largest allowed max(c, 0) -> gmax
// (float bits, atomicMax: every value is >= 0).  slice[i]: -2 not fitted, -1 every seeing, else the one seeing slice.
__global__ void __launch_bounds__(256) k_def_gemm(const float *__restrict__ V, int n, const float *__restrict__ cols, DefDev p,
                                                  const int *__restrict__ slice, const int *__restrict__ valid, unsigned *gmax) {
    __shared__ float sA[DEF_BK][DEF_LDA], sB[DEF_BK][DEF_LDA];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int row0 = blockIdx.y * DEF_BM;
    const int64_t col0 = (int64_t)blockIdx.x * DEF_BN;
    const int lr = tid >> 1, lk = (tid & 1) * 8; // this thread's loads: row / column lr of the tile, k lk .. lk+7
    const bool arow = row0 + lr < n, brow = col0 + lr < p.ncol;
    const float4 *ga = (const float4 *)(V + (size_t)(row0 + lr) * p.nbp + lk);
    const float4 *gb = (const float4 *)(cols + (size_t)(col0 + lr) * p.nbp + lk);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ra0 = arow ? ga[0] : z4, ra1 = arow ? ga[1] : z4, rb0 = brow ? gb[0] : z4, rb1 = brow ? gb[1] : z4;
    def_f32x16 acc[2][2];
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    const int i = lane & 31, kh = lane >> 5;
    for (int k0 = 0; k0 < p.nbp; k0 += DEF_BK) {
        __syncthreads();
        sA[lk + 0][lr] = ra0.x; sA[lk + 1][lr] = ra0.y; sA[lk + 2][lr] = ra0.z; sA[lk + 3][lr] = ra0.w;
        sA[lk + 4][lr] = ra1.x; sA[lk + 5][lr] = ra1.y; sA[lk + 6][lr] = ra1.z; sA[lk + 7][lr] = ra1.w;
        sB[lk + 0][lr] = rb0.x; sB[lk + 1][lr] = rb0.y; sB[lk + 2][lr] = rb0.z; sB[lk + 3][lr] = rb0.w;
        sB[lk + 4][lr] = rb1.x; sB[lk + 5][lr] = rb1.y; sB[lk + 6][lr] = rb1.z; sB[lk + 7][lr] = rb1.w;
        __syncthreads();
        if (k0 + DEF_BK < p.nbp) { // the next tile's loads overlap this tile's products
            const int q = (k0 + DEF_BK) / 4;
            ra0 = arow ? ga[q] : z4; ra1 = arow ? ga[q + 1] : z4; rb0 = brow ? gb[q] : z4; rb1 = brow ? gb[q + 1] : z4;
        }
#pragma unroll
        for (int kk = 0; kk < DEF_BK; kk += 2) {
            const float a0 = sA[kk + kh][wm * 64 + i], a1 = sA[kk + kh][wm * 64 + 32 + i];
            const float b0 = sB[kk + kh][wn * 64 + i], b1 = sB[kk + kh][wn * 64 + 32 + i];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // epilogue: lane holds column (lane & 31) of each 32 x 32 tile, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int ns = 2 * p.S + 1, per_se = (p.n_h + 1) * p.n_r;
    for (int b = 0; b < 2; b++) {
        const int64_t col = col0 + wn * 64 + b * 32 + i;
        const bool cin = col < p.ncol;
        const int m = cin ? (int)(col / ns) : 0;
        const bool cval = cin && valid[m];
        const int ise = m / per_se;
        const int64_t g = col / p.group;
        for (int a = 0; a < 2; a++)
            for (int r = 0; r < 16; r++) {
                const int row = row0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int sl = row < n ? slice[row] : -2;
                const bool ok = cval && sl >= -1 && (sl == -1 || sl == ise);
                const float c = acc[a][b][r];
                unsigned x = ok && c > 0.0f ? __float_as_uint(c) : 0u;
                // segmented max over the 32 columns of this tile (groups are runs of consecutive columns)
                for (int d = 1; d < 32; d <<= 1) {
                    const unsigned y = __shfl_down(x, d, 32);
                    if (i + d < 32 && (col + d) / p.group == g) x = y > x ? y : x;
                }
                const bool head = i == 0 || (col - 1) / p.group != g;
                if (head && cin && x && row < n) atomicMax(&gmax[(size_t)row * p.n_groups + g], x);
            }
    }
}

// one trail per block (64 threads): the best group from gmax, the best column in it (scores recomputed as an fmaf chain over
// ascending k, as the matrix cores form them), its amplitude / offset / chi2 in double, and chi2 by height.
// res[i]: {column, a, b, chi2, |v~|^2}; cbh[i]: n_h + 1 doubles.
__global__ void k_def_pick(const float *V, const float *prof, const double *noise, const float *cols, const double *samp, DefDev p,
                           const int *slice, const int *valid, const int *gvalid, const unsigned *gmax, double *res, double *cbh) {
    const int t = blockIdx.x, sl = slice[t];
    const float *v = V + (size_t)t * p.nbp;
    const float *pr = prof + (size_t)t * p.nb;
    __shared__ unsigned long long keys[64];
    __shared__ int gbest;
    __shared__ double vn2;
    if (sl < -1) return;
    // the best group, lowest index on a tie: (score bits, complement of the group) keys, each lane over a stride of groups
    unsigned long long gk = 0;
    for (int g = threadIdx.x; g < p.n_groups; g += blockDim.x) {
        const unsigned x = gmax[(size_t)t * p.n_groups + g];
        const unsigned long long kk = x ? ((unsigned long long)x << 32) | (0xFFFFFFFFu - (unsigned)g) : 0ull;
        gk = kk > gk ? kk : gk;
    }
    keys[threadIdx.x] = gk;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < p.nb; k++) s += (double)v[k] * (double)v[k];
        vn2 = s;
        for (int j = 1; j < (int)blockDim.x; j++) gk = keys[j] > gk ? keys[j] : gk;
        gbest = gk ? (int)(0xFFFFFFFFu - (unsigned)(gk & 0xFFFFFFFFu)) : -1;
    }
    __syncthreads();
    const int ns = 2 * p.S + 1, per_se = (p.n_h + 1) * p.n_r;
    const double nz2 = noise[t] * noise[t];
    double *cb = cbh + (size_t)t * (p.n_h + 1);
    for (int ih = threadIdx.x; ih <= p.n_h; ih += blockDim.x) { // (|v~|^2 - m^2) / noise^2 over the allowed groups of height ih
        bool any = false;
        float mx = 0.0f;
        for (int ise = 0; ise < p.n_se; ise++) {
            if (sl >= 0 && ise != sl) continue;
            const int g = ise * (p.n_h + 1) + ih;
            if (!gvalid[g]) continue;
            any = true;
            const float x = __uint_as_float(gmax[(size_t)t * p.n_groups + g]);
            mx = x > mx ? x : mx;
        }
        cb[ih] = any ? (vn2 - (double)mx * (double)mx) / nz2 : NAN;
    }
    unsigned long long key = 0;
    if (gbest >= 0)
        for (int j = threadIdx.x; j < p.group; j += blockDim.x) {
            const int64_t col = (int64_t)gbest * p.group + j;
            const int m = (int)(col / ns);
            if (!valid[m] || (sl >= 0 && m / per_se != sl)) continue;
            const float *c = cols + (size_t)col * p.nbp;
            float acc = 0.0f;
            for (int k = 0; k < p.nbp; k++) acc = fmaf(v[k], c[k], acc);
            if (acc > 0.0f) {
                const unsigned long long kk = ((unsigned long long)__float_as_uint(acc) << 32) | (0xFFFFFFFFu - (unsigned)col);
                key = kk > key ? kk : key;
            }
        }
    __syncthreads();
    keys[threadIdx.x] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int j = 1; j < (int)blockDim.x; j++) key = keys[j] > key ? keys[j] : key;
    double *o = res + (size_t)t * 5;
    o[4] = vn2;
    if (!key) { o[0] = -1; o[1] = o[2] = o[3] = NAN; return; }
    const int64_t col = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu);
    const int m = (int)(col / ns), s = (int)(col % ns);
    const double *tm = samp + (size_t)m * p.nq + 2 * p.S - s;
    double sv = 0.0, st = 0.0;
    for (int k = 0; k < p.nb; k++) { sv += pr[k]; st += tm[k]; }
    const double vb = sv / p.nb, tb = st / p.nb;
    double sxy = 0.0, sxx = 0.0;
    for (int k = 0; k < p.nb; k++) { sxy += (pr[k] - vb) * (tm[k] - tb); sxx += (tm[k] - tb) * (tm[k] - tb); }
    const double a = sxy / sxx, b = vb - a * tb;
    double chi = 0.0;
    for (int k = 0; k < p.nb; k++) { const double r = pr[k] - a * tm[k] - b; chi += r * r; }
    o[0] = (double)col; o[1] = a; o[2] = b; o[3] = chi / nz2;
}
