// k_stars.h -- kernels of the source finder (include/lfdmi.h: source finder, steps 1 - 8).
//   k_stars_detect   one workgroup per 64 x 16 tile of a frame, halo sep + 1: validity test and byte swap as a pixel is loaded, h
//                    and S built separably in LDS, the window test on the few pixels with S >= T; one bit per pixel, a 64-bit
//                    word per tile row built by a ballot and stored by lane 0 (no atomic)
//   k_stars_rows     one workgroup per frame: popcount per row, exclusive scan over the rows (rs[y] = candidates above row y,
//                    rs[h] = n_found), the frame record
//   k_stars_measure  one workgroup per output slot: its row by bisection of the scan, its bit by a popcount walk; the
//                    (2 r_max + 3)^2 patch and its S in LDS; a wave per ring for the ring maxima; a lane per row for the sums
//                    of step 5, lane 0 adds them in ascending order
//   k_stars_catalog  a lane per catalogue row (step 8)
// The LDS rows have odd strides (83, 67 dwords): a column walk does not stay on one bank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define STR_THREADS 256
#define STR_TW 64                               // tile width = one word of the bit plane
#define STR_TH 16                               // tile height
#define STR_MAX_SEP 8
#define STR_HALO (STR_MAX_SEP + 1)
#define STR_LW (STR_TW + 2 * STR_HALO + 1)      // 83
#define STR_LH (STR_TH + 2 * STR_HALO)          // 34
#define STR_MAX_R 32                            // largest r_max
#define STR_PW (2 * STR_MAX_R + 3)              // 67: the patch a slot loads
#define STR_EXTENDED 1
#define STR_EDGE 2

typedef unsigned long long str_u64;

struct StarsDev {
    int h, w, be, sep, r_max, max_obj, wq;      // wq: 64-bit words per row of the bit plane
    double edge_frac;
};
struct StarsFrameDev {
    int status, n_found, n_out;
};
struct StarRec {
    int x, y, rad, flags;
    float s_peak, flux, xc, yc;
};

// a pixel as every step sees it: the byte-swapped value, 0 for a non-finite one
__device__ __forceinline__ float str_pixel(const uint32_t *src, size_t at, int be) {
    uint32_t bits = src[at];
    if (be) bits = __builtin_bswap32(bits);
    return (bits & 0x7F800000u) == 0x7F800000u ? 0.0f : __uint_as_float(bits);
}

__global__ __launch_bounds__(STR_THREADS) void k_stars_detect(const uint32_t *__restrict__ frames, size_t N, StarsDev p,
                                                              const float *__restrict__ thr, str_u64 *__restrict__ bits) {
    __shared__ float A[STR_LH * STR_LW];   // x, then S
    __shared__ float B[STR_LH * STR_LW];   // h
    const int f = blockIdx.z, R = p.sep + 1, LWu = STR_TW + 2 * R, LHu = STR_TH + 2 * R;
    const int tx0 = blockIdx.x * STR_TW, ty0 = blockIdx.y * STR_TH;
    const uint32_t *src = frames + (size_t)f * N;
    for (int idx = threadIdx.x; idx < LHu * LWu; idx += STR_THREADS) {
        const int ly = idx / LWu, lx = idx - ly * LWu, gy = ty0 - R + ly, gx = tx0 - R + lx;
        float v = 0.0f;
        if (gy >= 0 && gy < p.h && gx >= 0 && gx < p.w) v = str_pixel(src, (size_t)gy * p.w + gx, p.be);
        A[ly * STR_LW + lx] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < LHu * (LWu - 2); idx += STR_THREADS) {
        const int ly = idx / (LWu - 2), lx = idx - ly * (LWu - 2) + 1;
        const float *a = A + ly * STR_LW + lx;
        B[ly * STR_LW + lx] = (a[-1] + a[0]) + a[1];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (LHu - 2) * (LWu - 2); idx += STR_THREADS) {
        const int ly = idx / (LWu - 2) + 1, lx = idx - (ly - 1) * (LWu - 2) + 1;
        const float *b = B + ly * STR_LW + lx;
        A[ly * STR_LW + lx] = (b[-STR_LW] + b[0]) + b[STR_LW];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float T = thr[f];
    for (int r = wv; r < STR_TH; r += STR_THREADS / 64) {
        const int gy = ty0 + r, gx = tx0 + lane;
        if (gy >= p.h) break;   // (the same for every lane of the wave)
        bool cand = false;
        if (gx < p.w) {
            const float *s = A + (r + R) * STR_LW + lane + R;
            const float sp = s[0];
            if (sp >= T) {
                cand = true;
                const int dy0 = max(-p.sep, -gy), dy1 = min(p.sep, p.h - 1 - gy), dx0 = max(-p.sep, -gx), dx1 = min(p.sep, p.w - 1 - gx);
                for (int dy = dy0; dy <= dy1 && cand; dy++)
                    for (int dx = dx0; dx <= dx1; dx++) {
                        const float q = s[dy * STR_LW + dx];
                        const bool before = dy < 0 || (dy == 0 && dx < 0);
                        if (before ? !(sp > q) : ((dy | dx) != 0 && !(sp >= q))) { cand = false; break; }
                    }
            }
        }
        const str_u64 word = __ballot(cand);
        if (lane == 0) bits[((size_t)f * p.h + gy) * p.wq + blockIdx.x] = word;
    }
}

__global__ __launch_bounds__(STR_THREADS) void k_stars_rows(StarsDev p, const str_u64 *__restrict__ bits, int *__restrict__ rs,
                                                            StarsFrameDev *__restrict__ frec) {
    __shared__ int tot[STR_THREADS];
    const int f = blockIdx.x, per = (p.h + STR_THREADS - 1) / STR_THREADS;
    const int y0 = min((int)threadIdx.x * per, p.h), y1 = min(y0 + per, p.h);
    const str_u64 *bp = bits + (size_t)f * p.h * p.wq;
    int *out = rs + (size_t)f * (p.h + 1);
    int sum = 0;
    for (int y = y0; y < y1; y++) {
        int c = 0;
        for (int k = 0; k < p.wq; k++) c += __popcll(bp[(size_t)y * p.wq + k]);
        out[y] = c;
        sum += c;
    }
    tot[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int t = 0; t < STR_THREADS; t++) { const int c = tot[t]; tot[t] = acc; acc += c; }
        out[p.h] = acc;
        StarsFrameDev r;
        r.n_found = acc;
        r.n_out = min(acc, p.max_obj);
        r.status = acc > p.max_obj;
        frec[f] = r;
    }
    __syncthreads();
    int acc = tot[threadIdx.x];
    for (int y = y0; y < y1; y++) { const int c = out[y]; out[y] = acc; acc += c; }
}

__global__ __launch_bounds__(STR_THREADS) void k_stars_measure(const uint32_t *__restrict__ frames, size_t N, StarsDev p,
                                                               const float *__restrict__ efloor, const str_u64 *__restrict__ bits,
                                                               const int *__restrict__ rs, StarRec *__restrict__ recs) {
    __shared__ float X[STR_PW * STR_PW];
    __shared__ float S[STR_PW * STR_PW];
    __shared__ float M[STR_MAX_R + 1];
    __shared__ float rowa[2 * STR_MAX_R + 1], rowb[2 * STR_MAX_R + 1];
    __shared__ int pos[3];   // px, py, rad
    const int f = blockIdx.y, slot = blockIdx.x;
    const int *scan = rs + (size_t)f * (p.h + 1);
    if (slot >= min(scan[p.h], p.max_obj)) return;
    if (threadIdx.x == 0) {
        int lo = 0, hi = p.h - 1;   // the last row y with scan[y] <= slot
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (scan[mid] <= slot) lo = mid; else hi = mid - 1;
        }
        int k = slot - scan[lo], px = 0;
        const str_u64 *row = bits + ((size_t)f * p.h + lo) * p.wq;
        for (int wq = 0; wq < p.wq; wq++) {
            str_u64 wv = row[wq];
            const int c = __popcll(wv);
            if (k >= c) { k -= c; continue; }
            for (; k > 0; k--) wv &= wv - 1;
            px = (wq << 6) + __ffsll((long long)wv) - 1;
            break;
        }
        pos[0] = px; pos[1] = lo;
    }
    __syncthreads();
    const int px = pos[0], py = pos[1], R = p.r_max, PW = 2 * R + 3;
    const uint32_t *src = frames + (size_t)f * N;
    for (int idx = threadIdx.x; idx < PW * PW; idx += STR_THREADS) {
        const int ly = idx / PW, lx = idx - ly * PW, gy = py - R - 1 + ly, gx = px - R - 1 + lx;
        float v = 0.0f;
        if (gy >= 0 && gy < p.h && gx >= 0 && gx < p.w) v = str_pixel(src, (size_t)gy * p.w + gx, p.be);
        X[ly * STR_PW + lx] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < (PW - 2) * (PW - 2); idx += STR_THREADS) {
        const int ly = idx / (PW - 2) + 1, lx = idx - (ly - 1) * (PW - 2) + 1;
        const float *a = X + ly * STR_PW + lx;
        const float h0 = (a[-STR_PW - 1] + a[-STR_PW]) + a[-STR_PW + 1], h1 = (a[-1] + a[0]) + a[1], h2 = (a[STR_PW - 1] + a[STR_PW]) + a[STR_PW + 1];
        S[ly * STR_PW + lx] = (h0 + h1) + h2;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, C = (R + 1) * STR_PW + R + 1;   // C: the peak's place in the patch
    for (int r = 1 + wv; r <= R; r += STR_THREADS / 64) {
        float m = -INFINITY;
        for (int i = lane; i < 8 * r; i += 64) {
            const int side = i / (2 * r), j = i - side * 2 * r;
            const int dy = side == 0 ? -r : side == 1 ? -r + j : side == 2 ? r : r - j;
            const int dx = side == 0 ? -r + j : side == 1 ? r : side == 2 ? r - j : -r;
            const int gy = py + dy, gx = px + dx;
            if (gy >= 0 && gy < p.h && gx >= 0 && gx < p.w) m = fmaxf(m, S[C + dy * STR_PW + dx]);
        }
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) M[r] = m;
    }
    __syncthreads();
    const float sp = S[C];
    if (threadIdx.x == 0) {
        const float E = fmaxf((float)(p.edge_frac * (double)sp), efloor[f]);
        int rad = 0;
        for (int r = 1; r <= R; r++)
            if (M[r] < E) { rad = r; break; }
        pos[2] = rad;
    }
    __syncthreads();
    const int rad = pos[2];
    const int dx0 = max(-rad, -px), dx1 = min(rad, p.w - 1 - px), dy0 = max(-rad, -py), dy1 = min(rad, p.h - 1 - py);
    if ((int)threadIdx.x <= dy1 - dy0) {
        const int dy = dy0 + (int)threadIdx.x;
        const float *a = X + C + dy * STR_PW;
        float sa = 0.0f, sb = 0.0f;
        for (int dx = dx0; dx <= dx1; dx++) {
            const float v = a[dx];
            sa = sa + v;
            sb = sb + v * (float)dx;
        }
        rowa[threadIdx.x] = sa;
        rowb[threadIdx.x] = sb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double F = 0.0, MX = 0.0, MY = 0.0;
        for (int k = 0; k <= dy1 - dy0; k++) {
            F = F + (double)rowa[k];
            MX = MX + (double)rowb[k];
            MY = MY + (double)(dy0 + k) * (double)rowa[k];
        }
        StarRec o;
        o.x = px; o.y = py; o.rad = rad;
        o.flags = (rad == 0 ? STR_EXTENDED : 0) | ((dx0 != -rad || dx1 != rad || dy0 != -rad || dy1 != rad) ? STR_EDGE : 0);
        o.s_peak = sp;
        o.flux = (float)F;
        o.xc = F > 0.0 ? (float)((double)px + MX / F) : (float)px;
        o.yc = F > 0.0 ? (float)((double)py + MY / F) : (float)py;
        recs[(size_t)f * p.max_obj + slot] = o;
    }
}

// step 8: row i of frame f (count[f] = n_out rows carry a source; the rest are zero but for ndetect = 1)
__global__ __launch_bounds__(STR_THREADS) void k_stars_catalog(const StarRec *__restrict__ recs, const int *__restrict__ n_out, int max_obj,
                                                               double pixscale, int *__restrict__ count, float *__restrict__ rowc,
                                                               float *__restrict__ colc, float *__restrict__ psfmag, float *__restrict__ petro90,
                                                               int *__restrict__ nobserve, int *__restrict__ ndetect) {
    const int f = blockIdx.y, i = blockIdx.x * STR_THREADS + threadIdx.x;
    if (i >= max_obj) return;
    const int cnt = min(n_out[f], max_obj);
    if (i == 0) count[f] = cnt;
    const size_t o1 = (size_t)f * max_obj + i, o5 = o1 * 5;
    float r = 0.0f, c = 0.0f, pet = 0.0f;
    int nob = 0;
    if (i < cnt) {
        const StarRec s = recs[o1];
        r = (float)s.x; c = (float)s.y;
        pet = (float)((double)s.rad * pixscale);
        nob = (s.flags & STR_EXTENDED) ? 0 : 1;
    }
    for (int k = 0; k < 5; k++) {
        rowc[o5 + k] = r; colc[o5 + k] = c; psfmag[o5 + k] = 0.0f; petro90[o5 + k] = pet;
    }
    nobserve[o1] = nob;
    ndetect[o1] = 1;   // (the padding too: nobserve != ndetect, as catalogs.empty_packed has it)
}
