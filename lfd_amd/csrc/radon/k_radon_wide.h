// k_radon_wide.h -- the wide-trail search's own kernels (include/lfdmi.h: faint-trail search, steps 13 - 16; host side in
// radon.hip).  The last level is stored by the non-scoring k_radon_level of k_radon.h as one plane [y][s] per orientation; the
// extent and the peel of a round are k_radon_extent and k_radon_peel of k_radon_lines.h with the band's width.
//   k_radon_wide          a workgroup takes RADW_Y rows x RADW_S slopes of that plane and max_width - 1 halo rows above them
//                         into LDS (a wave's loads run along s: contiguous), the counts widened to 32 bits; every width
//                         1, 2, 4, .. is scored as the in-place doubling B_2k[y] = B_k[y] + B_k[y + k] makes it.  A lane owns one
//                         slope and meets its entries in ascending (k, y), so a strict comparison keeps the lowest of equal
//                         scores; the width-1 best, which is the plain search's, is kept beside the overall one.  Two partial
//                         records per workgroup, plain stores
//   k_radon_wide_finish   one workgroup per frame: the best band, ties to the lowest (k, q, s, y), and the best line of
//                         width 1, ties to the lowest (q, s, y), of the partial records; no atomics
#pragma once
#include "k_radon.h"

#define RADW_MAXW 16     // LFDMI_RADON_MAX_WIDTH
#define RADW_Y 64        // rows of entries per workgroup
#define RADW_S 64        // slopes per workgroup (P of a small frame if that is less)
#define RADW_ROWS (RADW_Y + RADW_MAXW - 1)
#define RADW_IT ((RADW_ROWS + RAD_THREADS / RADW_S - 1) / (RAD_THREADS / RADW_S))   // rows a lane owns at most

struct RadonWidePart {
    float snr, sum;
    int s, y, n, k;         // n < 0: no candidate
};
struct RadonWideRec {
    int status, q, y0, s, n_pix;
    float sum, snr;
    int k;
};

// is band a better than b?  larger snr; ties to the lowest (k, q, s, y)
__device__ __forceinline__ bool rad_wide_better(float sa, int ka, int qa, int ssa, int ya, float sb, int kb, int qb, int ssb, int yb) {
    const bool lower = ka < kb || (ka == kb && (qa < qb || (qa == qb && (ssa < ssb || (ssa == ssb && ya < yb)))));
    return sa > sb || (sa == sb && lower);
}

// the best of red[0 .. RAD_THREADS - 1] under the tie rule into red[0] (q is the workgroup's: it does not take part)
__device__ __forceinline__ void rad_wide_reduce(RadonWidePart *red, int tid) {
    __syncthreads();
    for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const RadonWidePart x = red[tid + w], m = red[tid];
            if (x.n >= 0 && (m.n < 0 || rad_wide_better(x.snr, x.k, 0, x.s, x.y, m.snr, m.k, 0, m.s, m.y))) red[tid] = x;
        }
        __syncthreads();
    }
}

// S, N: the plane set that holds the last level of orientation pair o (grid.z = frame * 2 + (q & 1)); grid.x = the plane's
// R + P - 1 rows in blocks of RADW_Y, grid.y = its P slopes in blocks of min(RADW_S, P).  wpart: 2 records per workgroup (the
// best band, the best of width 1) at ((f * 4 + q) * wstride + blockIdx.x * gridDim.y + blockIdx.y) * 2.
__global__ __launch_bounds__(RAD_THREADS) void k_radon_wide(const float *__restrict__ S, const uint16_t *__restrict__ N, RadonDev p, int o,
                                                            int maxw, const float *__restrict__ sigma, RadonWidePart *__restrict__ wpart,
                                                            int wstride) {
    __shared__ float lb[RADW_ROWS * RADW_S];
    __shared__ int lc[RADW_ROWS * RADW_S];
    __shared__ RadonWidePart red[RAD_THREADS];
    const int tid = threadIdx.x, q = 2 * o + (blockIdx.z & 1), f = blockIdx.z >> 1;
    const int R = p.R[o], P = p.P[o], RP = R + P - 1;
    const int ws = min(RADW_S, P), rpp = RAD_THREADS / ws;      // (powers of two: a lane keeps its slope from pass to pass)
    const int sl = tid % ws, r0 = tid / ws, s = (int)blockIdx.y * ws + sl;
    const int yi0 = (int)blockIdx.x * RADW_Y;                   // row yi of the plane is y = yi - (P - 1)
    const int nrows = RADW_Y + maxw - 1, nout = min(RADW_Y, RP - yi0);
    const size_t base = (size_t)f * p.frame_elems + p.off[q] + (size_t)s;
    for (int row = r0; row < nrows; row += rpp) {
        const int yi = yi0 + row;
        float v = 0.0f;
        int m = 0;
        if (yi < RP) {                                          // (a row above R - 1 reads +0 / 0)
            const size_t a = base + (size_t)yi * P;
            v = S[a];
            m = N[a];
        }
        lb[row * ws + sl] = v;
        lc[row * ws + sl] = m;
    }
    __syncthreads();
    const float sg = sigma[f];
    float bs = 0.0f, bsum = 0.0f, ps = 0.0f, psum = 0.0f;
    int by = 0, bn = -1, bk = 0, py = 0, pn = -1;
    for (int k = 1;; k *= 2) {
        const long long need = (long long)k * p.min_len;
        for (int row = r0; row < nout; row += rpp) {            // a lane scores only what it wrote itself
            const int c = lc[row * ws + sl];
            if (c < need) continue;
            const float b = lb[row * ws + sl];
            const float snr = __fdiv_rn(b, __fmul_rn(sg, sqrtf((float)c)));
            const bool take = bn < 0 || snr > bs;
            bs = take ? snr : bs; bsum = take ? b : bsum; by = take ? yi0 + row - (P - 1) : by; bn = take ? c : bn; bk = take ? k : bk;
        }
        if (k == 1) { ps = bs; psum = bsum; py = by; pn = bn; }
        if (2 * k > maxw) break;
        // B_2k, C_2k of the rows whose 2k lines are all in the tile, in place: read, barrier, write
        const int lim = nrows - (2 * k - 1);
        float tv[RADW_IT];
        int tn[RADW_IT];
#pragma unroll
        for (int it = 0; it < RADW_IT; it++) {
            const int row = r0 + it * rpp;
            tv[it] = 0.0f; tn[it] = 0;
            if (row < lim) {
                tv[it] = lb[row * ws + sl] + lb[(row + k) * ws + sl];
                tn[it] = lc[row * ws + sl] + lc[(row + k) * ws + sl];
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RADW_IT; it++) {
            const int row = r0 + it * rpp;
            if (row < lim) {
                lb[row * ws + sl] = tv[it];
                lc[row * ws + sl] = tn[it];
            }
        }
        __syncthreads();
    }
    RadonWidePart *out = wpart + (((size_t)f * 4 + q) * wstride + (size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2;
    red[tid].snr = bs; red[tid].sum = bsum; red[tid].s = s; red[tid].y = by; red[tid].n = bn; red[tid].k = bk;
    rad_wide_reduce(red, tid);
    if (tid == 0) out[0] = red[0];
    __syncthreads();
    red[tid].snr = ps; red[tid].sum = psum; red[tid].s = s; red[tid].y = py; red[tid].n = pn; red[tid].k = 1;
    rad_wide_reduce(red, tid);
    if (tid == 0) out[1] = red[0];
}

// np0 / np1: workgroups of k_radon_wide per orientation of {0, 1} / {2, 3}.  rec: the plain search's record of the frame
// (k_radon_finish's), wrec: its band
__global__ __launch_bounds__(RAD_THREADS) void k_radon_wide_finish(const RadonWidePart *__restrict__ wpart, int wstride, int np0, int np1,
                                                                   RadonWideRec *__restrict__ wrec, RadonRec *__restrict__ rec) {
    __shared__ RadonWidePart red[RAD_THREADS];
    __shared__ int rq[RAD_THREADS];
    const int tid = threadIdx.x, f = blockIdx.x;
    for (int which = 0; which < 2; which++) {       // 0: the band (ties to the lowest (k, q, s, y)), 1: width 1 (k is 1 throughout)
        RadonWidePart b;
        b.snr = 0.0f; b.sum = 0.0f; b.s = 0; b.y = 0; b.n = -1; b.k = 0;
        int bq = 0;
        for (int q = 0; q < 4; q++) {
            const int np = q < 2 ? np0 : np1;
            const RadonWidePart *pq = wpart + ((size_t)f * 4 + q) * wstride * 2 + which;
            for (int i = tid; i < np; i += RAD_THREADS) {
                const RadonWidePart x = pq[2 * i];
                if (x.n >= 0 && (b.n < 0 || rad_wide_better(x.snr, x.k, q, x.s, x.y, b.snr, b.k, bq, b.s, b.y))) { b = x; bq = q; }
            }
        }
        __syncthreads();
        red[tid] = b;
        rq[tid] = bq;
        __syncthreads();
        for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const RadonWidePart x = red[tid + w], m = red[tid];
                if (x.n >= 0 && (m.n < 0 || rad_wide_better(x.snr, x.k, rq[tid + w], x.s, x.y, m.snr, m.k, rq[tid], m.s, m.y))) {
                    red[tid] = x;
                    rq[tid] = rq[tid + w];
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const RadonWidePart x = red[0];
            const bool none = x.n < 0;
            if (which == 0) {
                RadonWideRec r;
                r.status = none ? 1 : 0; r.q = none ? 0 : rq[0]; r.y0 = none ? 0 : x.y; r.s = none ? 0 : x.s; r.n_pix = none ? 0 : x.n;
                r.sum = none ? 0.0f : x.sum; r.snr = none ? 0.0f : x.snr; r.k = none ? 0 : x.k;
                wrec[f] = r;
            } else {
                RadonRec r;
                r.pad = 0;
                r.status = none ? 1 : 0; r.q = none ? 0 : rq[0]; r.y0 = none ? 0 : x.y; r.s = none ? 0 : x.s; r.n_pix = none ? 0 : x.n;
                r.sum = none ? 0.0f : x.sum; r.snr = none ? 0.0f : x.snr;
                rec[f] = r;
            }
        }
    }
}
