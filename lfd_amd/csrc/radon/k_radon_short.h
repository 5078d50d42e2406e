// k_radon_short.h -- the short-trail search's own kernel (include/lfdmi.h: faint-trail search, steps 10 - 12; host side in
// radon.hip).  The candidates are scored where they are stored, by k_radon_level<4, false, true> of k_radon.h; the extent and
// the peel of a round are k_radon_extent and k_radon_peel of k_radon_lines.h on the candidate's parent line.
//   k_radon_short_finish   one workgroup per frame: the best of the scoring levels' partial records, ties to the lowest
//                          (L, q, j, s, y), and its parent line (step 11) by the dyadic path on the device
#pragma once
#include "k_radon.h"
#include "k_radon_lines.h"

#define RADS_MAX_LEVELS 32   // scored (orientation pair, level) entries at most: L = 64 .. 32768 in each of two pairs

// where the scoring levels of a round put their partial records: entry e is level L[e] of orientation pair o[e], whose grid
// has cnt[e] workgroups per orientation; a frame's records are total long, entry e's start at off[e] (q even, then q odd)
struct RadonShortDev {
    int ne;
    int L[RADS_MAX_LEVELS], o[RADS_MAX_LEVELS], cnt[RADS_MAX_LEVELS];
    long long off[RADS_MAX_LEVELS];
    long long total;
};
struct RadonShortRec {
    int status, q, y0, s, n_pix;    // (q, y0, s): the parent line
    float sum, snr;
    int level, strip, ys, ss;       // the candidate: (L, j, y, s)
    int pad;
};
struct RadonShortBest {
    float snr, sum;
    int s, y, n, j, L, q;
};

// is candidate a better than b?  larger snr; ties to the lowest (L, q, j, s, y)
__device__ __forceinline__ bool rad_short_better(const RadonShortBest &a, const RadonShortBest &b) {
    if (a.snr != b.snr) return a.snr > b.snr;
    if (a.L != b.L) return a.L < b.L;
    if (a.q != b.q) return a.q < b.q;
    if (a.j != b.j) return a.j < b.j;
    if (a.s != b.s) return a.s < b.s;
    return a.y < b.y;
}

__global__ __launch_bounds__(RAD_THREADS) void k_radon_short_finish(const RadonShortPart *__restrict__ spart, RadonDev p, RadonShortDev d,
                                                                    RadonShortRec *__restrict__ rec) {
    __shared__ RadonShortBest red[RAD_THREADS];
    const int tid = threadIdx.x, f = blockIdx.x;
    RadonShortBest b;
    b.snr = 0.0f; b.sum = 0.0f; b.s = 0; b.y = 0; b.n = -1; b.j = 0; b.L = 0; b.q = 0;
    for (int e = 0; e < d.ne; e++) {
        const RadonShortPart *pe = spart + (size_t)f * d.total + d.off[e];
        const int cnt = d.cnt[e];
        for (int i = tid; i < 2 * cnt; i += RAD_THREADS) {
            const RadonShortPart x = pe[i];
            if (x.n < 0) continue;
            RadonShortBest c;
            c.snr = x.snr; c.sum = x.sum; c.s = x.s; c.y = x.y; c.n = x.n; c.j = x.j; c.L = d.L[e]; c.q = 2 * d.o[e] + (i >= cnt);
            if (b.n < 0 || rad_short_better(c, b)) b = c;
        }
    }
    red[tid] = b;
    __syncthreads();
    for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const RadonShortBest x = red[tid + w], m = red[tid];
            if (x.n >= 0 && (m.n < 0 || rad_short_better(x, m))) red[tid] = x;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const RadonShortBest x = red[0];
        RadonShortRec r;
        r.pad = 0;
        if (x.n < 0) {
            r.status = 1; r.q = 0; r.y0 = 0; r.s = 0; r.n_pix = 0; r.sum = 0.0f; r.snr = 0.0f;
            r.level = 0; r.strip = 0; r.ys = 0; r.ss = 0;
        } else {
            // step 11: the full line whose path over strip j is the candidate's
            const int P = p.P[x.q >> 1], sp = x.s * (P / x.L);
            r.status = 0; r.q = x.q; r.s = sp; r.y0 = x.y - rad_path(x.j * x.L, sp, P);
            r.n_pix = x.n; r.sum = x.sum; r.snr = x.snr;
            r.level = x.L; r.strip = x.j; r.ys = x.y; r.ss = x.s;
        }
        rec[f] = r;
    }
}
