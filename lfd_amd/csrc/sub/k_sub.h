// k_sub.h -- device side of the trail subtraction (include/lfdmi.h: trail subtraction).  The cells come from the trail strips'
// own kernels (../strip/k_strip.h: k_strip_cull, k_strip_render) and never leave the device; two kernels follow them.
// k_sub_model turns a segment's cells into its float table: section backgrounds, cell excesses and the running median along the
// trail, all in int64, then one conversion per cell.  k_sub_render walks the (job, tile) list the strips' cull made (the same
// band, so the same tiles), interpolates every segment's table at the pixel centres and subtracts, segments in ascending index.
// Every count and every q_removed is an integer sum and the peak an integer maximum: nothing depends on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../strip/k_strip.h"   // (its kernels have internal linkage: this unit launches its own copies)

#define SUB_THREADS 256
#define SUB_WAVES (SUB_THREADS / 64)
#define SUB_ROWS 16                                        // sections of a segment a block of k_sub_model owns
#define SUB_MAX_R 8                                        // largest half-window of the running median
#define SUB_WIN (2 * SUB_MAX_R + 1)                        // values a cell's median holds at most
#define SUB_HALO (SUB_ROWS + 2 * SUB_MAX_R)                // rows of excesses a block keeps in LDS
#define SUB_ABSENT 0x7fffffffffffffffll                    // an absent excess (|X| < 2^42: no excess has this value); sorts last

// what the segment's kernels add to StripSeg
struct SubSeg {
    int32_t kw;                 // bin b is a wing bin iff |b - K| >= kw (step 2, decided on the host)
    int32_t K;
};

// the device's part of a record
struct SubStat {
    int32_t n_usable, n_model, n_pix, pad;
    unsigned long long q_removed;   // (two's complement: the sum of signed values)
    unsigned long long peak;        // sub_peak_key of the largest m; 0: no model cell
};

struct SubModelDev {
    int32_t R, min_sec, min_n, min_wing;
};

// a float as an unsigned integer of the same order (no NaN comes here), above the cell's index complemented: the maximum of the
// keys is the largest m, among equals the lowest cell j * n_off + b, which is the lowest j and then the lowest b
__device__ __forceinline__ unsigned long long sub_peak_key(float m, uint32_t cell) {
    const uint32_t b = __float_as_uint(m);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(~cell);
}

// One block per (segment, run of SUB_ROWS sections): blockIdx.x is the segment of the chunk, blockIdx.y the run.  Steps 2 to 4
// of the definition.  (a) a wave per row of the run and its halo of R rows on either side: the wing bins' n and q summed over
// the lanes, B = Q / N.  (b) a thread per cell of those rows: the excess q / n - B, or SUB_ABSENT, into LDS.  (c) a thread per
// cell of the run: the at most 2R + 1 values of its column in registers, the two middle ones found by rank (a value's rank is
// the number of values below it, equal ones in row order; absent ones rank last), the table entry, n_model and the peak.
// Integer division only; every loop that holds a barrier or a shuffle is uniform over the wave that runs it.
__global__ void __launch_bounds__(SUB_THREADS) k_sub_model(const StripSeg *segs, const SubSeg *sub, const StripCell *cells, SubModelDev p,
                                                            float *table, SubStat *stat) {
    __shared__ long long X[SUB_HALO * STRIP_TAB_B];
    __shared__ long long B[SUB_HALO];
    __shared__ int usable[SUB_HALO];
    __shared__ int s_model, s_usable;
    __shared__ unsigned long long s_peak;
    const StripSeg s = segs[blockIdx.x];
    const int ja = (int)blockIdx.y * SUB_ROWS;
    if (ja >= s.n_sec) return;                              // (the whole block)
    const int jz = min(ja + SUB_ROWS, s.n_sec);             // its rows [ja, jz)
    const int ra = max(ja - p.R, 0), rz = min(jz + p.R, s.n_sec);   // with the halo [ra, rz)
    const int nrows = rz - ra, noff = s.n_off;
    const int K = sub[blockIdx.x].K, kw = sub[blockIdx.x].kw;
    const StripCell *c = cells + s.base;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_model = 0; s_usable = 0; s_peak = 0ull; }
    // (a)
    for (int r = wave; r < nrows; r += SUB_WAVES) {
        int N = 0;
        long long Q = 0ll;
        for (int b = lane; b < noff; b += 64)
            if (abs(b - K) >= kw) {
                const StripCell v = c[(int64_t)(ra + r) * noff + b];
                N += v.n;
                Q += (long long)v.q;
            }
        for (int d = 32; d > 0; d >>= 1) {
            N += __shfl_down(N, d, 64);
            Q += __shfl_down(Q, d, 64);
        }
        if (lane == 0) {
            const int ok = N >= p.min_wing;
            usable[r] = ok;
            B[r] = ok ? Q / (long long)N : 0ll;
        }
    }
    __syncthreads();
    // (b)
    for (int e = tid; e < nrows * noff; e += SUB_THREADS) {
        const int r = e / noff, b = e - r * noff;
        long long x = SUB_ABSENT;
        if (usable[r] && abs(b - K) < kw) {
            const StripCell v = c[(int64_t)(ra + r) * noff + b];
            if (v.n >= p.min_n) x = (long long)v.q / (long long)v.n - B[r];
        }
        X[r * STRIP_TAB_B + b] = x;
    }
    __syncthreads();
    // (c)
    int my_model = 0, my_usable = 0;
    unsigned long long my_peak = 0ull;
    for (int r = ja - ra + tid; r < jz - ra; r += SUB_THREADS) my_usable += usable[r];
    for (int e = tid; e < (jz - ja) * noff; e += SUB_THREADS) {
        const int rj = e / noff, b = e - rj * noff, j = ja + rj;
        float m = 0.0f;
        if (abs(b - K) < kw) {
            const int wa = max(j - p.R, 0) - ra, wz = min(j + p.R, s.n_sec - 1) - ra;   // the window's rows [wa, wz] of X
            long long x[SUB_WIN];
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < SUB_WIN; k++) {
                x[k] = wa + k <= wz ? X[(wa + k) * STRIP_TAB_B + b] : SUB_ABSENT;
                cnt += x[k] != SUB_ABSENT;
            }
            if (cnt >= p.min_sec) {
                const int lo_rank = (cnt - 1) >> 1, hi_rank = cnt >> 1;   // (equal when cnt is odd)
                long long lo = 0ll, hi = 0ll;
#pragma unroll
                for (int k = 0; k < SUB_WIN; k++) {
                    int rank = 0;
#pragma unroll
                    for (int l = 0; l < SUB_WIN; l++) rank += (x[l] < x[k]) || (x[l] == x[k] && l < k);
                    if (rank == lo_rank) lo = x[k];
                    if (rank == hi_rank) hi = x[k];
                }
                const long long M = lo + (hi - lo) / 2;
                m = (float)((double)M * 9.313225746154785e-10);   // 2^-30: exact conversion, exact product, one rounding
                my_model++;
                const unsigned long long key = sub_peak_key(m, (uint32_t)(j * noff + b));
                my_peak = key > my_peak ? key : my_peak;
            }
        }
        table[s.base + (int64_t)j * noff + b] = m;
    }
    if (my_model) atomicAdd(&s_model, my_model);
    if (my_peak) atomicMax(&s_peak, my_peak);
    if (my_usable) atomicAdd(&s_usable, my_usable);
    __syncthreads();
    if (tid == 0) {   // one global atomic per block and result
        if (s_usable) atomicAdd(&stat[blockIdx.x].n_usable, s_usable);
        if (s_model) {
            atomicAdd(&stat[blockIdx.x].n_model, s_model);
            atomicMax(&stat[blockIdx.x].peak, s_peak);
        }
    }
}

struct SubDev {
    int32_t h, w, ntx, nty;     // the frame and its tile grid
    int32_t be;                 // frames are big-endian (apply == 0 only)
    int32_t apply;              // 0: count, write no pixel
    int32_t vec;                // w % 4 == 0 and the frame buffer is 16-byte aligned: a thread's pixels are one load and one store
    int32_t pad;
};

// Persistent blocks walk the list of k_strip_cull.  A block owns a tile and a thread its STRIP_PX pixels, as in k_strip_render;
// the pixels stay in registers while the job's segments pass through LDS in chunks of STRIP_CHUNK, in ascending index, each
// with the block's verdict on whether it can reach the tile.  Step 5 of the definition per (pixel, segment): u, t, a, g in
// double, four reads of the segment's table (they come through L2: a tile touches at most 18 x 131 entries of it), the
// interpolation in float32 with every operation rounded on its own, one subtraction.  Whether a pixel takes part is decided on
// its value as passed, so a crossing changes no verdict.  n_pix and q_removed leave as one integer atomicAdd per wave and
// segment.  q_removed's terms come from strip_fix, which k_strip.h documents for |v| <= 1024 (e <= 137): here |v| can reach
// 2048 (excesses of +-2^41 at clip 1024, and the interpolation stays within a few ulp of its nodes), e <= 139, a shift of at
// most 19 on a 24-bit mantissa: below 2^43, checked for this use.  The image sees no atomic: a thread writes its own pixels
// once, after the last segment, and only those that changed.
__global__ void __launch_bounds__(SUB_THREADS) k_sub_render(uint32_t *frames, const StripJob *jobs, const StripSeg *segs, const float *table,
                                                             SubDev p, const int2 *list, const int *count, SubStat *stat) {
    __shared__ StripSeg S[STRIP_CHUNK];
    __shared__ int hit[STRIP_CHUNK];
    const int n = *count;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int col = (tid % STRIP_COLS) * STRIP_PX, row = tid / STRIP_COLS;
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int2 e = list[item];
        const StripJob jb = jobs[e.x];
        StripDev geo;
        geo.h = p.h; geo.w = p.w; geo.ntx = p.ntx; geo.nty = p.nty;
        int x0, x1, r0, r1;
        strip_tile_box(geo, e.y, x0, x1, r0, r1);
        const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
        const int x = x0 + col, r = r0 + row;
        const double yd = (double)(p.h - 1 - r);
        const size_t px = (size_t)r * p.w + x;
        const bool whole = r <= r1 && x + STRIP_PX - 1 <= x1 && p.vec;
        bool live[STRIP_PX], changed[STRIP_PX];
        float val[STRIP_PX];
        {
            uint32_t b[STRIP_PX] = {0u, 0u, 0u, 0u};
            if (whole) {
                const uint4 v = *(const uint4 *)(frames + jb.foff + px);
                b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
            } else {
#pragma unroll
                for (int m = 0; m < STRIP_PX; m++)
                    if (r <= r1 && x + m <= x1) b[m] = frames[jb.foff + px + m];
            }
#pragma unroll
            for (int m = 0; m < STRIP_PX; m++) {
                const uint32_t bits = p.be ? __builtin_bswap32(b[m]) : b[m];
                const uint32_t mag = bits & 0x7fffffffu;
                live[m] = r <= r1 && x + m <= x1 && mag != 0u && mag < 0x7f800000u;   // in the frame, not +-0, finite
                changed[m] = false;
                val[m] = __uint_as_float(bits);
            }
        }
        for (int c0 = jb.sb; c0 < jb.se; c0 += STRIP_CHUNK) {
            const int nc = min(STRIP_CHUNK, jb.se - c0);
            __syncthreads();   // (the chunk before, or the item before, has been read)
            if (tid < nc) {
                const StripSeg s = segs[c0 + tid];
                double tlo, thi, ulo, uhi;
                S[tid] = s;
                hit[tid] = strip_box_hit(s, (double)x0, (double)x1, ya, yb, &tlo, &thi, &ulo, &uhi);
            }
            __syncthreads();
            for (int k = 0; k < nc; k++) {
                if (!hit[k]) continue;   // (the same for the whole block)
                const int nsec = S[k].n_sec, noff = S[k].n_off;
                const float *T = table + S[k].base;
                const double Kd = S[k].kc - 0.5;   // (K + 0.5 and K are both exact)
                int cnt = 0;
                long long qs = 0ll;
#pragma unroll
                for (int m = 0; m < STRIP_PX; m++) {
                    const double ax = (double)(x + m) - S[k].x1, ay = yd - S[k].y1;
                    const double u = ax * S[k].nx + ay * S[k].ny;
                    const double t = ax * S[k].ex + ay * S[k].ey;
                    if (!(live[m] && t >= 0.0 && t <= S[k].L && fabs(u) <= S[k].half)) continue;
                    const double a = t * S[k].inv_s - 0.5, g = u * S[k].inv_u + Kd;
                    const int j0 = min(max((int)floor(a), 0), nsec - 1), j1 = min(j0 + 1, nsec - 1);
                    const int b0 = min(max((int)floor(g), 0), noff - 1), b1 = min(b0 + 1, noff - 1);
                    const float ft = (float)fmin(fmax(a - (double)j0, 0.0), 1.0);
                    const float fb = (float)fmin(fmax(g - (double)b0, 0.0), 1.0);
                    const float m00 = T[(int64_t)j0 * noff + b0], m01 = T[(int64_t)j0 * noff + b1];
                    const float m10 = T[(int64_t)j1 * noff + b0], m11 = T[(int64_t)j1 * noff + b1];
                    const float v0 = __fadd_rn(m00, __fmul_rn(fb, __fsub_rn(m01, m00)));
                    const float v1 = __fadd_rn(m10, __fmul_rn(fb, __fsub_rn(m11, m10)));
                    const float v = __fadd_rn(v0, __fmul_rn(ft, __fsub_rn(v1, v0)));
                    if (v != 0.0f) {
                        val[m] = __fsub_rn(val[m], v);
                        changed[m] = true;
                        cnt++;
                        qs += strip_fix(__float_as_uint(v));
                    }
                }
                for (int d = 32; d > 0; d >>= 1) {
                    cnt += __shfl_down(cnt, d, 64);
                    qs += __shfl_down(qs, d, 64);
                }
                if (lane == 0 && cnt) {
                    SubStat *o = stat + (c0 + k);
                    atomicAdd(&o->n_pix, cnt);
                    if (qs) atomicAdd(&o->q_removed, (unsigned long long)qs);
                }
            }
        }
        if (p.apply) {
            if (whole && changed[0] && changed[1] && changed[2] && changed[3]) {
                *(uint4 *)(frames + jb.foff + px) =
                    make_uint4(__float_as_uint(val[0]), __float_as_uint(val[1]), __float_as_uint(val[2]), __float_as_uint(val[3]));
            } else {
#pragma unroll
                for (int m = 0; m < STRIP_PX; m++)
                    if (changed[m]) frames[jb.foff + px + m] = __float_as_uint(val[m]);
            }
        }
    }
}
