// k_radon_lines.h -- kernels of the several-lines search (include/lfdmi.h: faint-trail search, steps 7 - 9; host side in
// radon.hip).  The rounds themselves run k_radon_first .. k_radon_finish of k_radon.h unchanged.
//   k_radon_extent   one workgroup per found line: gathers the line's cells along its dyadic path, one lane makes the sequential
//                    float32 prefix through LDS tiles into the handle's prefix arrays, then the workgroup scores every interval
//                    (c1, c2) -- about C * C / 2 scores per line, C = 1024 / 745 for an SDSS frame at bin 2 -- and reduces under
//                    the tie rule
//   k_radon_peel     a streaming copy of the frames that continue into the other V, M set, compacted (slot a <- the line's
//                    slot), with the line's band set to +0 / 0.  The band's centre per column (q = 0, 1) or per row of V
//                    (q = 2, 3: there the band runs along V's rows) is computed once per workgroup into LDS, so both orientation
//                    pairs are one row-contiguous pass
#pragma once
#include "k_radon.h"

#define RADL_ROWS 8      // rows of V a workgroup of k_radon_peel copies
#define RADL_TILE 1024   // prefix values staged in LDS at a time by k_radon_extent

struct RadonLineDev {
    int slot, q, y0, s;     // slot: the frame's place in the round's V, M and sigma
};
struct RadonExtDev {
    int c1, c2, n;          // n < 0: no candidate
    float sum, snr;
    int pad[3];
};

// definition step 7: the row offset of line (y, s) in column c of a working array of width P
__device__ __forceinline__ int rad_path(int c, int s, int P) {
    int d = 0;
    for (int n = P >> 1; n > 0; n >>= 1, s >>= 1)
        if (c & n) d += (s + 1) >> 1;
    return d;
}

// the cell (r, c) of orientation q in V (elements from the frame's start)
__device__ __forceinline__ size_t rad_cell(const RadonDev &p, int q, int r, int c) {
    if (q == 0) return (size_t)r * p.wb + c;
    if (q == 1) return (size_t)(p.hb - 1 - r) * p.wb + c;
    if (q == 2) return (size_t)c * p.wb + r;
    return (size_t)c * p.wb + (p.wb - 1 - r);
}

// pre / cnt: pstride = max(Hb, Wb) + 1 values per line.  width: NULL, or each line's band width k (step 16): a_c, m_c then sum
// the cells of rows y0 + d(c) .. y0 + d(c) + k-1, rows ascending
__global__ __launch_bounds__(RAD_THREADS) void k_radon_extent(const float *__restrict__ V, const uint16_t *__restrict__ M, RadonDev p,
                                                              const RadonLineDev *__restrict__ ln, const float *__restrict__ sigma,
                                                              int min_seg, float *pre, int *cnt, int pstride, RadonExtDev *__restrict__ ext,
                                                              const int *__restrict__ width) {
    __shared__ float ta[RADL_TILE];
    __shared__ int tm[RADL_TILE];
    __shared__ RadonExtDev red[RAD_THREADS];
    const int tid = threadIdx.x;
    const RadonLineDev L = ln[blockIdx.x];
    const int wk = width ? width[blockIdx.x] : 1;
    const int o = L.q >> 1, R = p.R[o], C = p.C[o], P = p.P[o];
    const float *Vf = V + (size_t)L.slot * p.hb * p.wb;
    const uint16_t *Mf = M + (size_t)L.slot * p.hb * p.wb;
    float *lp = pre + (size_t)blockIdx.x * pstride;
    int *lc = cnt + (size_t)blockIdx.x * pstride;
    // a_c, m_c and their prefixes, a tile at a time: all lanes gather, lane 0 accumulates in LDS, all lanes store
    float acc = 0.0f;
    int nacc = 0;
    for (int t0 = 0; t0 < C; t0 += RADL_TILE) {
        const int len = min(RADL_TILE, C - t0);
        for (int e = tid; e < len; e += RAD_THREADS) {
            const int c = t0 + e, r = L.y0 + rad_path(c, L.s, P);
            float v = 0.0f;
            int m = 0;
            if (r >= 0 && r < R) {
                const size_t a = rad_cell(p, L.q, r, c);
                v = Vf[a];
                m = Mf[a];
            }
            for (int u = 1; u < wk; u++) {
                float v2 = 0.0f;
                int m2 = 0;
                if (r + u >= 0 && r + u < R) {
                    const size_t a = rad_cell(p, L.q, r + u, c);
                    v2 = Vf[a];
                    m2 = Mf[a];
                }
                v = v + v2;
                m += m2;
            }
            ta[e] = v;
            tm[e] = m;
        }
        __syncthreads();
        if (tid == 0)
            for (int e = 0; e < len; e++) {
                acc = acc + ta[e];
                nacc += tm[e];
                ta[e] = acc;
                tm[e] = nacc;
            }
        __syncthreads();
        for (int e = tid; e < len; e += RAD_THREADS) {
            lp[t0 + e + 1] = ta[e];
            lc[t0 + e + 1] = tm[e];
        }
        __syncthreads();
    }
    if (tid == 0) { lp[0] = 0.0f; lc[0] = 0; }
    __syncthreads();
    // every interval c1 <= c2: a lane holds one c1, the c2 side comes through LDS (all lanes read one address: a broadcast).
    // A lane meets its intervals in ascending (c1, c2), so the strict comparison keeps the lowest of equal scores.
    const float sg = sigma[L.slot];
    float bs = 0.0f, bsum = 0.0f;
    int b1 = 0, b2 = 0, bn = -1;
    for (int cb = 0; cb < C; cb += RAD_THREADS) {
        const int c1 = cb + tid;
        const bool active = c1 < C;
        const float p1 = active ? lp[c1] : 0.0f;
        const int n1 = active ? lc[c1] : 0;
        for (int t0 = cb; t0 < C; t0 += RADL_TILE) {
            const int len = min(RADL_TILE, C - t0);
            __syncthreads();
            for (int e = tid; e < len; e += RAD_THREADS) {
                ta[e] = lp[t0 + e + 1];
                tm[e] = lc[t0 + e + 1];
            }
            __syncthreads();
            if (!active) continue;
            for (int e = max(0, c1 - t0); e < len; e++) {
                const int N = tm[e] - n1;
                if (N < min_seg) continue;
                const float A = ta[e] - p1;
                const float snr = __fdiv_rn(A, __fmul_rn(sg, sqrtf((float)N)));
                if (bn < 0 || snr > bs) { bs = snr; bsum = A; b1 = c1; b2 = t0 + e; bn = N; }
            }
        }
    }
    red[tid].c1 = b1; red[tid].c2 = b2; red[tid].n = bn; red[tid].sum = bsum; red[tid].snr = bs;
    __syncthreads();
    for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const RadonExtDev x = red[tid + w], m = red[tid];
            if (x.n >= 0 && (m.n < 0 || rad_better(x.snr, 0, x.c1, x.c2, m.snr, 0, m.c1, m.c2))) red[tid] = x;
        }
        __syncthreads();
    }
    if (tid == 0) {
        RadonExtDev x = red[0];
        x.pad[0] = x.pad[1] = x.pad[2] = 0;
        ext[blockIdx.x] = x;
    }
}

template <int VEC> struct RadCell;
template <> struct RadCell<8> {
    static __device__ __forceinline__ void load(const float *a, float *o) {
        const float4 x = *(const float4 *)a, y = *(const float4 *)(a + 4);
        o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w; o[4] = y.x; o[5] = y.y; o[6] = y.z; o[7] = y.w;
    }
    static __device__ __forceinline__ void load(const uint16_t *a, unsigned *o) {
        const uint4 v = *(const uint4 *)a;
        o[0] = v.x & 0xFFFFu; o[1] = v.x >> 16; o[2] = v.y & 0xFFFFu; o[3] = v.y >> 16;
        o[4] = v.z & 0xFFFFu; o[5] = v.z >> 16; o[6] = v.w & 0xFFFFu; o[7] = v.w >> 16;
    }
    static __device__ __forceinline__ void store(float *a, const float *o) {
        *(float4 *)a = make_float4(o[0], o[1], o[2], o[3]);
        *(float4 *)(a + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
    static __device__ __forceinline__ void store(uint16_t *a, const unsigned *o) {
        *(uint4 *)a = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
    }
};
template <> struct RadCell<1> {
    static __device__ __forceinline__ void load(const float *a, float *o) { o[0] = a[0]; }
    static __device__ __forceinline__ void load(const uint16_t *a, unsigned *o) { o[0] = a[0]; }
    static __device__ __forceinline__ void store(float *a, const float *o) { a[0] = o[0]; }
    static __device__ __forceinline__ void store(uint16_t *a, const unsigned *o) { a[0] = (uint16_t)o[0]; }
};

// Slot blockIdx.z of the output = slot ln[blockIdx.z].slot of the input without the band of half-width hw cells around the line.
// width: NULL, or each line's band width k (step 16): the blot then reaches hw cells beyond lines y0 and y0 + k-1.
// VEC = 8 needs Wb a multiple of 8 (then every row of V starts on 16 bytes and every row of M too); VEC = 1 takes any Wb.
template <int VEC>
__global__ __launch_bounds__(RAD_THREADS) void k_radon_peel(const float *__restrict__ Vin, const uint16_t *__restrict__ Min, RadonDev p,
                                                            const RadonLineDev *__restrict__ ln, int hw, float *__restrict__ Vout,
                                                            uint16_t *__restrict__ Mout, const int *__restrict__ width) {
    __shared__ int cc[RAD_THREADS * VEC];   // q = 0, 1: the band's centre row of V in each column of the tile
    __shared__ int cr[RADL_ROWS];           // q = 2, 3: the band's centre column of V in each row of the tile
    const int tid = threadIdx.x;
    const RadonLineDev L = ln[blockIdx.z];
    const int i0 = (int)blockIdx.x * RAD_THREADS * VEC, j0 = (int)blockIdx.y * RADL_ROWS;
    const int P = p.P[L.q >> 1];
    // (the band's further lines lie at higher working rows: below in V for the flipped orientations 1 and 3)
    const int more = hw + (width ? width[blockIdx.z] : 1) - 1, lo = L.q & 1 ? -more : -hw, hi = L.q & 1 ? hw : more;
    if (L.q < 2) {
        for (int e = tid; e < RAD_THREADS * VEC; e += RAD_THREADS) {
            const int r = L.y0 + rad_path(i0 + e, L.s, P);
            cc[e] = L.q == 0 ? r : p.hb - 1 - r;
        }
    } else if (tid < RADL_ROWS) {
        const int r = L.y0 + rad_path(j0 + tid, L.s, P);
        cr[tid] = L.q == 2 ? r : p.wb - 1 - r;
    }
    __syncthreads();
    const int i = i0 + tid * VEC;
    if (i >= p.wb) return;
    const size_t px = (size_t)p.hb * p.wb;
    const float *vi = Vin + (size_t)L.slot * px;
    const uint16_t *mi = Min + (size_t)L.slot * px;
    float *vo = Vout + (size_t)blockIdx.z * px;
    uint16_t *mo = Mout + (size_t)blockIdx.z * px;
    const bool byrow = L.q >= 2;
    int ctrs[VEC];                          // (the lane's own columns' centres: contiguous in LDS, read once)
#pragma unroll
    for (int k = 0; k < VEC; k++) ctrs[k] = byrow ? 0 : cc[tid * VEC + k];
#pragma unroll
    for (int jj = 0; jj < RADL_ROWS; jj++) {
        const int j = j0 + jj;
        if (j >= p.hb) break;
        const size_t a = (size_t)j * p.wb + i;
        float v[VEC];
        unsigned m[VEC];
        RadCell<VEC>::load(vi + a, v);
        RadCell<VEC>::load(mi + a, m);
        const int ctr = byrow ? cr[jj] : 0;
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            const int dist = byrow ? i + k - ctr : j - ctrs[k];
            const bool blot = dist >= lo && dist <= hi;
            v[k] = blot ? 0.0f : v[k];
            m[k] = blot ? 0u : m[k];
        }
        RadCell<VEC>::store(vo + a, v);
        RadCell<VEC>::store(mo + a, m);
    }
}
