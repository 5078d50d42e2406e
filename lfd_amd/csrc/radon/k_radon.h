// k_radon.h -- kernels of the faint-trail search (include/lfdmi.h: faint-trail search; host side in radon.hip).
//   k_radon_prep     validity test, byte swap and binning: V (float32) and M (16-bit counts), written once
//   k_radon_first    levels 1 .. G (G = 32 columns, or P/2 of a small frame) in LDS over a band of rows with its halo; the flip
//                    and the transposition of the orientation happen in its loads, which stay contiguous in V's rows
//   k_radon_level    one streaming level n -> 2n on planes laid out [strip][y][s]: the left strip's input is read straight
//                    from global memory, the right strip's, which sits on a diagonal (row y + t, slope t), through an LDS tile
//                    filled by row-contiguous loads; 16-byte accesses
//   k_radon_level<FINAL>  the last level: never written; every output is scored and the best (snr, s, y) of the workgroup kept
//   k_radon_level<SCORE>  a stored level 2n >= min_strip that also scores every output it stores as a short candidate (step 10)
//                    and keeps the workgroup's best in one partial record; the short search only (k_radon_short.h)
//   k_radon_finish   one workgroup per frame: the best of the partial records, ties to the lowest (q, s, y)
// A value of level n is stored only for rows -(n-1) .. R-1: what lies outside is +0 by the definition and is neither written
// nor read.  Built with -ffp-contract=off; the score uses the correctly rounded intrinsics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RAD_THREADS 256
#define RAD_G 32        // strip width k_radon_first reaches
#define RAD_BAND 64     // rows of level G a workgroup of k_radon_first writes (it loads RAD_BAND + G - 1)
#define RAD_TP (RAD_BAND + RAD_G + 1)   // LDS row count per column, odd
#define RAD_TT 32       // slopes of the input level per workgroup of k_radon_level
#define RAD_Y 128       // output rows per workgroup of k_radon_level
#define RAD_LS 33       // LDS row stride of the right strip's tile (the diagonal reads of a wave fall on distinct banks)

struct RadonDev {
    int h, w, b, hb, wb, be, min_len;
    float clip;
    int R[2], C[2], P[2];   // orientations {0, 1} and {2, 3}
    long long off[4];       // plane of orientation q within a frame's planes (elements)
    long long frame_elems;  // a frame's four planes (elements)
    int part_stride;        // partial records per (frame, orientation)
};
struct RadonPart {
    float snr, sum;
    int s, y, n;            // n < 0: no candidate
};
struct RadonShortPart {     // a workgroup's best short candidate of one level (its L, q come from the record's place)
    float snr, sum;
    int s, y, n, j;         // n < 0: no candidate
};
struct RadonRec {
    int status, q, y0, s, n_pix;
    float sum, snr;
    int pad;
};

// is candidate a (score, q, s, y) better than b?  larger snr; ties to the lowest (q, s, y)
__device__ __forceinline__ bool rad_better(float sa, int qa, int ssa, int ya, float sb, int qb, int ssb, int yb) {
    const bool lower = qa < qb || (qa == qb && (ssa < ssb || (ssa == ssb && ya < yb)));
    return sa > sb || (sa == sb && lower);
}

__global__ __launch_bounds__(RAD_THREADS) void k_radon_prep(const uint32_t *__restrict__ src, RadonDev p, float *__restrict__ V,
                                                            uint16_t *__restrict__ M) {
    const int i = blockIdx.x * RAD_THREADS + threadIdx.x, j = blockIdx.y, f = blockIdx.z;
    if (i >= p.wb) return;
    const uint32_t *fr = src + (size_t)f * p.h * p.w;
    float acc = 0.0f;
    int cnt = 0;
    for (int dy = 0; dy < p.b; dy++) {
        const int y = j * p.b + dy;
        if (y >= p.h) break;
        const uint32_t *row = fr + (size_t)(p.h - 1 - y) * p.w;
        for (int dx = 0; dx < p.b; dx++) {
            const int x = i * p.b + dx;
            if (x >= p.w) break;
            uint32_t bits = row[x];
            if (p.be) bits = __builtin_bswap32(bits);
            const float v = __uint_as_float(bits);
            const bool valid = (bits & 0x7F800000u) != 0x7F800000u && (bits & 0x7FFFFFFFu) != 0u && fabsf(v) <= p.clip;
            acc = acc + (valid ? v : 0.0f);
            cnt += valid;
        }
    }
    const size_t o = ((size_t)f * p.hb + j) * p.wb + i;
    V[o] = acc;
    M[o] = (uint16_t)cnt;
}

__global__ __launch_bounds__(RAD_THREADS) void k_radon_first(const float *__restrict__ V, const uint16_t *__restrict__ M, RadonDev p,
                                                             float *__restrict__ S, uint16_t *__restrict__ N) {
    __shared__ float ls[2][RAD_G * RAD_TP];
    __shared__ uint16_t ln[2][RAD_G * RAD_TP];
    const int tid = threadIdx.x, q = blockIdx.z & 3, f = blockIdx.z >> 2, o = q >> 1;
    const int R = p.R[o], C = p.C[o], P = p.P[o];
    const int G = min(RAD_G, P / 2), jg = blockIdx.y;
    if (jg >= P / G) return;
    const int yb = -(G - 1) + (int)blockIdx.x * RAD_BAND;
    if (yb > R - 1) return;
    const int T = RAD_BAND + G - 1;     // rows loaded: an output row y reads rows y .. y + G - 1
    const float *Vf = V + (size_t)f * p.hb * p.wb;
    const uint16_t *Mf = M + (size_t)f * p.hb * p.wb;
    for (int e = tid; e < G * T; e += RAD_THREADS) {
        int c, yy;
        if (q < 2) { c = e % G; yy = e / G; }     // V's rows run along c
        else { yy = e % T; c = e / T; }           // V's rows run along r: the transposition goes through LDS
        const int r = yb + yy, col = jg * G + c;
        float v = 0.0f;
        uint16_t m = 0;
        if (r >= 0 && r < R && col < C) {
            size_t a;
            if (q == 0) a = (size_t)r * p.wb + col;
            else if (q == 1) a = (size_t)(p.hb - 1 - r) * p.wb + col;
            else if (q == 2) a = (size_t)col * p.wb + r;
            else a = (size_t)col * p.wb + (p.wb - 1 - r);
            v = Vf[a];
            m = Mf[a];
        }
        ls[0][c * RAD_TP + yy] = v;
        ln[0][c * RAD_TP + yy] = m;
    }
    __syncthreads();
    int cur = 0;
    for (int n = 1; n < G; n *= 2) {
        const float *is = ls[cur];
        const uint16_t *in = ln[cur];
        float *os = ls[cur ^ 1];
        uint16_t *on = ln[cur ^ 1];
        const int n2 = 2 * n;
        for (int e = tid; e < G * T; e += RAD_THREADS) {
            const int s = e % n2, rest = e / n2, yy = rest % T, cs = rest / T;
            const int t = s >> 1, yy2 = yy + ((s + 1) >> 1);
            const int ia = ((2 * cs) * RAD_TP + yy) * n + t;
            float v = is[ia];
            uint16_t m = in[ia];
            if (yy2 < T) {      // (a row past the tile only feeds rows that are not written)
                const int ib = ((2 * cs + 1) * RAD_TP + yy2) * n + t;
                v = v + is[ib];
                m = (uint16_t)(m + in[ib]);
            }
            os[(cs * RAD_TP + yy) * n2 + s] = v;
            on[(cs * RAD_TP + yy) * n2 + s] = m;
        }
        __syncthreads();
        cur ^= 1;
    }
    const size_t RP = (size_t)R + P - 1;
    const size_t base = (size_t)f * p.frame_elems + p.off[q] + ((size_t)jg * RP + (size_t)(yb + P - 1)) * G;
    const int rows = min(RAD_BAND, R - yb);
    for (int e = tid; e < rows * G; e += RAD_THREADS) {   // level G of this strip: rows x G contiguous values
        S[base + e] = ls[cur][e];
        N[base + e] = ln[cur][e];
    }
}

template <int VEC> struct RadVec;
template <> struct RadVec<4> {
    static __device__ __forceinline__ void load(const float *a, float *o) {
        const float4 v = *(const float4 *)a;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    static __device__ __forceinline__ void load(const uint16_t *a, unsigned *o) {
        const ushort4 v = *(const ushort4 *)a;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    static __device__ __forceinline__ void store(float *a, const float *o) {
        *(float4 *)a = make_float4(o[0], o[1], o[2], o[3]);
        *(float4 *)(a + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
    static __device__ __forceinline__ void store(uint16_t *a, const unsigned *o) {
        *(uint4 *)a = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
    }
};
template <> struct RadVec<1> {
    static __device__ __forceinline__ void load(const float *a, float *o) { o[0] = a[0]; }
    static __device__ __forceinline__ void load(const uint16_t *a, unsigned *o) { o[0] = a[0]; }
    static __device__ __forceinline__ void store(float *a, const float *o) { a[0] = o[0]; a[1] = o[1]; }
    static __device__ __forceinline__ void store(uint16_t *a, const unsigned *o) { a[0] = (uint16_t)o[0]; a[1] = (uint16_t)o[1]; }
};

// Level n -> 2n of orientation pair o (grid.z = frame * 2 + (q & 1)).  VEC = 4 needs n >= 32; VEC = 1 takes any n.  FINAL: 2n = P.
// SCORE (never FINAL, VEC = 4 only): every stored output with N >= n b b (step 10: 2 N >= L b b, L = 2n) is scored, and the
// workgroup's best goes to spart[f * stotal + soff + (q & 1) * workgroups per q + its place in the grid].
template <int VEC, bool FINAL, bool SCORE = false>
__global__ __launch_bounds__(RAD_THREADS) void k_radon_level(const float *__restrict__ Sin, const uint16_t *__restrict__ Nin,
                                                             float *__restrict__ Sout, uint16_t *__restrict__ Nout, RadonDev p, int o, int n,
                                                             const float *__restrict__ sigma, RadonPart *__restrict__ part,
                                                             RadonShortPart *__restrict__ spart, long long soff, long long stotal) {
    static_assert(!SCORE || (VEC == 4 && !FINAL), "only a stored 16-byte level scores short candidates");
    __shared__ float lb[(RAD_Y + RAD_TT) * RAD_LS];
    __shared__ uint16_t lc[(RAD_Y + RAD_TT) * RAD_LS];
    const int tid = threadIdx.x, q = 2 * o + (blockIdx.z & 1), f = blockIdx.z >> 1;
    const int R = p.R[o], P = p.P[o];
    const int Tt = min(RAD_TT, n), chunks = n / Tt;
    const int j = blockIdx.y / chunks, t0 = (blockIdx.y % chunks) * Tt;
    const int yb = -(2 * n - 1) + (int)blockIdx.x * RAD_Y;
    const size_t RP = (size_t)R + P - 1;
    const size_t fbase = (size_t)f * p.frame_elems + p.off[q];
    float bs = 0.0f, bsum = 0.0f;
    int bss = 0, by = 0, bn = -1;
    if (yb <= R - 1) {
        const size_t offA = fbase + (size_t)(2 * j) * RP * n, offB = offA + RP * n;
        // the right strip's rows yb + t0 .. yb + t0 + RAD_Y + Tt - 1, slopes t0 .. t0 + Tt - 1
        const int per = Tt / VEC, nrows = RAD_Y + Tt;
        for (int e = tid; e < nrows * per; e += RAD_THREADS) {
            const int rr = e / per, c = (e % per) * VEC, y = yb + t0 + rr;
            float v[VEC];
            unsigned m[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) { v[k] = 0.0f; m[k] = 0u; }
            if (y >= -(n - 1) && y <= R - 1) {
                const size_t a = offB + (size_t)(y + P - 1) * n + t0 + c;
                RadVec<VEC>::load(Sin + a, v);
                RadVec<VEC>::load(Nin + a, m);
            }
#pragma unroll
            for (int k = 0; k < VEC; k++) {
                lb[rr * RAD_LS + c + k] = v[k];
                lc[rr * RAD_LS + c + k] = (uint16_t)m[k];
            }
        }
        __syncthreads();
        const int tq = tid % per, ry = tid / per, step = RAD_THREADS / per;
        const float sg = FINAL || SCORE ? sigma[f] : 0.0f;
        const unsigned need = SCORE ? (unsigned)(n * p.b * p.b) : 0u;
        for (int yy = ry; yy < RAD_Y; yy += step) {
            const int y = yb + yy;
            if (y > R - 1) break;
            float a[VEC];
            unsigned am[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) { a[k] = 0.0f; am[k] = 0u; }
            if (y >= -(n - 1)) {
                const size_t ad = offA + (size_t)(y + P - 1) * n + t0 + tq * VEC;
                RadVec<VEC>::load(Sin + ad, a);
                RadVec<VEC>::load(Nin + ad, am);
            }
            float os[2 * VEC];
            unsigned om[2 * VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) {
                const int tt = tq * VEC + k;
                const int i0 = (yy + tt) * RAD_LS + tt, i1 = i0 + RAD_LS;
                os[2 * k] = a[k] + lb[i0];
                os[2 * k + 1] = a[k] + lb[i1];
                om[2 * k] = am[k] + lc[i0];
                om[2 * k + 1] = am[k] + lc[i1];
            }
            if (!FINAL) {
                const size_t ao = fbase + ((size_t)j * RP + (size_t)(y + P - 1)) * (2 * n) + 2 * (t0 + tq * VEC);
                RadVec<VEC>::store(Sout + ao, os);
                RadVec<VEC>::store(Nout + ao, om);
                if constexpr (SCORE) {
#pragma unroll
                    for (int k = 0; k < 2 * VEC; k++) {
                        const int s = 2 * (t0 + tq * VEC) + k;
                        const float snr = __fdiv_rn(os[k], __fmul_rn(sg, sqrtf((float)om[k])));
                        const bool take = om[k] >= need && (bn < 0 || rad_better(snr, 0, s, y, bs, 0, bss, by));
                        bs = take ? snr : bs; bsum = take ? os[k] : bsum; bss = take ? s : bss; by = take ? y : by; bn = take ? (int)om[k] : bn;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2 * VEC; k++) {
                    if ((int)om[k] < p.min_len) continue;
                    const int s = 2 * (t0 + tq * VEC) + k;
                    // (sqrtf is the correctly rounded one here; __fsqrt_rn maps to the 1-ulp native instruction)
                    const float snr = __fdiv_rn(os[k], __fmul_rn(sg, sqrtf((float)om[k])));
                    const bool take = bn < 0 || rad_better(snr, 0, s, y, bs, 0, bss, by);
                    bs = take ? snr : bs; bsum = take ? os[k] : bsum; bss = take ? s : bss; by = take ? y : by; bn = take ? (int)om[k] : bn;
                }
            }
        }
    }
    if (FINAL) {
        __shared__ RadonPart red[RAD_THREADS];
        red[tid].snr = bs; red[tid].sum = bsum; red[tid].s = bss; red[tid].y = by; red[tid].n = bn;
        __syncthreads();
        for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const RadonPart x = red[tid + w], m = red[tid];
                if (x.n >= 0 && (m.n < 0 || rad_better(x.snr, 0, x.s, x.y, m.snr, 0, m.s, m.y))) red[tid] = x;
            }
            __syncthreads();
        }
        if (tid == 0) part[((size_t)f * 4 + q) * p.part_stride + (size_t)blockIdx.x * gridDim.y + blockIdx.y] = red[0];
    }
    if constexpr (SCORE) {
        __syncthreads();                        // the right strip's tile has been read: its LDS holds the reduction
        RadonPart *red = (RadonPart *)lb;
        red[tid].snr = bs; red[tid].sum = bsum; red[tid].s = bss; red[tid].y = by; red[tid].n = bn;
        __syncthreads();
        for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const RadonPart x = red[tid + w], m = red[tid];
                if (x.n >= 0 && (m.n < 0 || rad_better(x.snr, 0, x.s, x.y, m.snr, 0, m.s, m.y))) red[tid] = x;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const RadonPart x = red[0];
            RadonShortPart r;
            r.snr = x.snr; r.sum = x.sum; r.s = x.s; r.y = x.y; r.n = x.n; r.j = j;
            spart[(size_t)f * stotal + soff + (size_t)(q & 1) * gridDim.x * gridDim.y + (size_t)blockIdx.x * gridDim.y + blockIdx.y] = r;
        }
    }
}

// np0 / np1: partial records of orientations {0, 1} / {2, 3}
__global__ __launch_bounds__(RAD_THREADS) void k_radon_finish(const RadonPart *__restrict__ part, RadonDev p, int np0, int np1,
                                                              RadonRec *__restrict__ rec) {
    __shared__ RadonPart red[RAD_THREADS];
    __shared__ int rq[RAD_THREADS];
    const int tid = threadIdx.x, f = blockIdx.x;
    RadonPart b;
    b.snr = 0.0f; b.sum = 0.0f; b.s = 0; b.y = 0; b.n = -1;
    int bq = 0;
    for (int q = 0; q < 4; q++) {
        const int np = q < 2 ? np0 : np1;
        const RadonPart *pq = part + ((size_t)f * 4 + q) * p.part_stride;
        for (int i = tid; i < np; i += RAD_THREADS) {
            const RadonPart x = pq[i];
            if (x.n >= 0 && (b.n < 0 || rad_better(x.snr, q, x.s, x.y, b.snr, bq, b.s, b.y))) { b = x; bq = q; }
        }
    }
    red[tid] = b;
    rq[tid] = bq;
    __syncthreads();
    for (int w = RAD_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const RadonPart x = red[tid + w], m = red[tid];
            if (x.n >= 0 && (m.n < 0 || rad_better(x.snr, rq[tid + w], x.s, x.y, m.snr, rq[tid], m.s, m.y))) { red[tid] = x; rq[tid] = rq[tid + w]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        RadonRec r;
        const RadonPart x = red[0];
        r.pad = 0;
        if (x.n < 0) { r.status = 1; r.q = 0; r.y0 = 0; r.s = 0; r.n_pix = 0; r.sum = 0.0f; r.snr = 0.0f; }
        else { r.status = 0; r.q = rq[0]; r.y0 = x.y; r.s = x.s; r.n_pix = x.n; r.sum = x.sum; r.snr = x.snr; }
        rec[f] = r;
    }
}
