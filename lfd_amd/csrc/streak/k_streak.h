// k_streak.h -- kernels of the short-streak search (include/lfdmi.h: short-streak search; host side in streak.hip).
//   k_streak_prep     validity test, byte swap, fixed point and binning: one int2 {G, M} per binned cell, written once
//   k_streak_search   a workgroup owns STK_TR x STK_TC anchors of one orientation of one frame.  It stages their cells with a halo
//                     of L-1 columns and L-1 rows either side in LDS, value and count together (int2), q = 1 through the
//                     transposition in its loads.  A wave takes STK_TR / 4 anchor rows, its lanes consecutive c0: for the
//                     wave-uniform (s, i) the 64 addresses are consecutive, and the row offset is scalar arithmetic shared by
//                     the wave's rows.  Every existing segment is summed in int32 and scored; the workgroup's best goes out
//                     as one 64-bit key
//   k_streak_finish   one workgroup per frame: the largest key, decoded, its S and N summed again from the cells, the record
//   k_streak_peel     step 7 of the frames whose record is found, in place
// Every sum is an integer, so no result depends on the tiling or on the order of any reduction; the keys are compared with
// integer maxima only.  Built with -ffp-contract=off; the score uses the correctly rounded intrinsics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define STK_THREADS 256
#define STK_TC 64        // anchor columns of a workgroup of k_streak_search: a wave's lanes
#define STK_TR 16        // anchor rows of a workgroup: four per wave
#define STK_WR (STK_TR / (STK_THREADS / 64))
#define STK_MAX_CELLS 4096   // Hb and Wb at most: r0 and c0 take 12 bits each of the tie key

struct StreakDev {
    int h, w, b, hb, wb, be, L, hw;
    float clip, threshold;
    int nparts;             // partial keys per frame: the grid of k_streak_search over both orientations
};
struct StreakRec {          // lfdmi_streak up to snr
    int status, found, q, s, r0, c0, n_pix;
    float sum, snr;
};

// step 4's row offset of cell i of a segment of slope s (|s| = a, sign sg)
template <int L> __device__ __forceinline__ int stk_off(int a, int sg, int i) { return sg * ((2 * a * i + (L - 1)) / (2 * (L - 1))); }
__device__ __forceinline__ int stk_off_rt(int L, int s, int i) {
    const int a = s < 0 ? -s : s, o = (2 * a * i + (L - 1)) / (2 * (L - 1));
    return s < 0 ? -o : o;
}

// float32 bits in an order that unsigned comparison keeps, and back
__device__ __forceinline__ uint32_t stk_ord(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float stk_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
// the tie key (q, s + L-1, r0, c0), lowest first, inverted so that the larger key wins
__device__ __forceinline__ unsigned long long stk_key(float snr, int q, int sidx, int r0, int c0) {
    const uint32_t tie = ((uint32_t)q << 31) | ((uint32_t)sidx << 24) | ((uint32_t)r0 << 12) | (uint32_t)c0;
    return ((unsigned long long)stk_ord(snr) << 32) | (uint32_t)~tie;
}
// step 5's score of integer sums: one rounding to A, then the three of the faint-trail search
__device__ __forceinline__ float stk_amp(int S) { return (float)((double)S * (1.0 / 1048576.0)); }
__device__ __forceinline__ float stk_snr(int S, int N, float sg) { return __fdiv_rn(stk_amp(S), __fmul_rn(sg, sqrtf((float)N))); }

__global__ __launch_bounds__(STK_THREADS) void k_streak_prep(const uint32_t *__restrict__ src, StreakDev p, int2 *__restrict__ cells) {
    const int i = blockIdx.x * STK_THREADS + threadIdx.x, j = blockIdx.y, f = blockIdx.z;
    if (i >= p.wb) return;
    const uint32_t *fr = src + (size_t)f * p.h * p.w;
    int acc = 0, cnt = 0;
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
            if (valid) {
                acc += (int)__double2ll_rn((double)v * 1048576.0);
                cnt++;
            }
        }
    }
    cells[((size_t)f * p.hb + j) * p.wb + i] = make_int2(acc, cnt);
}

// idx: the frames of this round (slot z -> frame of the chunk); part: nparts keys per slot
template <int L>
__global__ __launch_bounds__(STK_THREADS) void k_streak_search(const int2 *__restrict__ cells, StreakDev p, const int *__restrict__ idx,
                                                               const float *__restrict__ sigma, unsigned long long *__restrict__ part) {
    constexpr int LC = STK_TC + L - 1, LR = STK_TR + 2 * (L - 1);
    extern __shared__ int2 stk_lds[];   // LR rows of LC cells
    __shared__ unsigned long long wg_best;
    const int tid = threadIdx.x, slot = blockIdx.z >> 1, q = blockIdx.z & 1;
    const int f = idx[slot];
    const int R = q ? p.wb : p.hb, C = q ? p.hb : p.wb;
    const int tc0 = blockIdx.x * STK_TC, tr0 = blockIdx.y * STK_TR;
    unsigned long long *out = part + (size_t)slot * p.nparts + ((size_t)q * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (C < L || tc0 > C - L || tr0 >= R) {   // no anchor here (the grid covers the larger orientation)
        if (tid == 0) *out = 0ull;
        return;
    }
    const int2 *fr = cells + (size_t)f * p.hb * p.wb;
    if (tid == 0) wg_best = 0ull;
    // the tile: working rows tr0 - (L-1) .. tr0 + STK_TR - 1 + (L-1), columns tc0 .. tc0 + LC - 1; what does not exist is 0.
    // Consecutive threads run along the array's rows: along c for q = 0, along r for q = 1
    if (q == 0) {
        for (int k = tid; k < LR * LC; k += STK_THREADS) {
            const int lr = k / LC, lc = k - lr * LC, r = tr0 - (L - 1) + lr, c = tc0 + lc;
            int2 v = make_int2(0, 0);
            if (r >= 0 && r < R && c < C) v = fr[(size_t)r * p.wb + c];
            stk_lds[k] = v;
        }
    } else {
        for (int k = tid; k < LR * LC; k += STK_THREADS) {
            const int lc = k / LR, lr = k - lc * LR, r = tr0 - (L - 1) + lr, c = tc0 + lc;
            int2 v = make_int2(0, 0);
            if (r >= 0 && r < R && c < C) v = fr[(size_t)c * p.wb + r];
            stk_lds[lr * LC + lc] = v;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, c0 = tc0 + lane;
    const int row0 = wave * STK_WR;            // the wave's first anchor row within the tile
    const float sg = sigma[f];
    const int need = L * p.b * p.b;
    const bool col_ok = c0 + L - 1 < C;
    unsigned long long best = 0ull;
    for (int s = -(L - 1); s <= L - 1; s++) {
        const int a = s < 0 ? -s : s, sgn = s < 0 ? -1 : 1;
        int S[STK_WR], N[STK_WR];
#pragma unroll
        for (int k = 0; k < STK_WR; k++) { S[k] = 0; N[k] = 0; }
#pragma unroll 8
        for (int i = 0; i < L; i++) {
            const int2 *cell = stk_lds + (row0 + (L - 1) + stk_off<L>(a, sgn, i)) * LC + lane + i;
#pragma unroll
            for (int k = 0; k < STK_WR; k++) {
                const int2 v = cell[k * LC];
                S[k] += v.x;
                N[k] += v.y;
            }
        }
#pragma unroll
        for (int k = 0; k < STK_WR; k++) {
            const int r0 = tr0 + row0 + k;
            const bool exists = col_ok && r0 < R && r0 + s >= 0 && r0 + s < R;
            if (exists && 2 * N[k] >= need) {
                const unsigned long long key = stk_key(stk_snr(S[k], N[k], sg), q, s + L - 1, r0, c0);
                best = key > best ? key : best;
            }
        }
    }
    if (best) atomicMax(&wg_best, best);
    __syncthreads();
    if (tid == 0) *out = wg_best;
}

__global__ __launch_bounds__(STK_THREADS) void k_streak_finish(const int2 *__restrict__ cells, StreakDev p, const int *__restrict__ idx,
                                                               const float *__restrict__ sigma, const unsigned long long *__restrict__ part,
                                                               StreakRec *__restrict__ rec) {
    __shared__ unsigned long long fr_best;
    const int tid = threadIdx.x, slot = blockIdx.x;
    if (tid == 0) fr_best = 0ull;
    __syncthreads();
    unsigned long long best = 0ull;
    for (int i = tid; i < p.nparts; i += STK_THREADS) {
        const unsigned long long k = part[(size_t)slot * p.nparts + i];
        best = k > best ? k : best;
    }
    if (best) atomicMax(&fr_best, best);
    __syncthreads();
    if (tid != 0) return;
    StreakRec r;
    r.status = 1; r.found = 0; r.q = 0; r.s = 0; r.r0 = 0; r.c0 = 0; r.n_pix = 0; r.sum = 0.0f; r.snr = 0.0f;
    const unsigned long long key = fr_best;
    if (key) {
        const uint32_t tie = ~(uint32_t)key;
        r.status = 0;
        r.q = (int)(tie >> 31);
        r.s = (int)((tie >> 24) & 127u) - (p.L - 1);
        r.r0 = (int)((tie >> 12) & 4095u);
        r.c0 = (int)(tie & 4095u);
        const int2 *fr = cells + (size_t)idx[slot] * p.hb * p.wb;
        int S = 0, N = 0;
        for (int i = 0; i < p.L; i++) {
            const int rr = r.r0 + stk_off_rt(p.L, r.s, i), cc = r.c0 + i;
            const int2 v = r.q ? fr[(size_t)cc * p.wb + rr] : fr[(size_t)rr * p.wb + cc];
            S += v.x;
            N += v.y;
        }
        r.n_pix = N;
        r.sum = stk_amp(S);
        r.snr = stk_unord((uint32_t)(key >> 32));
        r.found = r.snr >= p.threshold;
    }
    rec[slot] = r;
}

// the slots of the round that just ended: a frame whose record is found loses the record's footprint (step 7)
__global__ __launch_bounds__(STK_THREADS) void k_streak_peel(int2 *__restrict__ cells, StreakDev p, const int *__restrict__ idx,
                                                             const StreakRec *__restrict__ rec) {
    const int i = blockIdx.x * STK_THREADS + threadIdx.x, j = blockIdx.y, slot = blockIdx.z;
    if (i >= p.wb) return;
    const StreakRec r = rec[slot];
    if (r.status != 0 || !r.found) return;
    const int wr = r.q ? i : j, wc = r.q ? j : i;       // working (row, column) of cell (j, i)
    const int d = wc - r.c0;
    if (d < -p.hw || d > p.L - 1 + p.hw) return;
    const int ic = d < 0 ? 0 : (d > p.L - 1 ? p.L - 1 : d);
    int dr = wr - (r.r0 + stk_off_rt(p.L, r.s, ic));
    if (dr < 0) dr = -dr;
    if (dr <= p.hw) cells[((size_t)idx[slot] * p.hb + j) * p.wb + i] = make_int2(0, 0);
}
