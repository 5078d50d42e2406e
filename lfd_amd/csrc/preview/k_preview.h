// k_preview.h -- kernels of the frame previews (include/lfdmi.h: frame previews).
//   k_preview_bin     one wavefront per (frame, preview row, segment of 256 columns), four to a workgroup.  A lane owns four
//                     neighbouring columns and walks the b rows of the preview row: one 16 B load a row where every row starts on
//                     a 16 B boundary (p.vec), four 4 B loads otherwise; the byte swap and the validity test as a pixel is loaded,
//                     the row flip in the address, q by prev_fix.  The four sums and counts stay in registers; b = 1, 2, 4 leave
//                     4, 2, 1 cells in a lane, b = 8, 16 add 2, 4 lanes by shuffles (256 is a multiple of 16: no cell crosses a
//                     segment).  8 B per cell out, neighbouring lanes neighbouring cells.
//   k_preview_limits  one workgroup per frame.  Pass 0 of eight radix passes (8 bits each, from the top, keys = the cells with
//                     the sign bit flipped) also counts M.  A pass histograms the cells that match a rank's prefix into 256
//                     LDS counters; thread 0 walks them to the bucket that holds the rank.  Both ranks use one histogram while
//                     their prefixes are equal.  A wavefront whose matching cells share a bucket (the rule in the top passes,
//                     where every key starts alike) adds its count once.  GIVEN mode stops after the count.
//   k_preview_render  lut in LDS, a byte per thread: step 5 of the definition, one IEEE division and multiplication in double.
// Integer atomics on LDS only; no float sum, no transcendental.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PRV_THREADS 256
#define PRV_WAVES (PRV_THREADS / 64)
#define PRV_SEG 256                             // columns of a wavefront's item: 64 lanes x 4 pixels
#define PRV_SEL_THREADS 1024
#define PRV_LUT 4096
#define PRV_EMPTY_CELL ((long long)0x8000000000000000ull)   // INT64_MIN
#define PRV_OK 0
#define PRV_FLAT 1
#define PRV_EMPTY 2
#define PRV_RANK 0
#define PRV_GIVEN 1

struct PrevDev {
    int32_t h, w, be, lg;                       // lg = log2(bin)
    int32_t hp, wp, nseg, vec;                  // nseg = ceil(w / PRV_SEG); vec: 16 B loads are aligned
    int32_t mode, lo_ppm, hi_ppm, pad;
};
struct PrevFrameDev {
    long long lo, hi;
    int32_t n_cells, status;
};

// step 2 of the definition from the bits of a finite v, in integer arithmetic (exact; no denormal mode enters), as psf_fix
// (psf/k_psf.h) with the clamp: v = m * 2^(e - 150), so v * 2^30 = m * 2^(e - 120); |v| >= 2^24 (e >= 151) enters as 2^54
__device__ __forceinline__ long long prev_fix(uint32_t bits) {
    const int e = (int)((bits >> 23) & 0xffu);
    const long long m = (long long)(bits & 0x7fffffu) | (e ? 0x800000ll : 0ll);
    const int sh = (e ? e : 1) - 120;
    long long q;
    if (e >= 151) q = 1ll << 54;
    else if (sh >= 0) q = m << sh;
    else if (sh < -25) q = 0;                               // (m * 2^-26 < 1/4)
    else {
        const int s = -sh;
        q = (m + ((1ll << (s - 1)) - 1) + ((m >> s) & 1)) >> s;   // ties to even
    }
    return (bits >> 31) ? -q : q;
}

__global__ __launch_bounds__(PRV_THREADS) void k_preview_bin(const uint32_t *__restrict__ frames, size_t N, PrevDev p, int nf,
                                                             long long *__restrict__ cells) {
    const int lane = threadIdx.x & 63;
    const long long per_frame = (long long)p.hp * p.nseg;
    const long long item = (long long)blockIdx.x * PRV_WAVES + (threadIdx.x >> 6);
    if (item >= per_frame * nf) return;                     // (the same in every lane of a wavefront: the shuffles below are whole)
    const int f = (int)(item / per_frame);
    const int rem = (int)(item - (long long)f * per_frame);
    const int r = rem / p.nseg, s = rem - r * p.nseg;
    const int b = 1 << p.lg;
    const int c0 = s * PRV_SEG + lane * 4;                  // the lane's first column
    const int nv = min(max(p.w - c0, 0), 4);                // its columns inside the frame
    const int y0 = r * b, y1 = min(y0 + b, p.h);
    const uint32_t *fr = frames + (size_t)f * N;
    long long q[4] = {0, 0, 0, 0};
    int cnt[4] = {0, 0, 0, 0};
    for (int y = y0; y < y1; y++) {
        const uint32_t *row = fr + (size_t)(p.h - 1 - y) * p.w;   // flipped row y
        uint32_t v[4] = {0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u};
        if (p.vec) {
            if (nv) {                                       // (w % 4 == 0: a lane is inside with all four columns or with none)
                const uint4 t = *(const uint4 *)(row + c0);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < nv) v[j] = row[c0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j >= nv) continue;
            const uint32_t bits = p.be ? __builtin_bswap32(v[j]) : v[j];
            if (((bits >> 23) & 0xffu) == 0xffu) continue;  // inf, NaN
            q[j] += prev_fix(bits);
            cnt[j]++;
        }
    }
    // the lane's cells: 4, 2 or 1; with b = 8, 16 the lanes of a cell add up and the first of them writes
    int nc = 4 >> min(p.lg, 2);
    if (p.lg == 1) {
        q[0] += q[1]; cnt[0] += cnt[1];
        q[1] = q[2] + q[3]; cnt[1] = cnt[2] + cnt[3];
    } else if (p.lg >= 2) {
        q[0] += q[1] + q[2] + q[3];
        cnt[0] += cnt[1] + cnt[2] + cnt[3];
        if (p.lg >= 3) { q[0] += __shfl_xor(q[0], 1); cnt[0] += __shfl_xor(cnt[0], 1); }
        if (p.lg >= 4) { q[0] += __shfl_xor(q[0], 2); cnt[0] += __shfl_xor(cnt[0], 2); }
        if (p.lg >= 3 && (lane & ((1 << (p.lg - 2)) - 1))) nc = 0;
    }
    const int i0 = c0 >> p.lg;
    long long *dst = cells + ((size_t)f * p.hp + r) * p.wp;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < nc && i0 + j < p.wp)
            dst[i0 + j] = cnt[j] == 0 ? PRV_EMPTY_CELL : (cnt[j] == 1 ? q[j] : q[j] / cnt[j]);
}

// `in` lanes add 1 to hist[bucket]; a wavefront whose lanes agree on the bucket adds its count once
__device__ __forceinline__ void prev_hist_add(uint32_t *hist, bool in, int bucket, int lane) {
    const unsigned long long bal = __ballot(in);
    if (!bal) return;
    const int first = __ffsll((long long)bal) - 1;
    const int b0 = __shfl(bucket, first);
    if (__ballot(in && bucket == b0) == bal) {
        if (lane == first) atomicAdd(&hist[b0], (uint32_t)__popcll(bal));
    } else if (in) {
        atomicAdd(&hist[bucket], 1u);
    }
}

__global__ __launch_bounds__(PRV_SEL_THREADS) void k_preview_limits(const long long *__restrict__ cells, PrevDev p,
                                                                    const long long *__restrict__ given,
                                                                    PrevFrameDev *__restrict__ rec) {
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long s_prefix[2];
    __shared__ long long s_rank[2];
    __shared__ int s_done, s_M;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t nc = (size_t)p.hp * p.wp;
    const long long *c = cells + (size_t)f * nc;
    const unsigned long long SIGN = 0x8000000000000000ull;
    unsigned long long prefix[2] = {0, 0};
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        const unsigned long long mask = pass ? ~0ull << (shift + 8) : 0ull;
        const bool same = prefix[0] == prefix[1];
        if (tid < 512) hist[tid >> 8][tid & 255] = 0;
        __syncthreads();
        for (size_t base = (size_t)(tid & ~63); base < nc; base += PRV_SEL_THREADS) {   // (whole wavefronts: prev_hist_add ballots)
            const size_t i = base + lane;
            const long long m = i < nc ? c[i] : PRV_EMPTY_CELL;
            const bool act = m != PRV_EMPTY_CELL;
            const unsigned long long key = (unsigned long long)m ^ SIGN;
            const int bucket = (int)((key >> shift) & 255);
            prev_hist_add(hist[0], act && ((key ^ prefix[0]) & mask) == 0, bucket, lane);
            if (!same) prev_hist_add(hist[1], act && ((key ^ prefix[1]) & mask) == 0, bucket, lane);
        }
        __syncthreads();
        if (tid == 0) {
            int done = 0;
            if (pass == 0) {
                long long M = 0;
                for (int k = 0; k < 256; k++) M += hist[0][k];
                PrevFrameDev R;
                R.n_cells = s_M = (int32_t)M;
                R.lo = R.hi = 0;
                if (p.mode == PRV_GIVEN) { R.lo = given[2 * f]; R.hi = given[2 * f + 1]; }
                R.status = M == 0 ? PRV_EMPTY : (R.hi > R.lo ? PRV_OK : PRV_FLAT);
                if (M == 0 || p.mode == PRV_GIVEN) {
                    rec[f] = R;
                    done = 1;
                } else {
                    s_rank[0] = ((long long)p.lo_ppm * (M - 1)) / 1000000;
                    s_rank[1] = ((long long)p.hi_ppm * (M - 1)) / 1000000;
                }
            }
            s_done = done;
            if (!done)
                for (int t = 0; t < 2; t++) {
                    const uint32_t *hh = hist[same ? 0 : t];
                    long long rank = s_rank[t], cum = 0;
                    int k = 0;
                    for (; k < 255; k++) {                  // (the rank lies inside the matching cells: bucket 255 takes what is left)
                        if (cum + hh[k] > rank) break;
                        cum += hh[k];
                    }
                    s_rank[t] = rank - cum;
                    s_prefix[t] = prefix[t] | ((unsigned long long)k << shift);
                }
        }
        __syncthreads();
        if (s_done) return;
        prefix[0] = s_prefix[0];
        prefix[1] = s_prefix[1];
        __syncthreads();                                    // (s_prefix and hist are read before the next pass rewrites them)
    }
    if (tid == 0) {
        PrevFrameDev R;
        R.lo = (long long)(prefix[0] ^ SIGN);
        R.hi = (long long)(prefix[1] ^ SIGN);
        R.n_cells = s_M;
        R.status = R.hi > R.lo ? PRV_OK : PRV_FLAT;
        rec[f] = R;
    }
}

__global__ __launch_bounds__(PRV_THREADS) void k_preview_render(const long long *__restrict__ cells, PrevDev p,
                                                                const PrevFrameDev *__restrict__ rec, const uint8_t *__restrict__ lut,
                                                                uint8_t *__restrict__ out) {
    __shared__ uint4 s_lut4[PRV_LUT / 16];
    const uint8_t *s_lut = (const uint8_t *)s_lut4;
    s_lut4[threadIdx.x] = ((const uint4 *)lut)[threadIdx.x];   // (256 threads x 16 B; lut is the call's own allocation, aligned)
    __syncthreads();
    const int f = blockIdx.y;
    const size_t nc = (size_t)p.hp * p.wp;
    const PrevFrameDev R = rec[f];
    const long long *c = cells + (size_t)f * nc;
    uint8_t *o = out + (size_t)f * nc;
    const double range = (double)(R.hi - R.lo);
    for (size_t i = (size_t)blockIdx.x * PRV_THREADS + threadIdx.x; i < nc; i += (size_t)gridDim.x * PRV_THREADS) {
        const long long m = c[i];
        uint8_t byte = 0;
        if (R.status == PRV_OK && m != PRV_EMPTY_CELL) {
            const long long d = min(max(m, R.lo), R.hi) - R.lo;
            const int k = (int)(((double)d / range) * 4095.0);
            byte = s_lut[k];
        }
        o[i] = byte;
    }
}
