// k_lc.h -- device side of the light curves (include/lfdmi.h: light curves).  Two kernels, siblings of k_mask_cull and
// k_mask_render: k_lc_cull lists the (job, tile) pairs some segment's outer band reaches, k_lc_render reads the pixels of the
// listed tiles once and adds them, as fixed-point integers, to the five sums of every (segment, section) they belong to.  A job
// is a frame that carries at least one good segment; its segments are contiguous.  Every sum is an integer sum: no result
// depends on the tiling, on the order of the list or on the order in which the atomics arrive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LC_TILE_W 64
#define LC_TILE_H 16
#define LC_THREADS 256
#define LC_PX 4                                            // pixels of a thread: 4 neighbours of one row (one 16-byte load)
#define LC_COLS (LC_TILE_W / LC_PX)                        // threads along a tile row
#define LC_CHUNK 128                                       // segments in LDS at a time
#define LC_TAB 16                                          // sections of the LDS table: a tile spans at most 11 of one segment
// What the cull adds to a band's reach: the argument of MSK_SLACK (mask/k_mask.h), with bg_out <= 64 in place of half.  The same
// slack widens the t range from which a tile's lowest section is taken, so no pixel of the tile lies below it.
#define LC_SLACK 1e-3

struct LcSeg {
    double x1, y1;              // the first end point
    double ex, ey, nx, ny;      // unit direction e and normal (-e.y, e.x)
    double half, bg_in, bg_out; // core: |u| <= half; sky: bg_in <= |u| <= bg_out
    double L, inv;              // 0 <= t <= L; section floor(t * inv)
    int32_t n_sec;              // sections of the segment
    int32_t base;               // its first section's place in the sums
};

struct LcJob {
    int64_t foff;               // the frame's first pixel, in floats from the frame buffer's start
    int64_t moff;               // and in bytes from the mask buffer's start
    int32_t sb, se;             // its segments [sb, se)
};

struct LcDev {
    int32_t h, w, ntx, nty;     // the frame and its tile grid
    int32_t be;                 // frames are big-endian
    uint32_t skip_bits;         // a pixel with mask & skip_bits is invalid
    uint32_t clip_bits;         // the bits of clip (positive, finite): |v| <= clip is a comparison of the bit patterns
    int32_t vec;                // w % 4 == 0 and the frame buffer is 16-byte aligned: a thread's pixels are one load
    int32_t mvec;               // w % 4 == 0 and the mask buffer is 4-byte aligned
    int32_t pad;
};

// step 1 of the definition: q = llrint((double)v * 2^30) of a finite v with |v| <= 1024, from its bits in integer arithmetic
// (exact; it does not depend on a denormal mode).  v = m * 2^(e - 150) with m < 2^24, so v * 2^30 = m * 2^(e - 120).
__device__ __forceinline__ long long lc_fix(uint32_t bits) {
    const int e = (int)((bits >> 23) & 0xffu);
    const long long m = (long long)(bits & 0x7fffffu) | (e ? 0x800000ll : 0ll);
    const int sh = (e ? e : 1) - 120;
    long long q;
    if (sh >= 0) q = m << sh;                               // (e <= 137 here: below 2^41)
    else if (sh < -25) q = 0;                               // (m * 2^-26 < 1/4)
    else {
        const int s = -sh;
        q = (m + ((1ll << (s - 1)) - 1) + ((m >> s) & 1)) >> s;   // ties to even
    }
    return (bits >> 31) ? -q : q;
}

// Can the segment's outer band hold a pixel centre of the box [xa, xb] x [ya, yb] (flipped rows)?  Conservative, as msk_box_hit.
// *tlo: a lower bound of t over the box's pixel centres.
__device__ __forceinline__ bool lc_box_hit(const LcSeg &s, double xa, double xb, double ya, double yb, double *tlo) {
    const double cx = 0.5 * (xa + xb), cy = 0.5 * (ya + yb);
    const double hx = 0.5 * (xb - xa), hy = 0.5 * (yb - ya);
    const double ax = cx - s.x1, ay = cy - s.y1;
    const double u = ax * s.nx + ay * s.ny;
    const double t = ax * s.ex + ay * s.ey;
    const double rt = hx * fabs(s.ex) + hy * fabs(s.ey) + LC_SLACK;
    *tlo = t - rt;
    if (!(fabs(u) <= s.bg_out + (hx * fabs(s.nx) + hy * fabs(s.ny) + LC_SLACK))) return false;
    return t + rt >= 0.0 && t - rt <= s.L;
}

__device__ __forceinline__ void lc_tile_box(const LcDev &p, int tile, int &x0, int &x1, int &r0, int &r1) {
    const int ty = tile / p.ntx, tx = tile - ty * p.ntx;
    x0 = tx * LC_TILE_W; x1 = min(x0 + LC_TILE_W, p.w) - 1;
    r0 = ty * LC_TILE_H; r1 = min(r0 + LC_TILE_H, p.h) - 1;
}

// one thread per (job, tile): the pair is listed when any of the job's segments reaches the tile; the list's order is the order
// of arrival and no result depends on it
__global__ void __launch_bounds__(LC_THREADS) k_lc_cull(const LcJob *jobs, int njobs, const LcSeg *segs, LcDev p, int2 *list, int *count) {
    const int64_t g = (int64_t)blockIdx.x * LC_THREADS + threadIdx.x;
    const int ntiles = p.ntx * p.nty;
    if (g >= (int64_t)njobs * ntiles) return;
    const int job = (int)(g / ntiles), tile = (int)(g - (int64_t)job * ntiles);
    int x0, x1, r0, r1;
    lc_tile_box(p, tile, x0, x1, r0, r1);
    const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
    const LcJob jb = jobs[job];
    bool hit = false;
    double tlo;
    for (int k = jb.sb; k < jb.se && !hit; k++) hit = lc_box_hit(segs[k], (double)x0, (double)x1, ya, yb, &tlo);
    if (hit) list[atomicAdd(count, 1)] = make_int2(job, tile);
}

// the sum of v over the lanes of a wave, in every lane (integers: the order does not matter)
__device__ __forceinline__ int lc_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ long long lc_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Persistent blocks walk the list.  A block owns a tile: thread t owns the LC_PX pixels of row r0 + t / LC_COLS from column
// x0 + LC_PX (t % LC_COLS) on, which it loads once (16 bytes where p.vec), tests for validity and turns into q; a wave is four
// rows of the tile.  The job's segments pass through LDS in chunks of LC_CHUNK, each with the block's own verdict on whether it
// can reach the tile and with the tile's lowest section.  For a segment in hand a thread's pixels fall into at most two
// neighbouring sections (4 px of t against sec_len >= 8): it adds them up in two slots, the lanes of a wave that share a section
// add their slots up (shuffles over the runs of equal j a ballot finds) and one lane adds the run to the block's LDS table
// with integer atomics; after a barrier the non-zero entries go to the global sums with one atomicAdd each.  The loops that hold
// a barrier are uniform over the block, the ballot loops over the wave; a thread outside the frame only votes.
// cnt: 3 int32 per section (n_geom, n_core, n_sky), qsum: 2 x 64 bits per section (Q_core, Q_sky; two's complement).
__global__ void __launch_bounds__(LC_THREADS) k_lc_render(const uint32_t *frames, const uint8_t *mask, const LcJob *jobs, const LcSeg *segs, LcDev p,
                                                          const int2 *list, const int *count, int *cnt, unsigned long long *qsum) {
    __shared__ LcSeg S[LC_CHUNK];
    __shared__ int hit[LC_CHUNK];
    __shared__ int jlow[LC_CHUNK];
    __shared__ int T_cnt[3][LC_TAB];
    __shared__ unsigned long long T_q[2][LC_TAB];
    const int n = *count;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int col = (tid % LC_COLS) * LC_PX, row = tid / LC_COLS;
    if (tid < 3 * LC_TAB) (&T_cnt[0][0])[tid] = 0;
    if (tid < 2 * LC_TAB) (&T_q[0][0])[tid] = 0ull;
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int2 e = list[item];
        const LcJob jb = jobs[e.x];
        int x0, x1, r0, r1;
        lc_tile_box(p, e.y, x0, x1, r0, r1);
        const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
        const int x = x0 + col, r = r0 + row;
        const double yd = (double)(p.h - 1 - r);
        // the thread's pixels: in the frame?  valid?  q
        bool in[LC_PX], ok[LC_PX];
        long long q[LC_PX];
        {
            uint32_t b[LC_PX] = {0u, 0u, 0u, 0u};
            uint32_t mk[LC_PX] = {0u, 0u, 0u, 0u};
            const size_t px = (size_t)r * p.w + x;
            if (r <= r1 && x + LC_PX - 1 <= x1 && p.vec) {
                const uint4 v = *(const uint4 *)(frames + jb.foff + px);
                b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
            } else {
#pragma unroll
                for (int m = 0; m < LC_PX; m++)
                    if (r <= r1 && x + m <= x1) b[m] = frames[jb.foff + px + m];
            }
            if (mask) {
                if (r <= r1 && x + LC_PX - 1 <= x1 && p.mvec) {
                    const uint32_t v = *(const uint32_t *)(mask + jb.moff + px);
                    mk[0] = v & 0xffu; mk[1] = (v >> 8) & 0xffu; mk[2] = (v >> 16) & 0xffu; mk[3] = v >> 24;
                } else {
#pragma unroll
                    for (int m = 0; m < LC_PX; m++)
                        if (r <= r1 && x + m <= x1) mk[m] = mask[jb.moff + px + m];
                }
            }
#pragma unroll
            for (int m = 0; m < LC_PX; m++) {
                in[m] = r <= r1 && x + m <= x1;
                const uint32_t bits = p.be ? __builtin_bswap32(b[m]) : b[m];
                const uint32_t mag = bits & 0x7fffffffu;
                ok[m] = in[m] && mag != 0u && mag <= p.clip_bits && (mk[m] & p.skip_bits) == 0u;   // (clip is finite: inf and NaN lie above)
                q[m] = ok[m] ? lc_fix(bits) : 0ll;
            }
        }
        for (int c0 = jb.sb; c0 < jb.se; c0 += LC_CHUNK) {
            const int nc = min(LC_CHUNK, jb.se - c0);
            __syncthreads();   // (the chunk before, or the item before, has been read)
            if (tid < nc) {
                const LcSeg s = segs[c0 + tid];
                double tlo;
                S[tid] = s;
                hit[tid] = lc_box_hit(s, (double)x0, (double)x1, ya, yb, &tlo);
                // (x <= y gives fl(x * inv) <= fl(y * inv): no pixel of the tile has a section below this one)
                const double f = floor(fmax(tlo, 0.0) * s.inv);
                jlow[tid] = (int)fmin(f, (double)(s.n_sec - 1));
            }
            __syncthreads();
            for (int k = 0; k < nc; k++) {
                if (!hit[k]) continue;   // (the same for the whole block)
                const int j0 = jlow[k], nsec = S[k].n_sec, base = S[k].base;
                // the thread's two slots: sections ja and ja + 1 (a pixel of any other section goes to the sums directly)
                int ja = 0x3fffffff;                          // (no member pixel: ja + 1 must not overflow)
                int jm[LC_PX], cls[LC_PX];   // cls: 0 none, 1 core, 2 sky
#pragma unroll
                for (int m = 0; m < LC_PX; m++) {
                    const double ax = (double)(x + m) - S[k].x1, ay = yd - S[k].y1;
                    const double u = ax * S[k].nx + ay * S[k].ny;
                    const double t = ax * S[k].ex + ay * S[k].ey;
                    const bool part = in[m] && t >= 0.0 && t <= S[k].L;
                    const double au = fabs(u);
                    cls[m] = !part ? 0 : au <= S[k].half ? 1 : (au >= S[k].bg_in && au <= S[k].bg_out) ? 2 : 0;
                    jm[m] = cls[m] ? min((int)floor(t * S[k].inv), nsec - 1) : 0;
                    if (cls[m]) ja = min(ja, jm[m]);
                }
                int pk[2] = {0, 0};                          // n_geom | n_core << 10 | n_sky << 20: at most 256 each in a wave
                long long qc[2] = {0ll, 0ll}, qs[2] = {0ll, 0ll};
#pragma unroll
                for (int m = 0; m < LC_PX; m++) {
                    if (!cls[m]) continue;
                    const int d = jm[m] - ja, rel = jm[m] - j0;
                    const int add = cls[m] == 1 ? 1 + (ok[m] ? 1 << 10 : 0) : (ok[m] ? 1 << 20 : 0);
                    if (d <= 1 && rel >= 0 && rel < LC_TAB) {
                        pk[d] += add;
                        if (cls[m] == 1) qc[d] += q[m]; else qs[d] += q[m];
                    } else {                                 // (not reached while sec_len >= 8; kept so that no bound is an assumption)
                        const size_t sec = (size_t)(base + jm[m]);
                        if (cls[m] == 1) atomicAdd(cnt + 3 * sec, 1);
                        if (ok[m]) {
                            atomicAdd(cnt + 3 * sec + cls[m], 1);
                            atomicAdd(qsum + 2 * sec + (cls[m] - 1), (unsigned long long)q[m]);
                        }
                    }
                }
#pragma unroll
                for (int sl = 0; sl < 2; sl++) {
                    const int js = ja + sl;
                    unsigned long long pending = __ballot(pk[sl] != 0);
                    while (pending) {                        // (uniform over the wave)
                        const int lead = __ffsll((long long)pending) - 1;
                        const int jl = __shfl(js, lead);
                        const bool mine = pk[sl] != 0 && js == jl;
                        const int spk = lc_wave_sum(mine ? pk[sl] : 0);
                        const long long sqc = lc_wave_sum(mine ? qc[sl] : 0ll), sqs = lc_wave_sum(mine ? qs[sl] : 0ll);
                        if (lane == lead) {
                            const int rel = jl - j0;
                            if (spk & 1023) atomicAdd(&T_cnt[0][rel], spk & 1023);
                            if ((spk >> 10) & 1023) atomicAdd(&T_cnt[1][rel], (spk >> 10) & 1023);
                            if (spk >> 20) atomicAdd(&T_cnt[2][rel], spk >> 20);
                            if (sqc) atomicAdd(&T_q[0][rel], (unsigned long long)sqc);
                            if (sqs) atomicAdd(&T_q[1][rel], (unsigned long long)sqs);
                        }
                        pending &= ~__ballot(mine);
                    }
                }
                __syncthreads();
                // the table's non-zero entries: one global atomic each; the table is zero again for the next segment
                if (tid < 5 * LC_TAB) {
                    const int fld = tid / LC_TAB, rel = tid - fld * LC_TAB;
                    const size_t sec = (size_t)(base + min(j0 + rel, nsec - 1));
                    if (fld < 3) {
                        const int v = T_cnt[fld][rel];
                        if (v) { atomicAdd(cnt + 3 * sec + fld, v); T_cnt[fld][rel] = 0; }
                    } else {
                        const unsigned long long v = T_q[fld - 3][rel];
                        if (v) { atomicAdd(qsum + 2 * sec + (fld - 3), v); T_q[fld - 3][rel] = 0ull; }
                    }
                }
                __syncthreads();
            }
        }
    }
}
