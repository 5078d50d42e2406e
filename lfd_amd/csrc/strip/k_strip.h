// k_strip.h -- device side of the trail strips (include/lfdmi.h: trail strips).  Two kernels, siblings of k_lc_cull and
// k_lc_render: k_strip_cull lists the (job, tile) pairs some segment's band reaches, k_strip_render reads the pixels of the
// listed tiles once and adds them, as fixed-point integers, to the cell (section, offset bin) of every segment they belong to.
// A job is a frame that carries at least one good segment of the batch; its segments are contiguous.  Every sum is an integer
// sum: no result depends on the tiling, on the order of the list or on the order in which the atomics arrive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define STRIP_TILE_W 64
#define STRIP_TILE_H 16
#define STRIP_THREADS 256
#define STRIP_PX 4                                         // pixels of a thread: 4 neighbours of one row (one 16-byte load)
#define STRIP_COLS (STRIP_TILE_W / STRIP_PX)               // threads along a tile row
#define STRIP_CHUNK 128                                    // segments in LDS at a time
// The LDS table of one (tile, segment).  A tile's pixel centres span at most sqrt(63^2 + 15^2) = 64.8 px of t and of u: at
// sec_len >= 4 that is at most 18 sections, at step >= 0.5 at most 131 offset bins (and n_off <= 129 of them exist).  The
// offset is the fast index and the row length is odd, so neighbouring offsets are neighbouring banks and a lane that moves one
// section on moves 131 banks on.
#define STRIP_TAB_J 18
#define STRIP_TAB_B 131
#define STRIP_TAB (STRIP_TAB_J * STRIP_TAB_B)
// what the cull adds to a band's reach, and what the tile's lowest section and bin are taken below: the argument of MSK_SLACK
// (mask/k_mask.h), with half <= 64.5 px
#define STRIP_SLACK 1e-3

struct StripSeg {
    double x1, y1;              // the first end point
    double ex, ey, nx, ny;      // unit direction e and normal (-e.y, e.x)
    double half, L;             // |u| <= half, 0 <= t <= L
    double inv_s, inv_u, kc;    // section floor(t * inv_s); bin floor(u * inv_u + kc), kc = K + 0.5
    int32_t n_sec, n_off;       // sections and offset bins (2 K + 1) of the segment
    int64_t base;               // its first cell's place in the batch's cells
};

struct StripJob {
    int64_t foff;               // the frame's first pixel, in floats from the frame buffer's start
    int64_t moff;               // and in bytes from the mask buffer's start
    int32_t sb, se;             // its segments [sb, se)
};

struct StripDev {
    int32_t h, w, ntx, nty;     // the frame and its tile grid
    int32_t be;                 // frames are big-endian
    uint32_t skip_bits;         // a pixel with mask & skip_bits is invalid
    uint32_t clip_bits;         // the bits of clip (positive, finite): |v| <= clip is a comparison of the bit patterns
    int32_t vec;                // w % 4 == 0 and the frame buffer is 16-byte aligned: a thread's pixels are one load
    int32_t mvec;               // w % 4 == 0 and the mask buffer is 4-byte aligned
    int32_t pad;
};

// a cell in memory: lfdmi_strip_cell {int32 n_geom, n; int64 q}, reached as 4 ints / 2 x 64 bits
struct StripCell {
    int32_t n_geom, n;
    unsigned long long q;
};

// step 1 of the definition, as lc_fix (lc/k_lc.h): q = llrint((double)v * 2^30) of a finite v with |v| <= 1024, from its bits in
// integer arithmetic.  v = m * 2^(e - 150) with m < 2^24, so v * 2^30 = m * 2^(e - 120).
__device__ __forceinline__ long long strip_fix(uint32_t bits) {
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

// Can the segment's band hold a pixel centre of the box [xa, xb] x [ya, yb] (flipped rows)?  Conservative, as lc_box_hit.
// *tlo, *thi, *ulo, *uhi: bounds of t and of u over the box's pixel centres.
__device__ __forceinline__ bool strip_box_hit(const StripSeg &s, double xa, double xb, double ya, double yb, double *tlo, double *thi,
                                              double *ulo, double *uhi) {
    const double cx = 0.5 * (xa + xb), cy = 0.5 * (ya + yb);
    const double hx = 0.5 * (xb - xa), hy = 0.5 * (yb - ya);
    const double ax = cx - s.x1, ay = cy - s.y1;
    const double u = ax * s.nx + ay * s.ny;
    const double t = ax * s.ex + ay * s.ey;
    const double rt = hx * fabs(s.ex) + hy * fabs(s.ey) + STRIP_SLACK;
    const double ru = hx * fabs(s.nx) + hy * fabs(s.ny) + STRIP_SLACK;
    *tlo = t - rt; *thi = t + rt;
    *ulo = u - ru; *uhi = u + ru;
    if (!(fabs(u) <= s.half + ru)) return false;
    return t + rt >= 0.0 && t - rt <= s.L;
}

__device__ __forceinline__ void strip_tile_box(const StripDev &p, int tile, int &x0, int &x1, int &r0, int &r1) {
    const int ty = tile / p.ntx, tx = tile - ty * p.ntx;
    x0 = tx * STRIP_TILE_W; x1 = min(x0 + STRIP_TILE_W, p.w) - 1;
    r0 = ty * STRIP_TILE_H; r1 = min(r0 + STRIP_TILE_H, p.h) - 1;
}

// (both kernels have internal linkage: the trail subtraction, sub/, includes this header and launches its own copies)
// one thread per (job, tile): the pair is listed when any of the job's segments reaches the tile; the list's order is the order
// of arrival and no result depends on it
static __global__ void __launch_bounds__(STRIP_THREADS) k_strip_cull(const StripJob *jobs, int njobs, const StripSeg *segs, StripDev p, int2 *list,
                                                               int *count) {
    const int64_t g = (int64_t)blockIdx.x * STRIP_THREADS + threadIdx.x;
    const int ntiles = p.ntx * p.nty;
    if (g >= (int64_t)njobs * ntiles) return;
    const int job = (int)(g / ntiles), tile = (int)(g - (int64_t)job * ntiles);
    int x0, x1, r0, r1;
    strip_tile_box(p, tile, x0, x1, r0, r1);
    const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
    const StripJob jb = jobs[job];
    bool hit = false;
    double a, b, c, d;
    for (int k = jb.sb; k < jb.se && !hit; k++) hit = strip_box_hit(segs[k], (double)x0, (double)x1, ya, yb, &a, &b, &c, &d);
    if (hit) list[atomicAdd(count, 1)] = make_int2(job, tile);
}

// a run of a thread's pixels that share a cell: pk = n_geom | n << 16 (at most 4 each), q their sum.  Into the table when the cell
// lies in the window [j0, j0 + nj) x [b0, b0 + nb) the flush walks, else to memory directly (not reached at the parameter
// bounds; kept so that no bound is an assumption).
__device__ __forceinline__ void strip_add(uint32_t *T_c, unsigned long long *T_q, StripCell *cells, int64_t base, int n_off, int j, int b,
                                          int j0, int nj, int b0, int nb, uint32_t pk, long long q) {
    if (!pk) return;
    const int rj = j - j0, rb = b - b0;
    if (rj >= 0 && rj < nj && rb >= 0 && rb < nb) {
        const int at = rj * STRIP_TAB_B + rb;
        atomicAdd(T_c + at, pk);
        if (q) atomicAdd(T_q + at, (unsigned long long)q);
    } else {
        StripCell *c = cells + (base + (int64_t)j * n_off + b);
        atomicAdd(&c->n_geom, (int)(pk & 0xffffu));
        if (pk >> 16) atomicAdd(&c->n, (int)(pk >> 16));
        if (q) atomicAdd(&c->q, (unsigned long long)q);
    }
}

// Persistent blocks walk the list.  A block owns a tile: thread t owns the STRIP_PX pixels of row r0 + t / STRIP_COLS from
// column x0 + STRIP_PX (t % STRIP_COLS) on, which it loads once (16 bytes where p.vec), tests for validity and turns into q.  The
// job's segments pass through LDS in chunks of STRIP_CHUNK, each with the block's own verdict on whether it can reach the tile
// and with the window of sections and bins the tile can touch.  For a segment in hand a thread evaluates u, t, j, b of its
// pixels, adds neighbours that share a cell up in registers and adds every such run to the block's LDS table with integer
// atomics: one 32-bit add for both counts (a tile holds 1024 pixels, so 16 bits each), one 64-bit add for q.  There is no
// wave-level merge as in k_lc_render: there the lanes of a wave share one or two sections, here a cell is a section and a bin
// and the lanes of a wave that share one are few (a row of a wave is 64 px of one line, a bin is `step` px wide and a section
// sec_len px long), so the ballot loop would run nearly once per lane and cost more than the atomics it saves; only the merge
// that costs nothing is kept, the thread's own.  After a barrier the window's non-zero entries go to memory with one atomicAdd
// per count and per q.  The loops that hold a barrier are uniform over the block.
static __global__ void __launch_bounds__(STRIP_THREADS) k_strip_render(const uint32_t *frames, const uint8_t *mask, const StripJob *jobs,
                                                                 const StripSeg *segs, StripDev p, const int2 *list, const int *count,
                                                                 StripCell *cells) {
    __shared__ StripSeg S[STRIP_CHUNK];
    __shared__ int hit[STRIP_CHUNK];
    __shared__ int jlow[STRIP_CHUNK], jnum[STRIP_CHUNK], blow[STRIP_CHUNK], bnum[STRIP_CHUNK];
    __shared__ uint32_t T_c[STRIP_TAB];
    __shared__ unsigned long long T_q[STRIP_TAB];
    const int n = *count;
    const int tid = (int)threadIdx.x;
    const int col = (tid % STRIP_COLS) * STRIP_PX, row = tid / STRIP_COLS;
    for (int e = tid; e < STRIP_TAB; e += STRIP_THREADS) { T_c[e] = 0u; T_q[e] = 0ull; }
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int2 e = list[item];
        const StripJob jb = jobs[e.x];
        int x0, x1, r0, r1;
        strip_tile_box(p, e.y, x0, x1, r0, r1);
        const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
        const int x = x0 + col, r = r0 + row;
        const double yd = (double)(p.h - 1 - r);
        // the thread's pixels: in the frame?  valid?  q
        bool in[STRIP_PX], ok[STRIP_PX];
        long long q[STRIP_PX];
        {
            uint32_t b[STRIP_PX] = {0u, 0u, 0u, 0u};
            uint32_t mk[STRIP_PX] = {0u, 0u, 0u, 0u};
            const size_t px = (size_t)r * p.w + x;
            if (r <= r1 && x + STRIP_PX - 1 <= x1 && p.vec) {
                const uint4 v = *(const uint4 *)(frames + jb.foff + px);
                b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
            } else {
#pragma unroll
                for (int m = 0; m < STRIP_PX; m++)
                    if (r <= r1 && x + m <= x1) b[m] = frames[jb.foff + px + m];
            }
            if (mask) {
                if (r <= r1 && x + STRIP_PX - 1 <= x1 && p.mvec) {
                    const uint32_t v = *(const uint32_t *)(mask + jb.moff + px);
                    mk[0] = v & 0xffu; mk[1] = (v >> 8) & 0xffu; mk[2] = (v >> 16) & 0xffu; mk[3] = v >> 24;
                } else {
#pragma unroll
                    for (int m = 0; m < STRIP_PX; m++)
                        if (r <= r1 && x + m <= x1) mk[m] = mask[jb.moff + px + m];
                }
            }
#pragma unroll
            for (int m = 0; m < STRIP_PX; m++) {
                in[m] = r <= r1 && x + m <= x1;
                const uint32_t bits = p.be ? __builtin_bswap32(b[m]) : b[m];
                const uint32_t mag = bits & 0x7fffffffu;
                ok[m] = in[m] && mag != 0u && mag <= p.clip_bits && (mk[m] & p.skip_bits) == 0u;   // (clip is finite: inf and NaN lie above)
                q[m] = ok[m] ? strip_fix(bits) : 0ll;
            }
        }
        for (int c0 = jb.sb; c0 < jb.se; c0 += STRIP_CHUNK) {
            const int nc = min(STRIP_CHUNK, jb.se - c0);
            __syncthreads();   // (the chunk before, or the item before, has been read; the first time: the table is zero)
            if (tid < nc) {
                const StripSeg s = segs[c0 + tid];
                double tlo, thi, ulo, uhi;
                S[tid] = s;
                hit[tid] = strip_box_hit(s, (double)x0, (double)x1, ya, yb, &tlo, &thi, &ulo, &uhi);
                // (x <= y gives fl(x * inv) <= fl(y * inv), and the additions, floor and the clamps keep the order: no pixel of
                // the tile has a section or a bin below the window's first or above its last)
                const double top_j = (double)(s.n_sec - 1), top_b = (double)(s.n_off - 1);
                const int ja = (int)fmin(floor(fmax(tlo, 0.0) * s.inv_s), top_j);
                const int jz = (int)fmin(floor(fmax(fmin(thi, s.L), 0.0) * s.inv_s), top_j);
                const int ba = (int)fmin(fmax(floor(fmax(ulo, -s.half) * s.inv_u + s.kc), 0.0), top_b);
                const int bz = (int)fmin(fmax(floor(fmin(uhi, s.half) * s.inv_u + s.kc), 0.0), top_b);
                jlow[tid] = ja; jnum[tid] = max(0, min(STRIP_TAB_J, jz - ja + 1));
                blow[tid] = ba; bnum[tid] = max(0, min(STRIP_TAB_B, bz - ba + 1));
            }
            __syncthreads();
            for (int k = 0; k < nc; k++) {
                if (!hit[k]) continue;   // (the same for the whole block)
                const int j0 = jlow[k], nj = jnum[k], b0 = blow[k], nb = bnum[k];
                const int nsec = S[k].n_sec, noff = S[k].n_off;
                const int64_t base = S[k].base;
                int cj = -1, cb = -1;
                uint32_t pk = 0u;
                long long qs = 0ll;
#pragma unroll
                for (int m = 0; m < STRIP_PX; m++) {
                    const double ax = (double)(x + m) - S[k].x1, ay = yd - S[k].y1;
                    const double u = ax * S[k].nx + ay * S[k].ny;
                    const double t = ax * S[k].ex + ay * S[k].ey;
                    if (!(in[m] && t >= 0.0 && t <= S[k].L && fabs(u) <= S[k].half)) continue;
                    const int j = min((int)floor(t * S[k].inv_s), nsec - 1);
                    const int b = min(max((int)floor(u * S[k].inv_u + S[k].kc), 0), noff - 1);
                    if (j != cj || b != cb) {
                        strip_add(T_c, T_q, cells, base, noff, cj, cb, j0, nj, b0, nb, pk, qs);
                        cj = j; cb = b; pk = 0u; qs = 0ll;
                    }
                    pk += 1u + (ok[m] ? 1u << 16 : 0u);
                    qs += q[m];
                }
                strip_add(T_c, T_q, cells, base, noff, cj, cb, j0, nj, b0, nb, pk, qs);
                __syncthreads();
                // the window's non-zero entries: one global atomic each; the table is zero again for the next segment
                for (int e2 = tid; e2 < nj * nb; e2 += STRIP_THREADS) {
                    const int rj = e2 / nb, rb = e2 - rj * nb, at = rj * STRIP_TAB_B + rb;
                    const uint32_t v = T_c[at];
                    if (!v) continue;
                    StripCell *c = cells + (base + (int64_t)(j0 + rj) * noff + (b0 + rb));
                    atomicAdd(&c->n_geom, (int)(v & 0xffffu));
                    if (v >> 16) atomicAdd(&c->n, (int)(v >> 16));
                    const unsigned long long qv = T_q[at];
                    if (qv) atomicAdd(&c->q, qv);
                    T_c[at] = 0u; T_q[at] = 0ull;
                }
                __syncthreads();
            }
        }
    }
}
