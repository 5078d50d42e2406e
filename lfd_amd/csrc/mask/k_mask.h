// k_mask.h -- device side of the trail masks (include/lfdmi.h: trail masks).  Two kernels: k_mask_cull lists the (job, tile)
// pairs some segment's band reaches, k_mask_render flags (and fills) the pixels of the listed tiles and counts them.  A job is a
// frame that carries at least one good segment; its segments are contiguous and in ascending index order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MSK_TILE_W 64
#define MSK_TILE_H 16
#define MSK_THREADS 256
#define MSK_WAVES (MSK_THREADS / MSK_TILE_W)               // a wave is one row of a tile
#define MSK_ROWS (MSK_TILE_H / MSK_WAVES)                  // rows of a tile per thread
#define MSK_CHUNK 128                                      // segments in LDS at a time
// What the cull adds to a band's reach.  It compares u and t of a tile's centre with the band; a pixel centre's u and t differ
// from the tile centre's by at most the half extent in exact arithmetic, and the rounding of either is a few ulp of
// max(|x1|, |y1|, w + h) <= 1e9, below 1e-6 px.  half may be any finite double, and half + (reach + slack) rounds at half's
// magnitude: where that rounding exceeds the slack, half itself dwarfs every |u| <= 2e9 + 1e6 of a frame and the test passes
// either way; below that the sum is at least half + reach + slack / 2.  So no tile the cull drops has a pixel inside a band.
#define MSK_SLACK 1e-3

enum { MSK_FILL_NONE = 0, MSK_FILL_ZERO = 1, MSK_FILL_NAN = 2, MSK_FILL_VALUE = 3 };

struct MaskSeg {
    double x1, y1;              // the first end point
    double ex, ey, nx, ny;      // unit direction e and normal (-e.y, e.x)
    double half, lo, hi;        // the band: |u| <= half, lo <= t <= hi (lo = -cap, hi = L + cap)
    float fill;
    uint32_t bits;
};

struct MaskJob {
    int64_t foff;               // the frame's first pixel, in floats from the frame buffer's start
    int64_t moff;               // and in bytes from the mask buffer's start
    int32_t sb, se;             // its segments [sb, se)
};

struct MaskDev {
    int32_t h, w, ntx, nty;     // the frame and its tile grid
    int32_t fill_mode, pad;
};

// step 3 of the definition: doubles, left to right, no contraction (-ffp-contract=off)
__device__ __forceinline__ bool msk_inside(const MaskSeg &s, double x, double y) {
    const double ax = x - s.x1, ay = y - s.y1;
    const double u = ax * s.nx + ay * s.ny;
    const double t = ax * s.ex + ay * s.ey;
    return fabs(u) <= s.half && t >= s.lo && t <= s.hi;
}

// Can the segment's band hold a pixel centre of the box [xa, xb] x [ya, yb] (flipped rows)?  Conservative.
__device__ __forceinline__ bool msk_box_hit(const MaskSeg &s, double xa, double xb, double ya, double yb) {
    const double cx = 0.5 * (xa + xb), cy = 0.5 * (ya + yb);
    const double hx = 0.5 * (xb - xa), hy = 0.5 * (yb - ya);
    const double ax = cx - s.x1, ay = cy - s.y1;
    const double u = ax * s.nx + ay * s.ny;
    if (!(fabs(u) <= s.half + (hx * fabs(s.nx) + hy * fabs(s.ny) + MSK_SLACK))) return false;
    const double t = ax * s.ex + ay * s.ey;
    const double rt = hx * fabs(s.ex) + hy * fabs(s.ey) + MSK_SLACK;
    return t + rt >= s.lo && t - rt <= s.hi;
}

__device__ __forceinline__ void msk_tile_box(const MaskDev &p, int tile, int &x0, int &x1, int &r0, int &r1) {
    const int ty = tile / p.ntx, tx = tile - ty * p.ntx;
    x0 = tx * MSK_TILE_W; x1 = min(x0 + MSK_TILE_W, p.w) - 1;
    r0 = ty * MSK_TILE_H; r1 = min(r0 + MSK_TILE_H, p.h) - 1;
}

// one thread per (job, tile): the pair is listed when any of the job's segments reaches the tile.  The order of the list is the
// order of arrival; no result depends on it (a tile is rendered by one block, whichever comes to it).
__global__ void __launch_bounds__(MSK_THREADS) k_mask_cull(const MaskJob *jobs, int njobs, const MaskSeg *segs, MaskDev p, int2 *list,
                                                          int *count) {
    const int64_t g = (int64_t)blockIdx.x * MSK_THREADS + threadIdx.x;
    const int ntiles = p.ntx * p.nty;
    if (g >= (int64_t)njobs * ntiles) return;
    const int job = (int)(g / ntiles), tile = (int)(g - (int64_t)job * ntiles);
    int x0, x1, r0, r1;
    msk_tile_box(p, tile, x0, x1, r0, r1);
    const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
    const MaskJob jb = jobs[job];
    bool hit = false;
    for (int k = jb.sb; k < jb.se && !hit; k++) hit = msk_box_hit(segs[k], (double)x0, (double)x1, ya, yb);
    if (hit) list[atomicAdd(count, 1)] = make_int2(job, tile);
}

// Persistent blocks walk the list.  A block owns a tile: thread (lane, wave) owns the pixels of column x0 + lane in rows
// r0 + wave + MSK_WAVES m.  The job's segments pass through LDS in chunks of MSK_CHUNK, in index order, each with the block's
// own verdict on whether it can reach the tile; a thread ORs the bits of the segments that hold its pixels and keeps the fill
// of the first one.  Every loop and every ballot is uniform over the block: a thread outside the frame only votes "outside".
// seg_counts[k]: pixels inside segment k (one atomicAdd per wave and segment); job_counts[j]: pixels of job j inside any.
__global__ void __launch_bounds__(MSK_THREADS) k_mask_render(float *frames, uint8_t *mask, const MaskJob *jobs, const MaskSeg *segs, MaskDev p,
                                                            const int2 *list, const int *count, int *seg_counts, int *job_counts) {
    __shared__ MaskSeg S[MSK_CHUNK];
    __shared__ int hit[MSK_CHUNK];
    const int n = *count;
    const int lane = threadIdx.x & (MSK_TILE_W - 1), wave = threadIdx.x / MSK_TILE_W;
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int2 e = list[item];
        const MaskJob jb = jobs[e.x];
        int x0, x1, r0, r1;
        msk_tile_box(p, e.y, x0, x1, r0, r1);
        const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
        const int x = x0 + lane;
        const double xd = (double)x;
        uint32_t bits[MSK_ROWS];
        float fill[MSK_ROWS];
#pragma unroll
        for (int m = 0; m < MSK_ROWS; m++) { bits[m] = 0; fill[m] = 0.0f; }
        for (int c0 = jb.sb; c0 < jb.se; c0 += MSK_CHUNK) {
            const int nc = min(MSK_CHUNK, jb.se - c0);
            __syncthreads();   // (the chunk before, or the item before, has been read)
            if ((int)threadIdx.x < nc) {
                const MaskSeg s = segs[c0 + threadIdx.x];
                S[threadIdx.x] = s;
                hit[threadIdx.x] = msk_box_hit(s, (double)x0, (double)x1, ya, yb);
            }
            __syncthreads();
            for (int k = 0; k < nc; k++) {
                if (!hit[k]) continue;   // (the same for the whole block)
                int cnt = 0;
#pragma unroll
                for (int m = 0; m < MSK_ROWS; m++) {
                    const int r = r0 + wave + m * MSK_WAVES;
                    const bool in = x <= x1 && r <= r1 && msk_inside(S[k], xd, (double)(p.h - 1 - r));
                    if (in) {
                        if (!bits[m]) fill[m] = S[k].fill;
                        bits[m] |= S[k].bits;
                    }
                    cnt += __popcll(__ballot(in));
                }
                if (lane == 0 && cnt) atomicAdd(seg_counts + c0 + k, cnt);
            }
        }
        int cnt = 0;
#pragma unroll
        for (int m = 0; m < MSK_ROWS; m++) {
            const bool in = bits[m] != 0;   // (bits of a segment are never 0)
            if (in) {
                const size_t px = (size_t)(r0 + wave + m * MSK_WAVES) * p.w + x;
                if (mask) mask[jb.moff + px] |= (uint8_t)bits[m];
                if (p.fill_mode == MSK_FILL_ZERO) frames[jb.foff + px] = 0.0f;
                else if (p.fill_mode == MSK_FILL_NAN) frames[jb.foff + px] = __uint_as_float(0x7fc00000u);
                else if (p.fill_mode == MSK_FILL_VALUE) frames[jb.foff + px] = fill[m];
            }
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0 && cnt) atomicAdd(job_counts + e.x, cnt);
    }
}
