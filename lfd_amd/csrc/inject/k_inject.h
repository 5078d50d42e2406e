// k_inject.h -- device side of the trail injection (include/lfdmi.h: trail injection).  Two kernels: k_inject_cull lists the
// (job, tile) pairs some trail's band reaches, k_inject_render adds the trails to the pixels of the listed tiles.  A job is a
// frame that carries at least one trail; its trails are contiguous and in ascending index order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define INJ_TILE_W 64
#define INJ_TILE_H 16
#define INJ_THREADS 256
#define INJ_ROWS (INJ_TILE_W * INJ_TILE_H / INJ_THREADS)   // rows of a tile per thread
#define INJ_MAX_TABLE 4097
// What the culls add to a band's half-width.  They compare u and t of a tile's (or pixel's) centre with the band; a sample
// point's u and t differ from the centre's by at most the half extent in exact arithmetic, and the rounding of either is a few
// ulp of max(|rho|, w + h) <= 1e9, below 1e-6 px.  So nothing a cull drops has a sample inside a band.
#define INJ_SLACK 1e-3

struct InjTrail {
    double c, s, rho, fx, fy;   // the line: normal (c, s), foot point f; the direction is (-s, c)
    double t0, t1;              // -inf / +inf when unbounded
    double amp;
    int32_t table, bounded;     // bounded: t0 or t1 is finite
};

struct InjJob {
    int64_t off;                // the frame's first pixel, in floats from the buffer's start
    int32_t tb, te;             // its trails [tb, te)
};

struct InjDev {
    int32_t h, w, ntx, nty;     // the frame and its tile grid
    int32_t ss, M, table_len, pad;
    double step, halfw;         // table_step; M * table_step
    double ss2;                 // (double)(ss * ss)
    double off[8];              // o_m = (m + 1/2) / ss - 1/2
};

// Does the trail's band reach the box of sample points around the pixels [xa, xb] x [ya, yb] (flipped rows)?
__device__ __forceinline__ bool inj_box_hit(const InjTrail &t, double xa, double xb, double ya, double yb, double halfw) {
    const double cx = 0.5 * (xa + xb), cy = 0.5 * (ya + yb);
    const double hx = 0.5 * (xb - xa) + 0.5, hy = 0.5 * (yb - ya) + 0.5;
    const double ac = fabs(t.c), as = fabs(t.s);
    const double u = cx * t.c + cy * t.s - t.rho;
    if (!(fabs(u) <= halfw + hx * ac + hy * as + INJ_SLACK)) return false;
    if (!t.bounded) return true;
    const double tt = (cx - t.fx) * -t.s + (cy - t.fy) * t.c;
    const double rt = hx * as + hy * ac + INJ_SLACK;
    return tt + rt >= t.t0 && tt - rt <= t.t1;
}

__device__ __forceinline__ void inj_tile_box(const InjDev &p, int tile, int &x0, int &x1, int &r0, int &r1) {
    const int ty = tile / p.ntx, tx = tile - ty * p.ntx;
    x0 = tx * INJ_TILE_W; x1 = min(x0 + INJ_TILE_W, p.w) - 1;
    r0 = ty * INJ_TILE_H; r1 = min(r0 + INJ_TILE_H, p.h) - 1;
}

// one thread per (job, tile): the pair is listed when any of the job's trails reaches the tile.  The order of the list is the
// order of arrival; no result depends on it (a tile is rendered by one block, whichever comes to it).
__global__ void __launch_bounds__(INJ_THREADS) k_inject_cull(const InjJob *jobs, int njobs, const InjTrail *trails, InjDev p, int2 *list,
                                                            int *count) {
    const int64_t g = (int64_t)blockIdx.x * INJ_THREADS + threadIdx.x;
    const int ntiles = p.ntx * p.nty;
    if (g >= (int64_t)njobs * ntiles) return;
    const int job = (int)(g / ntiles), tile = (int)(g - (int64_t)job * ntiles);
    int x0, x1, r0, r1;
    inj_tile_box(p, tile, x0, x1, r0, r1);
    const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
    const InjJob jb = jobs[job];
    bool hit = false;
    for (int k = jb.tb; k < jb.te && !hit; k++) hit = inj_box_hit(trails[k], (double)x0, (double)x1, ya, yb, p.halfw);
    if (hit) list[atomicAdd(count, 1)] = make_int2(job, tile);
}

// The trail's contribution to pixel (x, yf) (yf: the flipped row), steps 3 and 4 of the definition.  T: the table in LDS, 2M+2
// nodes (the last one repeats node 2M).
__device__ __forceinline__ float inj_pixel_add(const InjTrail &t, const InjDev &p, const float *T, double x, double yf) {
    const double dx = -t.s, dy = t.c, top = (double)(2 * p.M);
    double acc = 0.0;
    for (int i = 0; i < p.ss; i++) {
        const double py = yf + p.off[i];
        const double pys = py * t.s, tys = (py - t.fy) * dy;
        for (int j = 0; j < p.ss; j++) {
            const double px = x + p.off[j];
            if (t.bounded) {
                const double tt = (px - t.fx) * dx + tys;
                if (tt < t.t0 || tt > t.t1) continue;
            }
            const double u = px * t.c + pys - t.rho;
            const double q = u / p.step + (double)p.M;
            if (!(q >= 0.0 && q <= top)) continue;
            const double kf = floor(q);
            const float a = (float)(q - kf);
            const int k = (int)kf;
            const float lo = T[k], hi = T[k + 1];
            acc += (double)(lo + a * (hi - lo));
        }
    }
    return (float)(t.amp * acc / p.ss2);
}

// Persistent blocks walk the list.  A block owns a tile: thread (lane, wave) owns the pixels of column x0 + lane in rows
// r0 + wave + 4 m, loops over the job's trails in index order and keeps its pixels in registers; a pixel is loaded when the first
// non-zero addend arrives and stored only then.  No atomics, and nothing is written where no trail adds.
__global__ void __launch_bounds__(INJ_THREADS) k_inject_render(float *frames, const InjJob *jobs, const InjTrail *trails, const float *tables,
                                                              InjDev p, const int2 *list, const int *count) {
    __shared__ float T[INJ_MAX_TABLE + 1];
    const int n = *count;
    const int lane = threadIdx.x & (INJ_TILE_W - 1), wave = threadIdx.x / INJ_TILE_W;
    int cur = -1;   // the table in LDS (the same for every thread of the block)
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int2 e = list[item];
        const InjJob jb = jobs[e.x];
        int x0, x1, r0, r1;
        inj_tile_box(p, e.y, x0, x1, r0, r1);
        const double ya = (double)(p.h - 1 - r1), yb = (double)(p.h - 1 - r0);
        const int x = x0 + lane;
        float v[INJ_ROWS];
        unsigned loaded = 0;
        for (int k = jb.tb; k < jb.te; k++) {
            const InjTrail t = trails[k];
            if (!inj_box_hit(t, (double)x0, (double)x1, ya, yb, p.halfw)) continue;   // (the same for the whole block)
            if (t.table != cur) {
                __syncthreads();
                for (int i = threadIdx.x; i <= p.table_len; i += INJ_THREADS)
                    T[i] = tables[(size_t)t.table * p.table_len + min(i, p.table_len - 1)];
                cur = t.table;
                __syncthreads();
            }
            if (x > x1) continue;
#pragma unroll
            for (int m = 0; m < INJ_ROWS; m++) {
                const int r = r0 + wave + m * (INJ_THREADS / INJ_TILE_W);
                if (r > r1) continue;
                const double xd = (double)x, yf = (double)(p.h - 1 - r);
                if (!inj_box_hit(t, xd, xd, yf, yf, p.halfw)) continue;
                const float add = inj_pixel_add(t, p, T, xd, yf);
                if (add != 0.0f) {
                    float *px = frames + jb.off + (size_t)r * p.w + x;
                    if (!(loaded >> m & 1)) { v[m] = *px; loaded |= 1u << m; }
                    v[m] = v[m] + add;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < INJ_ROWS; m++)
            if (loaded >> m & 1) frames[jb.off + (size_t)(r0 + wave + m * (INJ_THREADS / INJ_TILE_W)) * p.w + x] = v[m];
    }
}
