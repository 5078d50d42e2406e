// k_rounds.h -- device side of the detection rounds (include/lfdmi.h: detection rounds).  One kernel: k_rounds_gather writes the
// work slot of every frame that continues from that frame's source, native float32, with +0 wherever the pixel centre lies in
// one of the frame's bands so far.  One pass, 4 B read and 4 B written per pixel; no slot is the source of another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RND_TILE_W 256                                     // a wave is one row of a tile: 64 lanes x 16 B = 1 KiB per access
#define RND_TILE_H 16
#define RND_THREADS 256
#define RND_WAVES (RND_THREADS / 64)
#define RND_MAX_BANDS 7                                    // LFDMI_ROUNDS_MAX_TRAILS - 1
// what the tile test adds to a band's reach: as MSK_SLACK of the trail masks (k_mask.h), whose argument holds here unchanged --
// the rounding of u at a tile's centre is below 1e-6 px for every segment the geometry accepts
#define RND_SLACK 1e-3

struct RoundsBand {
    double x1, y1;              // the first end point of the record's segment
    double ex, ey, nx, ny;      // unit direction e and normal (-e.y, e.x), from the host
    double half;
};

struct RoundsSlot {
    int64_t src;                // the frame's first pixel, in floats from the source buffer's start
    int32_t nb, pad;            // bands in use
    RoundsBand b[RND_MAX_BANDS];
};

// step 3 of the trail masks with cap = +inf: doubles, left to right, no contraction (-ffp-contract=off).  -cap and L + cap are
// -inf and +inf there, so the two tests on t are written against them.  They hold for every finite t and fail only for a NaN t,
// which the masks' expression rejects too; the host admits only finite geometry (coordinates up to 1e6), so here they guard
// nothing and cost two multiplications and an addition per pixel and band: kept so that the expression is the masks' own.
__device__ __forceinline__ bool rnd_inside(const RoundsBand &s, double x, double y) {
    const double ax = x - s.x1, ay = y - s.y1;
    const double u = ax * s.nx + ay * s.ny;
    const double t = ax * s.ex + ay * s.ey;
    return fabs(u) <= s.half && t >= -__builtin_inf() && t <= __builtin_inf();
}

// Can the band hold a pixel centre of the box [xa, xb] x [ya, yb] (flipped rows)?  Conservative, as msk_box_hit.
__device__ __forceinline__ bool rnd_box_hit(const RoundsBand &s, double xa, double xb, double ya, double yb) {
    const double cx = 0.5 * (xa + xb), cy = 0.5 * (ya + yb);
    const double hx = 0.5 * (xb - xa), hy = 0.5 * (yb - ya);
    const double u = (cx - s.x1) * s.nx + (cy - s.y1) * s.ny;
    return fabs(u) <= s.half + (hx * fabs(s.nx) + hy * fabs(s.ny) + RND_SLACK);
}

// hits: bit k set when band k can reach the tile (the same for the whole workgroup)
__device__ __forceinline__ uint32_t rnd_px(uint32_t v, bool be, uint32_t hits, const RoundsBand *B, double x, double y) {
    for (uint32_t m = hits; m; m &= m - 1)
        if (rnd_inside(B[__builtin_ctz(m)], x, y)) return 0u;   // +0.0f
    return be ? __builtin_bswap32(v) : v;
}

// grid (tiles across, tiles down, slots).  A workgroup owns the RND_TILE_W x RND_TILE_H tile (blockIdx.x, blockIdx.y) of slot
// blockIdx.z; wave v owns its rows r0 + v + RND_WAVES m.  A row of a tile is copied with 16 B accesses between its first and its
// last 16 B boundary and with 4 B accesses outside them, when source and destination sit alike in their 16 B lines; otherwise
// (frames of h * w % 4 != 0 in another slot than their index) with 4 B accesses throughout.  src == dst + slot offset is allowed
// (host frames uploaded into their slots): a thread reads and writes only its own pixels.
__global__ void __launch_bounds__(RND_THREADS) k_rounds_gather(const uint32_t *src, uint32_t *dst, const RoundsSlot *slots, int h, int w, int be) {
    __shared__ RoundsBand B[RND_MAX_BANDS];
    __shared__ int hit[RND_MAX_BANDS];
    const RoundsSlot *sl = slots + blockIdx.z;
    const int nb = min(sl->nb, RND_MAX_BANDS);
    const int x0 = blockIdx.x * RND_TILE_W, x1 = min(x0 + RND_TILE_W, w);          // columns [x0, x1)
    const int r0 = blockIdx.y * RND_TILE_H, r1 = min(r0 + RND_TILE_H, h);          // buffer rows [r0, r1)
    if ((int)threadIdx.x < nb) {
        const RoundsBand s = sl->b[threadIdx.x];
        B[threadIdx.x] = s;
        hit[threadIdx.x] = rnd_box_hit(s, (double)x0, (double)(x1 - 1), (double)(h - r1), (double)(h - 1 - r0));
    }
    __syncthreads();
    uint32_t hits = 0;
    for (int k = 0; k < nb; k++) hits |= hit[k] ? 1u << k : 0u;
    const size_t N = (size_t)h * w;
    const uint32_t *sp = src + sl->src;
    uint32_t *dp = dst + (size_t)blockIdx.z * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool swap = be != 0;
    for (int r = r0 + wave; r < r1; r += RND_WAVES) {
        const uint32_t *s = sp + (size_t)r * w;
        uint32_t *d = dp + (size_t)r * w;
        const double y = (double)(h - 1 - r);
        const int sa = (int)(((uintptr_t)(s + x0) >> 2) & 3), da = (int)(((uintptr_t)(d + x0) >> 2) & 3);
        if (sa != da) {
            for (int x = x0 + lane; x < x1; x += 64) d[x] = rnd_px(s[x], swap, hits, B, (double)x, y);
            continue;
        }
        const int xa = min(x1, x0 + ((4 - sa) & 3));        // the first column on a 16 B boundary
        const int xb = xa + ((x1 - xa) & ~3);                // the end of the last whole 16 B
        if (lane < xa - x0) d[x0 + lane] = rnd_px(s[x0 + lane], swap, hits, B, (double)(x0 + lane), y);
        if (lane < x1 - xb) d[xb + lane] = rnd_px(s[xb + lane], swap, hits, B, (double)(xb + lane), y);
        for (int x = xa + 4 * lane; x < xb; x += 256) {
            uint4 v = *(const uint4 *)(s + x);
            v.x = rnd_px(v.x, swap, hits, B, (double)x, y);
            v.y = rnd_px(v.y, swap, hits, B, (double)(x + 1), y);
            v.z = rnd_px(v.z, swap, hits, B, (double)(x + 2), y);
            v.w = rnd_px(v.w, swap, hits, B, (double)(x + 3), y);
            *(uint4 *)(d + x) = v;
        }
    }
}
