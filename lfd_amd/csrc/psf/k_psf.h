// k_psf.h -- kernels of the frame seeing (include/lfdmi.h: frame seeing).
//   k_psf_measure  one wavefront per record of the source finder, four to a workgroup: the status rules in their order (every
//                  lane reads the same record, so each branch is uniform over the wave), the crowding test with a lane per
//                  other record, then the (2 (win + gap + ring) + 1)^2 square row by row with neighbouring lanes on neighbouring
//                  columns (at most 65 columns: lane 0 takes the 65th), the byte swap and the validity test as a pixel is loaded,
//                  q by psf_fix.  A lane keeps seven int64 sums of the raw q (ring; window: 1, dx, dy, dx^2, dy^2, dx dy) in
//                  registers; they are added across the wave by shuffles, and lane 0 subtracts b times the window's own
//                  sums of 1, dx^2 and dy^2 (those of dx, dy and dx dy are 0), which is sum (q - b) f exactly.
//   k_psf_pack     one workgroup per frame: the OK records in record order by ballot and prefix count, the first max_used of
//                  them copied out, the count of every status.
// No atomic, no transcendental, no float arithmetic beyond the comparison of s_peak with its floor.  The square is not kept:
// neither LDS nor more registers than the seven sums are needed, since b enters the sums linearly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>


#define PSF_THREADS 256
#define PSF_WAVES (PSF_THREADS / 64)
#define PSF_OK 0
#define PSF_NOT_CANDIDATE 1
#define PSF_CLIPPED 2
#define PSF_CROWDED 3
#define PSF_BAD_PIXEL 4
#define PSF_STATUSES 5
#define PSF_NONE 255                            // a slot past the frame's n_out

struct PsfDev {
    int32_t h, w, be, max_obj;
    int32_t win, gap, ring, iso, rad_max, max_used;
    uint32_t sat_bits;                          // the bits of sat (positive, finite): |v| <= sat compares the bit patterns
    int32_t pad;
};
struct PsfStarRec {                             // lfdmi_star
    int32_t x, y, rad, flags;
    float s_peak, flux, xc, yc;
};
struct PsfStarDev {                             // lfdmi_psf_star
    int32_t index, n_ring;
    long long Q0, Qx, Qy, Qxx, Qyy, Qxy, Q_ring;
};
struct PsfFrameDev {
    int32_t n_ok, n_packed;
    int32_t count[PSF_STATUSES];
    int32_t pad;
};

// q = llrint((double)v * 2^30) of a finite v, as lc_fix (lc/k_lc.h) and strip_fix (strip/k_strip.h) have it, from its bits in
// integer arithmetic (exact; it does not depend on a denormal mode).  v = m * 2^(e - 150) with m < 2^24, so v * 2^30 =
// m * 2^(e - 120); here |v| <= 4096, so e <= 139 and |q| <= 2^42.
__device__ __forceinline__ long long psf_fix(uint32_t bits) {
    const int e = (int)((bits >> 23) & 0xffu);
    const long long m = (long long)(bits & 0x7fffffu) | (e ? 0x800000ll : 0ll);
    const int sh = (e ? e : 1) - 120;
    long long q;
    if (sh >= 0) q = m << sh;
    else if (sh < -25) q = 0;                               // (m * 2^-26 < 1/4)
    else {
        const int s = -sh;
        q = (m + ((1ll << (s - 1)) - 1) + ((m >> s) & 1)) >> s;   // ties to even
    }
    return (bits >> 31) ? -q : q;
}

// the sum of v over the lanes of a wave, in every lane (integers: the order does not matter)
__device__ __forceinline__ int psf_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ long long psf_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(PSF_THREADS) void k_psf_measure(const uint32_t *__restrict__ frames, size_t N, PsfDev p,
                                                             const PsfStarRec *__restrict__ recs, const int *__restrict__ n_out,
                                                             const float *__restrict__ peak_floor, uint8_t *__restrict__ status,
                                                             PsfStarDev *__restrict__ sums) {
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * PSF_WAVES + (threadIdx.x >> 6);
    if (i >= p.max_obj) return;                 // (the same for the whole wave, as every branch below)
    const size_t slot = (size_t)f * p.max_obj + i;
    const int cnt = min(max(n_out[f], 0), p.max_obj);
    if (i >= cnt) {
        if (lane == 0) status[slot] = PSF_NONE;
        return;
    }
    const PsfStarRec *fr = recs + (size_t)f * p.max_obj;
    const PsfStarRec r = fr[i];
    const int H = p.win + p.gap + p.ring;       // at most 32
    int st = PSF_OK;
    if (r.flags != 0 || r.rad == 0 || r.rad > p.rad_max || !(r.s_peak >= peak_floor[f])) st = PSF_NOT_CANDIDATE;
    else if (r.x < H || r.x > p.w - 1 - H || r.y < H || r.y > p.h - 1 - H) st = PSF_CLIPPED;   // (w, h >= 1 and H >= 0: no overflow)
    else {
        bool near = false;
        for (int j = lane; j < cnt; j += 64) {
            if (j == i) continue;
            const long long dx = (long long)fr[j].x - r.x, dy = (long long)fr[j].y - r.y;
            const long long d = max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy);
            near = near || d <= (long long)p.iso;
        }
        if (__ballot(near)) st = PSF_CROWDED;
    }
    long long qr = 0, q0 = 0, qx = 0, qy = 0, qxx = 0, qyy = 0, qxy = 0;
    if (st == PSF_OK) {
        const uint32_t *src = frames + (size_t)f * N;
        const int side = 2 * H + 1, inner = p.win + p.gap;
        bool bad = false;
        for (int ry = 0; ry < side; ry++) {
            const int dy = ry - H;
            const uint32_t *row = src + (size_t)(r.y + dy) * p.w + (r.x - H);   // (the square lies in the frame: not CLIPPED)
            for (int c = lane; c < side; c += 64) {
                uint32_t bits = row[c];
                if (p.be) bits = __builtin_bswap32(bits);
                const uint32_t mag = bits & 0x7fffffffu;
                if (mag == 0u || mag > p.sat_bits) { bad = true; continue; }   // (sat is finite: inf and NaN lie above)
                const long long q = psf_fix(bits);
                const int dx = c - H, d = max(abs(dx), abs(dy));
                if (d > inner) qr += q;
                else if (d <= p.win) {
                    q0 += q; qx += q * dx; qy += q * dy;
                    qxx += q * (dx * dx); qyy += q * (dy * dy); qxy += q * (dx * dy);
                }
            }
        }
        if (__ballot(bad)) st = PSF_BAD_PIXEL;
    }
    if (st == PSF_OK) {
        qr = psf_wave_sum(qr); q0 = psf_wave_sum(q0); qx = psf_wave_sum(qx); qy = psf_wave_sum(qy);
        qxx = psf_wave_sum(qxx); qyy = psf_wave_sum(qyy); qxy = psf_wave_sum(qxy);
    }
    if (lane != 0) return;
    status[slot] = (uint8_t)st;
    if (st != PSF_OK) return;
    const int side = 2 * H + 1, core = 2 * (p.win + p.gap) + 1, ww = 2 * p.win + 1;
    const int n_ring = side * side - core * core;                    // ring >= 1: never 0
    const long long b = qr / n_ring;                                 // truncates, as C divides
    const long long s2 = (long long)ww * (p.win * (p.win + 1) * ww / 3);   // sum of dx^2 (of dy^2) over the window
    PsfStarDev o;
    o.index = i; o.n_ring = n_ring;
    o.Q0 = q0 - b * ((long long)ww * ww);
    o.Qx = qx; o.Qy = qy;
    o.Qxx = qxx - b * s2; o.Qyy = qyy - b * s2;
    o.Qxy = qxy;
    o.Q_ring = qr;
    sums[slot] = o;
}

__global__ __launch_bounds__(PSF_THREADS) void k_psf_pack(PsfDev p, const int *__restrict__ n_out, const uint8_t *__restrict__ status,
                                                          const PsfStarDev *__restrict__ sums, PsfStarDev *__restrict__ out,
                                                          PsfFrameDev *__restrict__ frec) {
    __shared__ int wtot[PSF_WAVES];
    __shared__ int ctot[PSF_WAVES][PSF_STATUSES];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cnt = min(max(n_out[f], 0), p.max_obj);
    const size_t base = (size_t)f * p.max_obj;
    int mine[PSF_STATUSES] = {0, 0, 0, 0, 0};
    int done = 0;                               // OK records before this round (the same in every thread)
    for (int i0 = 0; i0 < cnt; i0 += PSF_THREADS) {   // (uniform over the block: the barriers are reached by all)
        const int i = i0 + (int)threadIdx.x;
        const int st = i < cnt ? (int)status[base + i] : PSF_NONE;
        if (st < PSF_STATUSES) mine[st]++;
        const bool ok = st == PSF_OK;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int pos = done + __popcll(m & ((1ull << lane) - 1ull));
        int all = 0;
        for (int k = 0; k < PSF_WAVES; k++) {
            if (k < wv) pos += wtot[k];
            all += wtot[k];
        }
        if (ok && pos < p.max_used) out[(size_t)f * p.max_used + pos] = sums[base + i];
        done += all;
        __syncthreads();                        // (wtot is written again in the next round)
    }
#pragma unroll
    for (int k = 0; k < PSF_STATUSES; k++) {
        const int s = psf_wave_sum(mine[k]);
        if (lane == 0) ctot[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PsfFrameDev o;
        for (int k = 0; k < PSF_STATUSES; k++) {
            int s = 0;
            for (int v = 0; v < PSF_WAVES; v++) s += ctot[v][k];
            o.count[k] = s;
        }
        o.n_ok = done;
        o.n_packed = min(done, p.max_used);
        o.pad = 0;
        frec[f] = o;
    }
}
