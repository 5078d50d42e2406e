// k_radon_null.h -- kernels of the null peaks (include/lfdmi.h: faint-trail search, null peaks, steps 17 - 22; host side in
// radon.hip).  The transform and the scoring of a scrambled frame run k_radon_first .. k_radon_finish and the short and wide
// kernels unchanged.
//   k_radon_prep_null   k_radon_prep of the scrambled frame X'[i] = X[j(i)] (step 18) that is never stored: every binned cell
//                       reads its b x b source pixels through the gather.  Slot blockIdx.z is one realisation of one frame of the
//                       chunk (its key and the frame's place come from `slots`), so the K realisations of a frame sit in
//                       neighbouring slots and gather from the same 4 H W bytes
//   k_radon_prep_scheme<SCHEME>  k_radon_prep of an in-place null frame (step 21) that is never stored: the same binning loop,
//                       validity test and accumulator, a thread per binned cell with neighbouring lanes on neighbouring
//                       columns.  SIGNFLIP reads the cell's own pixels and flips the sign bit by the pixel's hash; ROWSHIFT
//                       reads its row from column (c + o(r)) mod W on, so a wavefront's loads are consecutive addresses that
//                       wrap once; COLSHIFT reads every column from a row of its own, (r + o(c)) mod H: 4-byte loads a row
//                       stride apart
//   k_radon_null_lines  the found records of a chunk as lines for k_radon_extent (the short and wide kinds: steps 12 and 16
//                       give a found record its segment), so the call needs no wait in between; a slot without a found record
//                       gets a line whose extent is computed and ignored
#pragma once
#include "k_radon_lines.h"

struct RadonNullSlot {
    uint32_t klo, khi;      // the realisation's key k (step 17)
    int frame, pad;         // the frame's place among the chunk's frames
};

// murmur3's 32-bit finaliser
__device__ __forceinline__ uint32_t rad_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// definition step 18: the source pixel of buffer index i in a frame of npix pixels
__device__ __forceinline__ uint32_t rad_null_source(uint32_t i, uint32_t klo, uint32_t khi, uint32_t npix) {
    const uint32_t a = rad_fmix32(i * 0x9E3779B1u + klo);
    const uint32_t u = rad_fmix32(a ^ khi);
    return (uint32_t)(((uint64_t)u * npix) >> 32);      // < npix: u < 2^32
}

__global__ __launch_bounds__(RAD_THREADS) void k_radon_prep_null(const uint32_t *__restrict__ src, RadonDev p,
                                                                 const RadonNullSlot *__restrict__ slots, float *__restrict__ V,
                                                                 uint16_t *__restrict__ M) {
    const int i = blockIdx.x * RAD_THREADS + threadIdx.x, j = blockIdx.y, a = blockIdx.z;
    if (i >= p.wb) return;
    const RadonNullSlot sl = slots[a];
    const uint32_t npix = (uint32_t)p.h * (uint32_t)p.w;
    const uint32_t *fr = src + (size_t)sl.frame * npix;
    float acc = 0.0f;
    int cnt = 0;
    for (int dy = 0; dy < p.b; dy++) {
        const int y = j * p.b + dy;
        if (y >= p.h) break;
        const uint32_t row = (uint32_t)(p.h - 1 - y) * (uint32_t)p.w;
        for (int dx = 0; dx < p.b; dx++) {
            const int x = i * p.b + dx;
            if (x >= p.w) break;
            uint32_t bits = fr[rad_null_source(row + (uint32_t)x, sl.klo, sl.khi, npix)];
            if (p.be) bits = __builtin_bswap32(bits);
            const float v = __uint_as_float(bits);
            const bool valid = (bits & 0x7F800000u) != 0x7F800000u && (bits & 0x7FFFFFFFu) != 0u && fabsf(v) <= p.clip;
            acc = acc + (valid ? v : 0.0f);
            cnt += valid;
        }
    }
    const size_t o = ((size_t)a * p.hb + j) * p.wb + i;
    V[o] = acc;
    M[o] = (uint16_t)cnt;
}

// definition steps 18 and 21: u(i) of key (klo, khi)
__device__ __forceinline__ uint32_t rad_null_u(uint32_t i, uint32_t klo, uint32_t khi) {
    return rad_fmix32(rad_fmix32(i * 0x9E3779B1u + klo) ^ khi);
}

#define RADN_SIGNFLIP 1     // LFDMI_RADON_NULL_SIGNFLIP .. COLSHIFT (radon.hip asserts it)
#define RADN_ROWSHIFT 2
#define RADN_COLSHIFT 3

template <int SCHEME>
__global__ __launch_bounds__(RAD_THREADS) void k_radon_prep_scheme(const uint32_t *__restrict__ src, RadonDev p,
                                                                   const RadonNullSlot *__restrict__ slots, float *__restrict__ V,
                                                                   uint16_t *__restrict__ M) {
    static_assert(SCHEME == RADN_SIGNFLIP || SCHEME == RADN_ROWSHIFT || SCHEME == RADN_COLSHIFT, "an in-place scheme");
    const int i = blockIdx.x * RAD_THREADS + threadIdx.x, j = blockIdx.y, a = blockIdx.z;
    if (i >= p.wb) return;
    const RadonNullSlot sl = slots[a];
    const uint32_t H = (uint32_t)p.h, W = (uint32_t)p.w;
    const uint32_t *fr = src + (size_t)sl.frame * H * W;
    uint32_t oc[4] = {0, 0, 0, 0};          // COLSHIFT: o(c) of the cell's columns (b <= 4)
    if (SCHEME == RADN_COLSHIFT)
        for (int dx = 0; dx < p.b; dx++) oc[dx] = (uint32_t)(((uint64_t)rad_null_u((uint32_t)(i * p.b + dx), sl.klo, sl.khi) * H) >> 32);
    float acc = 0.0f;
    int cnt = 0;
    for (int dy = 0; dy < p.b; dy++) {
        const int y = j * p.b + dy;
        if (y >= p.h) break;
        const uint32_t r = (uint32_t)(p.h - 1 - y);
        uint32_t orow = 0;
        if (SCHEME == RADN_ROWSHIFT) orow = (uint32_t)(((uint64_t)rad_null_u(r, sl.klo, sl.khi) * W) >> 32);     // < W
        for (int dx = 0; dx < p.b; dx++) {
            const int x = i * p.b + dx;
            if (x >= p.w) break;
            uint32_t rs = r, cs = (uint32_t)x;
            if (SCHEME == RADN_ROWSHIFT) { cs += orow; cs -= cs >= W ? W : 0u; }            // x < W and o < W: one wrap at most
            if (SCHEME == RADN_COLSHIFT) { rs += oc[dx]; rs -= rs >= H ? H : 0u; }
            uint32_t bits = fr[(size_t)rs * W + cs];
            if (p.be) bits = __builtin_bswap32(bits);
            if (SCHEME == RADN_SIGNFLIP) bits ^= rad_null_u(r * W + (uint32_t)x, sl.klo, sl.khi) & 0x80000000u;
            const float v = __uint_as_float(bits);
            const bool valid = (bits & 0x7F800000u) != 0x7F800000u && (bits & 0x7FFFFFFFu) != 0u && fabsf(v) <= p.clip;
            acc = acc + (valid ? v : 0.0f);
            cnt += valid;
        }
    }
    const size_t o = ((size_t)a * p.hb + j) * p.wb + i;
    V[o] = acc;
    M[o] = (uint16_t)cnt;
}

#define RADN_STATUS 0   // where every kind's record holds these fields, in ints (radon.hip asserts it of each)
#define RADN_Q 1
#define RADN_Y0 2
#define RADN_S 3
#define RADN_SNR 6

// rec: the chunk's records, `stride` ints each, every kind's beginning with status, q, y0, s, n_pix, sum, snr; wfield: the
// place of the band's width in a record, or < 0 (then width is not written)
__global__ __launch_bounds__(RAD_THREADS) void k_radon_null_lines(const int *__restrict__ rec, int stride, int wfield, float threshold,
                                                                  int n, RadonLineDev *__restrict__ ln, int *__restrict__ width) {
    const int a = blockIdx.x * RAD_THREADS + threadIdx.x;
    if (a >= n) return;
    const int *r = rec + (size_t)a * stride;
    const bool found = r[RADN_STATUS] == 0 && __int_as_float(r[RADN_SNR]) >= threshold;
    RadonLineDev L;
    L.slot = a; L.q = found ? r[RADN_Q] : 0; L.y0 = found ? r[RADN_Y0] : 0; L.s = found ? r[RADN_S] : 0;
    ln[a] = L;
    if (wfield >= 0) width[a] = found ? r[wfield] : 1;
}
