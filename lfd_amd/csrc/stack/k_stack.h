// k_stack.h -- kernels of the stacked cross-sections (include/lfdmi.h: stacked cross-sections, steps 1, 3 and 4).
//   k_stack_block    one workgroup per (segment, half, block of <= 32 columns): the band's pixels go through LDS once -- validity
//                    test, byte swap and the bin index (double) as they are loaded -- then each lane owns bins and walks the
//                    block's columns in the defined order: a pixel reaches exactly one bin, so there is no atomic
//   k_stack_combine  one workgroup per (segment, half): the block sums in ascending block order
// The LDS tile is [column][cross offset] with an odd row stride S: x-major segments load along a (lanes on consecutive columns:
// stores S dwords apart, conflict-free for an odd S), y-major ones along b (lanes on consecutive offsets); the bin walk reads
// near-consecutive offsets of one column from consecutive lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define STK_THREADS 256
#define STK_COLS 32
#define STK_MAX_STRIDE 255   // 32 columns x 255 offsets x (value + bin) = 65280 bytes of LDS

struct StkSeg {
    double a1, b1, g, cosphi;
    double halfband;        // (P + step / 2) / cosphi: how far from bc(a) a binned pixel can lie, in b
    double wb;              // step / cosphi: a bin's extent in b
    long long frame_off;    // the frame's first element in the frames buffer
    int xmajor;
    int E;                  // cross offsets of a block's tile (<= the launch's stride)
};
struct StkItem {
    int seg, a_lo, a_hi, pad;   // columns a_lo .. a_hi of one block (at most STK_COLS of them)
};
struct StkHalf {
    int item0, n_items, out, pad;   // its blocks are items item0 .. item0 + n_items - 1; out: row of the sums / counts arrays
};
struct StkDev {
    int h, w, be, K, nb, S;
    float clip;
    double inv, kc;         // 1 / step, K + 0.5
};

__device__ __forceinline__ int stk_origin(const StkSeg &sg, const StkItem &it) {
    const double c0 = sg.b1 + sg.g * ((double)it.a_lo - sg.a1), c1 = sg.b1 + sg.g * ((double)it.a_hi - sg.a1);
    return (int)floor(fmin(c0, c1) - sg.halfband) - 2;
}

__global__ __launch_bounds__(STK_THREADS) void k_stack_block(const uint32_t *__restrict__ frames, const StkSeg *__restrict__ segs,
                                                             const StkItem *__restrict__ items, StkDev p, float *__restrict__ part_sum,
                                                             int *__restrict__ part_cnt) {
    extern __shared__ float stk_lds[];
    float *val = stk_lds;
    int *kid = (int *)(stk_lds + STK_COLS * p.S);
    const StkItem it = items[blockIdx.x];
    const StkSeg sg = segs[it.seg];
    const int ncol = min(it.a_hi - it.a_lo + 1, STK_COLS), E = min(sg.E, p.S), org = stk_origin(sg, it);
    const int A = sg.xmajor ? p.w : p.h, B = sg.xmajor ? p.h : p.w;
    const uint32_t *src = frames + sg.frame_off;
    for (int idx = threadIdx.x; idx < STK_COLS * E; idx += STK_THREADS) {
        int al, bl;
        if (sg.xmajor) { al = idx & (STK_COLS - 1); bl = idx >> 5; }
        else { al = idx / E; bl = idx - al * E; }
        if (al >= ncol) continue;
        const int a = it.a_lo + al, b = org + bl;
        int k = -1;
        float v = 0.0f;
        if (a >= 0 && a < A && b >= 0 && b < B) {
            const int x = sg.xmajor ? a : b, y = sg.xmajor ? b : a;
            uint32_t bits = src[(size_t)(p.h - 1 - y) * p.w + x];
            if (p.be) bits = __builtin_bswap32(bits);
            const float f = __uint_as_float(bits);
            if ((bits & 0x7F800000u) != 0x7F800000u && (bits & 0x7FFFFFFFu) != 0u && fabsf(f) <= p.clip) {
                const double bc = sg.b1 + sg.g * ((double)a - sg.a1);
                const double t = ((double)b - bc) * sg.cosphi * p.inv + p.kc;
                if (t >= 0.0 && t < (double)p.nb) { k = (int)t; v = f; }
            }
        }
        val[al * p.S + bl] = v;
        kid[al * p.S + bl] = k;
    }
    __syncthreads();
    // bin k of column a holds the pixels b with (b - bc) in [(k - K - 1/2) wb, (k - K + 1/2) wb) up to rounding: the window below
    // covers them with a pixel to spare on either side; what belongs to the bin is decided by the stored index alone
    const int win = (int)ceil(sg.wb) + 2;
    for (int k = threadIdx.x; k < p.nb; k += STK_THREADS) {
        float acc = 0.0f;
        int cnt = 0;
        const double lo = ((double)(k - p.K) - 0.5) * sg.wb - (double)org;
        for (int al = 0; al < ncol; al++) {
            const double bc = sg.b1 + sg.g * ((double)(it.a_lo + al) - sg.a1);
            const int f = (int)floor(bc + lo);
            for (int j = 0; j < win; j++) {
                const int bl = f + j;
                if (bl < 0 || bl >= E) continue;
                const bool hit = kid[al * p.S + bl] == k;
                // (a miss adds +0: the accumulator starts at +0 and sums of non-zero values never give -0, so it changes nothing)
                acc = acc + (hit ? val[al * p.S + bl] : 0.0f);
                cnt += hit;
            }
        }
        part_sum[(size_t)blockIdx.x * p.nb + k] = acc;
        part_cnt[(size_t)blockIdx.x * p.nb + k] = cnt;
    }
}

__global__ __launch_bounds__(STK_THREADS) void k_stack_combine(const StkHalf *__restrict__ halves, int nb, const float *__restrict__ part_sum,
                                                               const int *__restrict__ part_cnt, float *__restrict__ sums,
                                                               int *__restrict__ counts) {
    const StkHalf hf = halves[blockIdx.x];
    for (int k = threadIdx.x; k < nb; k += STK_THREADS) {
        float acc = 0.0f;
        int cnt = 0;
        for (int i = 0; i < hf.n_items; i++) {
            acc = acc + part_sum[(size_t)(hf.item0 + i) * nb + k];
            cnt += part_cnt[(size_t)(hf.item0 + i) * nb + k];
        }
        sums[(size_t)hf.out * nb + k] = acc;
        counts[(size_t)hf.out * nb + k] = cnt;
    }
}
