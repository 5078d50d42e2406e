// k_sky.h -- kernels of the sky normalisation (include/lfdmi.h: sky normalisation; host side in sky.hip).
//   k_sky_cells   one workgroup per (frame, mesh cell): the clipped median / MAD of the cell, every statistic an exact radix select
//   k_sky_mesh    one workgroup per frame: frame values, empty-cell fill, 3 x 3 median filter, the record
//   k_sky_apply   out = (x - bkg) * gain at copy rate; bkg bilinear between cell centres
// Built with -ffp-contract=off: every float operation below is rounded on its own, as the definition says.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SKY_THREADS 256
#define SKY_LDS_MAX 16384   // cell pixels kept in LDS (128 x 128 x 4 B = 64 KB); larger cells are re-read through L2
#define SKY_ROW_SPLIT 4     // k_sky_apply: workgroups per (column span, mesh row interval), rows interleaved

struct SkyDev {
    int h, w, cell, ny, nx, n_clip, filter, mode, be;
    double k_clip, target_sigma;
};
struct SkyRec {
    int status, n_empty;
    float sky, sigma, gain;
    int pad;
};

__device__ __forceinline__ uint32_t sky_bswap(uint32_t v) { return __builtin_bswap32(v); }
// order-preserving key of a float (not NaN): ascending keys = ascending values
__device__ __forceinline__ uint32_t sky_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sky_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// the pixel as the statistics see it: false for NaN / Inf; -0 counts as +0 (the two compare equal, a selection must not tell them apart)
__device__ __forceinline__ bool sky_pixel(uint32_t bits, int be, float &v) {
    if (be) bits = sky_bswap(bits);
    if ((bits & 0x7F800000u) == 0x7F800000u) return false;
    if (bits == 0x80000000u) bits = 0u;
    v = __uint_as_float(bits);
    return true;
}

struct SkySel {
    int hist[256];
    unsigned kmin, kmax;
    int m, digit, rank;
};

// Lower median (rank (m-1)/2) of the keys get(i, key) reports live for i in [0, n), by all SKY_THREADS threads of the workgroup.
// Returns the live count m (0: *out untouched).  The keys are first reduced to their range [kmin, kmax]: the radix passes (8 bits
// each, LDS histogram atomics) then start at the highest bit in which the live keys differ, which for sky pixels of one cell
// leaves two or three passes of the four and spreads the first of them over the histogram instead of one hot bin.
template <class F>
__device__ int sky_select(F get, int n, SkySel &s, uint32_t *out) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid == 0) { s.kmin = 0xFFFFFFFFu; s.kmax = 0u; s.m = 0; }
    __syncthreads();
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    int c = 0;
    for (int i = tid; i < n; i += SKY_THREADS) {
        uint32_t k;
        if (get(i, k)) { mn = min(mn, k); mx = max(mx, k); c++; }
    }
    for (int off = 32; off; off >>= 1) {
        mn = min(mn, (unsigned)__shfl_xor((int)mn, off));
        mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
        c += __shfl_xor(c, off);
    }
    if ((tid & 63) == 0 && c) { atomicMin(&s.kmin, mn); atomicMax(&s.kmax, mx); atomicAdd(&s.m, c); }
    __syncthreads();
    const int m = s.m;
    if (m == 0) return 0;
    const unsigned kmin = s.kmin, range = s.kmax - kmin;
    int rem = range ? 32 - __clz(range) : 0;   // bits of (key - kmin) not yet decided
    unsigned prefix = 0;
    int r = (m - 1) >> 1;
    while (rem > 0) {
        const int wd = min(8, rem), shift = rem - wd;
        const unsigned dmask = (1u << wd) - 1u;
        s.hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SKY_THREADS) {
            uint32_t k;
            if (get(i, k)) {
                const unsigned d = k - kmin;
                if (rem >= 32 || (d >> rem) == (prefix >> rem)) atomicAdd(&s.hist[(d >> shift) & dmask], 1);
            }
        }
        __syncthreads();
        if (tid < 64) {   // one wave: 4 bins per lane, inclusive scan across lanes; exactly one lane holds the rank
            const int c0 = s.hist[4 * tid], c1 = s.hist[4 * tid + 1], c2 = s.hist[4 * tid + 2], c3 = s.hist[4 * tid + 3];
            const int tot = c0 + c1 + c2 + c3;
            int inc = tot;
            for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(inc, off); if (tid >= off) inc += t; }
            const int exc = inc - tot;
            if (r >= exc && r < inc) {
                int rr = r - exc, d = 4 * tid;
                if (rr >= c0) { rr -= c0; d++; if (rr >= c1) { rr -= c1; d++; if (rr >= c2) { rr -= c2; d++; } } }
                s.digit = d;
                s.rank = rr;
            }
        }
        __syncthreads();
        prefix |= (unsigned)s.digit << shift;
        r = s.rank;
        rem = shift;
    }
    *out = kmin + prefix;
    return m;
}

// The pixels of one cell: float bits in LDS (finite ones only, -0 as +0, any order), or the cell itself in global memory.
struct SkyCellSrc {
    const uint32_t *lds;   // non-NULL: the LDS copy
    const uint32_t *g;     // the cell's first pixel
    int w, cw, be;
    double lo, hi;         // the running clip interval
    __device__ __forceinline__ bool value(int i, float &v) const {
        if (lds) v = __uint_as_float(lds[i]);
        else {
            const int r = i / cw, c = i - r * cw;
            if (!sky_pixel(g[(size_t)r * w + c], be, v)) return false;
        }
        const double d = (double)v;
        return d >= lo && d <= hi;
    }
};

// cb / cs: the cell's b and s (definition step 2); ne: 1 when the cell is not empty.  grid (nx, ny, frames).
__global__ void __launch_bounds__(SKY_THREADS)
k_sky_cells(const uint32_t *frames, size_t fstride, SkyDev p, int vec, int use_lds, float *cb, float *cs, int *ne) {
    extern __shared__ uint32_t sky_vals[];
    __shared__ SkySel sel;
    __shared__ int n0_s;
    const int ci = blockIdx.x, cj = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const int r0 = cj * p.cell, c0 = ci * p.cell;
    const int ch = min(p.cell, p.h - r0), cw = min(p.cell, p.w - c0), area = ch * cw;
    const uint32_t *g = frames + (size_t)f * fstride + (size_t)r0 * p.w + c0;
    const size_t o = (size_t)f * p.ny * p.nx + (size_t)cj * p.nx + ci;
    const bool in_lds = use_lds != 0;   // the host's choice for the whole mesh: a full cell fits SKY_LDS_MAX
    SkyCellSrc src;
    src.lds = nullptr; src.g = g; src.w = p.w; src.cw = cw; src.be = p.be;
    src.lo = -__builtin_inf(); src.hi = __builtin_inf();
    int n = area;
    if (in_lds) {
        if (tid == 0) n0_s = 0;
        __syncthreads();
        if (vec) {   // 16 B per lane along the rows: a 64-pixel cell row is one 256 B segment
            const int nv = cw >> 2;
            for (int q = tid; q < ch * nv; q += SKY_THREADS) {
                const int r = q / nv, c4 = q - r * nv;
                const uint4 raw = *reinterpret_cast<const uint4 *>(g + (size_t)r * p.w + 4 * c4);
                float v[4];
                bool ok[4];
                ok[0] = sky_pixel(raw.x, p.be, v[0]); ok[1] = sky_pixel(raw.y, p.be, v[1]);
                ok[2] = sky_pixel(raw.z, p.be, v[2]); ok[3] = sky_pixel(raw.w, p.be, v[3]);
                const int cnt = (int)ok[0] + (int)ok[1] + (int)ok[2] + (int)ok[3];
                if (cnt) {
                    int at = atomicAdd(&n0_s, cnt);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (ok[k]) sky_vals[at++] = __float_as_uint(v[k]);
                }
            }
        } else {
            for (int q = tid; q < area; q += SKY_THREADS) {
                const int r = q / cw, c = q - r * cw;
                float v;
                if (sky_pixel(g[(size_t)r * p.w + c], p.be, v)) sky_vals[atomicAdd(&n0_s, 1)] = __float_as_uint(v);
            }
        }
        __syncthreads();
        n = n0_s;
        src.lds = sky_vals;
    }
    float medf = 0.0f, madf = 0.0f;
    for (int t = 0; t <= p.n_clip; t++) {
        uint32_t k = 0;
        const int m = sky_select([&](int i, uint32_t &key) { float v; if (!src.value(i, v)) return false; key = sky_key(v); return true; },
                                 n, sel, &k);
        if (t == 0 && 8 * (long long)m < (long long)area) {   // empty (m == 0 included); the whole workgroup takes this branch
            if (tid == 0) { cb[o] = 0.0f; cs[o] = 0.0f; ne[o] = 0; }
            return;
        }
        medf = sky_unkey(k);
        const float med = medf;
        // |v - med| is not negative: its bits are ordered as they are
        sky_select([&](int i, uint32_t &key) { float v; if (!src.value(i, v)) return false; key = __float_as_uint(fabsf(v - med)); return true; },
                   n, sel, &k);
        madf = __uint_as_float(k);
        if (t < p.n_clip) {
            const double d = p.k_clip * 1.4826 * (double)madf;
            src.lo = fmax(src.lo, (double)medf - d);
            src.hi = fmin(src.hi, (double)medf + d);
        }
    }
    if (tid == 0) { cb[o] = medf; cs[o] = (float)(1.4826 * (double)madf); ne[o] = 1; }
}

// lower median of v[0 .. n), n <= 9, by rank counting (ties broken by index); registers only
__device__ __forceinline__ float sky_lowmed9(const float (&v)[9], int n) {
    const int r = (n - 1) >> 1;
    float out = v[0];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        int lt = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) lt += (j < n) && ((v[j] < v[i]) || (v[j] == v[i] && j < i));
        if (i < n && lt == r) out = v[i];
    }
    return out;
}

// definition steps 3 - 5 for one frame per workgroup.  fb / fs: the filled meshes (scratch); mb / ms: the filtered ones.
__global__ void __launch_bounds__(SKY_THREADS)
k_sky_mesh(SkyDev p, const float *cb_all, const float *cs_all, const int *ne_all, float *fb_all, float *fs_all, float *mb_all,
           float *ms_all, SkyRec *rec) {
    __shared__ SkySel sel;
    const int f = blockIdx.x, tid = threadIdx.x, nc = p.ny * p.nx;
    const size_t o = (size_t)f * nc;
    const float *cb = cb_all + o, *cs = cs_all + o;
    const int *ne = ne_all + o;
    float *fb = fb_all + o, *fs = fs_all + o, *mb = mb_all + o, *ms = ms_all + o;
    uint32_t kb = 0, ks = 0;
    const int n_ne = sky_select([&](int i, uint32_t &key) { if (!ne[i]) return false; key = sky_key(cb[i]); return true; }, nc, sel, &kb);
    sky_select([&](int i, uint32_t &key) { if (!ne[i]) return false; key = sky_key(cs[i]); return true; }, nc, sel, &ks);
    if (n_ne == 0) {   // LFDMI_SKY_NO_SKY
        const float nan = __builtin_nanf("");
        for (int i = tid; i < nc; i += SKY_THREADS) { mb[i] = nan; ms[i] = nan; }
        if (tid == 0) { SkyRec r; r.status = 1; r.n_empty = nc; r.sky = nan; r.sigma = nan; r.gain = 1.0f; r.pad = 0; rec[f] = r; }
        return;
    }
    const float sky = sky_unkey(kb), sigma = sky_unkey(ks);
    for (int i = tid; i < nc; i += SKY_THREADS) {
        float b = cb[i], s = cs[i];
        if (!ne[i]) {
            const int cj = i / p.nx, ci = i - cj * p.nx;
            float vb[9], vs[9];
            int n = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                const int j = cj + q / 3 - 1, k = ci + q % 3 - 1;
                vb[q] = 0.0f; vs[q] = 0.0f;
                if (q != 4 && j >= 0 && j < p.ny && k >= 0 && k < p.nx && ne[j * p.nx + k]) {
                    // (kept in neighbour order: the slots are packed below)
                    vb[q] = cb[j * p.nx + k]; vs[q] = cs[j * p.nx + k];
                    n |= 1 << q;
                }
            }
            // pack the present neighbours to the front, in order
            float wb[9], ws[9];
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) { wb[q] = 0.0f; ws[q] = 0.0f; }
#pragma unroll
            for (int q = 0; q < 9; q++) {
                if (n & (1 << q)) {
#pragma unroll
                    for (int z = 0; z < 9; z++) if (z == cnt) { wb[z] = vb[q]; ws[z] = vs[q]; }
                    cnt++;
                }
            }
            if (cnt) { b = sky_lowmed9(wb, cnt); s = sky_lowmed9(ws, cnt); }
            else { b = sky; s = sigma; }
        }
        fb[i] = b; fs[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < nc; i += SKY_THREADS) {
        if (p.filter == 1) { mb[i] = fb[i]; ms[i] = fs[i]; continue; }
        const int cj = i / p.nx, ci = i - cj * p.nx;
        float wb[9], ws[9];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 9; q++) { wb[q] = 0.0f; ws[q] = 0.0f; }
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const int j = cj + q / 3 - 1, k = ci + q % 3 - 1;
            if (j >= 0 && j < p.ny && k >= 0 && k < p.nx) {
                const float b = fb[j * p.nx + k], s = fs[j * p.nx + k];
#pragma unroll
                for (int z = 0; z < 9; z++) if (z == cnt) { wb[z] = b; ws[z] = s; }
                cnt++;
            }
        }
        mb[i] = sky_lowmed9(wb, cnt); ms[i] = sky_lowmed9(ws, cnt);
    }
    if (tid == 0) {
        SkyRec r;
        r.status = 0; r.n_empty = nc - n_ne; r.sky = sky; r.sigma = sigma; r.gain = 1.0f; r.pad = 0;
        if (p.mode == 1) {   // LFDMI_SKY_NORMALISE
            if (sigma == 0.0f) r.status = 2;   // LFDMI_SKY_NO_NOISE
            else r.gain = (float)(p.target_sigma / (double)sigma);
        }
        rec[f] = r;
    }
}

// out = (x - bkg) * gain.  A workgroup takes SKY_THREADS * V columns of the rows between two cell centres (mesh row interval j:
// rows [rstart[j], rstart[j + 1])): there top / bot of definition step 6 depend on the column only and stay in registers, a row
// adds its ty.  col_i / col_tx, rstart / row_ty: the host's tables of step 6.  grid (column spans, ny * SKY_ROW_SPLIT, frames).
// in == out is allowed: every pixel is read and written by the same thread.
template <int V>
__global__ void __launch_bounds__(SKY_THREADS)
k_sky_apply(const uint32_t *in, size_t in_stride, float *out, size_t out_stride, SkyDev p, const float *mb_all, const SkyRec *rec,
            const int *col_i, const float *col_tx, const int *rstart, const float *row_ty) {
    const int f = blockIdx.z, j = blockIdx.y / SKY_ROW_SPLIT, part = blockIdx.y % SKY_ROW_SPLIT;
    const int x0 = (blockIdx.x * SKY_THREADS + threadIdx.x) * V;
    if (x0 >= p.w) return;
    const SkyRec r = rec[f];
    const float gain = r.gain;
    const float *m = mb_all + (size_t)f * p.ny * p.nx;
    const int j2 = min(j + 1, p.ny - 1);
    float top[V], bot[V];
#pragma unroll
    for (int c = 0; c < V; c++) {
        if (r.status == 1) { top[c] = 0.0f; bot[c] = 0.0f; continue; }   // NO_SKY: the input, non-finite pixels zeroed
        const int i = col_i[x0 + c], i2 = min(i + 1, p.nx - 1);
        const float tx = col_tx[x0 + c];
        const float a = m[j * p.nx + i], b = m[j * p.nx + i2], c2 = m[j2 * p.nx + i], d = m[j2 * p.nx + i2];
        top[c] = a + tx * (b - a);
        bot[c] = c2 + tx * (d - c2);
    }
    const uint32_t *src = in + (size_t)f * in_stride;
    float *dst = out + (size_t)f * out_stride;
    const int y1 = rstart[j + 1];
    for (int y = rstart[j] + part; y < y1; y += SKY_ROW_SPLIT) {
        const float ty = row_ty[y];
        const size_t at = (size_t)y * p.w + x0;
        uint32_t raw[V];
        if (V == 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(src + at);
            raw[0] = q.x; raw[V > 1 ? 1 : 0] = q.y; raw[V > 2 ? 2 : 0] = q.z; raw[V > 3 ? 3 : 0] = q.w;
        } else raw[0] = src[at];
        float o[V];
#pragma unroll
        for (int c = 0; c < V; c++) {
            uint32_t bits = p.be ? sky_bswap(raw[c]) : raw[c];
            const float bkg = top[c] + ty * (bot[c] - top[c]);
            const float x = __uint_as_float(bits);
            o[c] = ((bits & 0x7F800000u) == 0x7F800000u) ? 0.0f : (x - bkg) * gain;
        }
        if (V == 4) *reinterpret_cast<float4 *>(dst + at) = make_float4(o[0], o[V > 1 ? 1 : 0], o[V > 2 ? 2 : 0], o[V > 3 ? 3 : 0]);
        else dst[at] = o[0];
    }
}
