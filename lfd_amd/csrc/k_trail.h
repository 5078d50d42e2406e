// k_trail.h -- trail profiles (lfdmi_measure_trails): refine the detected line of a frame and measure its cross-section.
// The procedure and its constants are defined in include/lfdmi.h ("trail profiles"); tests/trail_ref.py restates it.  Every
// value below is reproduced exactly by that restatement: samples are float32 with a fixed operation order (the library is
// built with -ffp-contract=off), medians are exact selections (no summation order), and the per-frame fit runs its sums in
// double, sequentially, in one lane.
//
// One call works on a compacted list of frames (found != 0), in chunks of at most G (the context's max_inflight) slots:
//   k_trail_mask   remove_stars' squares (k_rs_boxes' output) -> a bit plane per slot, buffer rows, 32 columns per word
//   k_trail_init   the start line's positions (per slot, one thread)
//   k_trail_seg    one workgroup per (slot, segment): a wave's lanes are the segment's positions, its 64 samples at one
//                  offset are sorted across the lanes (bitonic, __shfl_xor) and the lower median is read from one lane
//   k_trail_fit    one wave per slot: lanes take segments (background, noise, amplitude, centre), lane 0 finds the run and
//                  fits the line, moves it, and sets up the next pass's positions; finished frames drop out here
//   k_trail_prof   one workgroup per (slot, profile bin): keys of the valid samples in LDS, then an exact radix select
//   k_trail_final  one wave per slot: background and noise (lanes rank the wing bins), peak, fwhm, depth, end points
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define TRAIL_MAX_R 64                  // half_width <= 64: 2R+1 <= 129 offsets
#define TRAIL_MAX_K 512                 // profile bins 2K+1 <= 1025
#define TRAIL_SEG_THREADS 256

// per-slot state of a call (device), one per frame of the compacted list
struct TrailState {
    double fx, fy, dx, dy;   // foot point and unit direction (flipped frame)
    const void *img;         // the frame (caller's device memory, or the staging slot of a host frame)
    int frame;               // index of the frame in the call (row of the output)
    int slot;                // slot within its chunk (mask plane, segment tables)
    int chunk_frame;         // index of the frame within its chunk (catalogue squares)
    int status;              // 0 running / done ok, > 0 LFDMI_TRAIL_*, < 0 an lfdmi_status
    int tmin, npos, nseg;    // positions of the current line
    int s0, s1;              // the extent: segments s0 .. s1 of the last pass
    int min_valid;           // fewest valid samples in a profile bin
    int done;                // finished (ok or not): later kernels leave the slot alone
};

struct TrailDev {            // lfdmi_trail_params as the kernels use them
    int R, L, n_iter, wing, K, maxseg, maxpos, be, h, w, wq;
    double k_sig, P, step, pixscale;
};

// the sample of definition step 2 (NaN: not valid)
__device__ __forceinline__ float trail_load(const void *img, size_t idx, int be) {
    uint32_t u = ((const uint32_t *)img)[idx];
    if (be) u = __builtin_bswap32(u);
    return __uint_as_float(u);
}

__device__ __forceinline__ bool trail_star(const uint32_t *plane, int wq, int r, int c) {
    return plane && ((plane[(size_t)r * wq + (c >> 5)] >> (c & 31)) & 1u);
}

__device__ float trail_sample(const TrailDev &p, const void *img, const uint32_t *plane, double x, double y) {
    const double xf = floor(x), yf = floor(y);
    if (!(xf >= 0.0 && xf <= (double)(p.w - 2) && yf >= 0.0 && yf <= (double)(p.h - 2))) return __builtin_nanf("");
    const int x0 = (int)xf, y0 = (int)yf;
    const int r0 = p.h - 1 - y0, r1 = r0 - 1;   // buffer rows of y0 and y0 + 1
    if (trail_star(plane, p.wq, r0, x0) || trail_star(plane, p.wq, r0, x0 + 1) || trail_star(plane, p.wq, r1, x0) ||
        trail_star(plane, p.wq, r1, x0 + 1))
        return __builtin_nanf("");
    const size_t w = (size_t)p.w;
    const float v00 = trail_load(img, (size_t)r0 * w + x0, p.be), v10 = trail_load(img, (size_t)r0 * w + x0 + 1, p.be);
    const float v01 = trail_load(img, (size_t)r1 * w + x0, p.be), v11 = trail_load(img, (size_t)r1 * w + x0 + 1, p.be);
    if (!(isfinite(v00) && isfinite(v10) && isfinite(v01) && isfinite(v11))) return __builtin_nanf("");
    const float a = (float)(x - xf), b = (float)(y - yf);
    const float top = v00 + a * (v10 - v00);
    const float bot = v01 + a * (v11 - v01);
    return top + b * (bot - top);
}

// positions of a line (definition step 2): tmin, npos (0: none)
__device__ __forceinline__ void trail_range(const TrailDev &p, TrailState &s) {
    double lo = -INFINITY, hi = INFINITY;
    bool empty = false;
    const double f[2] = {s.fx, s.fy}, d[2] = {s.dx, s.dy}, mx[2] = {(double)(p.w - 1), (double)(p.h - 1)};
    for (int a = 0; a < 2; a++) {
        if (d[a] != 0.0) {
            const double t1 = (0.0 - f[a]) / d[a], t2 = (mx[a] - f[a]) / d[a];
            lo = fmax(lo, fmin(t1, t2));
            hi = fmin(hi, fmax(t1, t2));
        } else if (f[a] < 0.0 || f[a] > mx[a]) {
            empty = true;
        }
    }
    s.tmin = 0; s.npos = 0; s.nseg = 0;
    if (empty || !(lo <= hi)) return;
    const double a = ceil(lo), b = floor(hi);
    if (!(a <= b)) return;
    s.tmin = (int)a;
    s.npos = (int)(b - a) + 1;
    const int rem = s.npos % p.L;
    s.nseg = s.npos / p.L + (2 * rem >= p.L ? 1 : 0);
}

// after trail_range: TOO_SHORT / capacity, or ready for a pass
__device__ __forceinline__ void trail_check(const TrailDev &p, TrailState &s) {
    if (s.npos < 2 * p.L) { s.status = 2; s.done = 1; return; }   // LFDMI_TRAIL_TOO_SHORT
    if (s.npos > p.maxpos || s.nseg > p.maxseg) { s.status = -5; s.done = 1; }  // LFDMI_ERR_CAPACITY (never for frames of the ctx)
}

// remove_stars' squares (rows [x, y) x columns [z, w) of the buffer) of the chunk's frames -> per-slot bit planes
__global__ void __launch_bounds__(256)
k_trail_mask(const TrailState *st, int nact, int max_obj, const int4 *boxes, uint32_t *planes, TrailDev p) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= nact || i >= max_obj) return;
    const TrailState &s = st[k];
    const int4 bx = boxes[(size_t)s.chunk_frame * max_obj + i];
    if (bx.y <= bx.x || bx.w <= bx.z) return;
    uint32_t *plane = planes + (size_t)s.slot * p.h * p.wq;
    const int wa = bx.z >> 5, wb = (bx.w - 1) >> 5, nw = wb - wa + 1;
    for (int q = lane; q < (bx.y - bx.x) * nw; q += 64) {
        const int r = bx.x + q / nw, wq_ = wa + q % nw;
        uint32_t m = 0xFFFFFFFFu;
        if (wq_ == wa) m &= 0xFFFFFFFFu << (bx.z & 31);
        if (wq_ == wb) m &= 0xFFFFFFFFu >> (31 - ((bx.w - 1) & 31));
        atomicOr(&plane[(size_t)r * p.wq + wq_], m);
    }
}

__global__ void k_trail_init(TrailState *st, int nact, TrailDev p) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nact) return;
    TrailState s = st[k];
    trail_range(p, s);
    trail_check(p, s);
    st[k] = s;
}

// m_s(u) for every segment s and offset u in [-R, R]: segm[(slot * maxseg + s) * (2R+1) + (u + R)]
__global__ void __launch_bounds__(TRAIL_SEG_THREADS)
k_trail_seg(const TrailState *st, int nact, const uint32_t *planes, float *segm, TrailDev p) {
    const int k = blockIdx.y, sg = blockIdx.x;
    if (k >= nact) return;
    const TrailState s = st[k];
    if (s.done || sg >= s.nseg) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = TRAIL_SEG_THREADS / 64;
    const uint32_t *plane = planes ? planes + (size_t)s.slot * p.h * p.wq : nullptr;
    const int j = sg * p.L + lane;
    const bool in = lane < p.L && j < s.npos;
    const double t = (double)(s.tmin + j);
    const double nx = s.dy, ny = -s.dx;
    const int nu = 2 * p.R + 1;
    float *out = segm + ((size_t)s.slot * p.maxseg + sg) * nu;
    for (int ui = wv; ui < nu; ui += nwv) {
        const double u = (double)(ui - p.R);
        float v = __builtin_nanf("");
        if (in) {
            const double x = s.fx + t * s.dx + u * nx;
            const double y = s.fy + t * s.dy + u * ny;
            v = trail_sample(p, s.img, plane, x, y);
        }
        const bool ok = !isnan(v);
        const int m = __popcll(__ballot(ok));
        float key = ok ? v : INFINITY;
        // bitonic sort of the 64 lanes' values, ascending by lane
        for (int size = 2; size <= 64; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const float o = __shfl_xor(key, stride);
                const bool up = (lane & size) == 0;
                const bool lower = (lane & stride) == 0;
                key = (lower == up) ? fminf(key, o) : fmaxf(key, o);
            }
        const float med = __shfl(key, m > 0 ? (m - 1) >> 1 : 0);
        if (lane == 0) out[ui] = m > 0 ? med : __builtin_nanf("");
    }
}

// lower median (rank (n-1)/2, ties broken by index) of n values produced by f(i); exact selection without a buffer
template <typename F>
__device__ double trail_lowmed(int n, F f) {
    const int r = (n - 1) >> 1;
    for (int i = 0; i < n; i++) {
        const double vi = f(i);
        int lt = 0;
        for (int j = 0; j < n; j++) {
            const double vj = f(j);
            lt += (vj < vi) || (vj == vi && j < i);
        }
        if (lt == r) return vi;
    }
    return __builtin_nan("");
}

// wing offsets of [-R, R] in index order: i = 0 .. 2*wing-1 -> u index
__device__ __forceinline__ int trail_wing_idx(const TrailDev &p, int i) { return i < p.wing ? i : 2 * p.R + 1 - 2 * p.wing + i; }

// one wave per slot: segment statistics (lanes), then the run, the fit and the next pass's positions (lane 0)
__global__ void __launch_bounds__(64)
k_trail_fit(TrailState *st, int nact, const float *segm, double *sA, double *sC, int *sSig, int last, TrailDev p) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= nact) return;
    TrailState s = st[k];
    if (s.done) return;
    const int nu = 2 * p.R + 1;
    for (int sg = lane; sg < s.nseg; sg += 64) {
        const float *m = segm + ((size_t)s.slot * p.maxseg + sg) * nu;
        bool nan = false;
        for (int ui = 0; ui < nu; ui++) nan |= isnan(m[ui]);
        double A = 0.0, c = 0.0;
        int sig = 0;
        if (!nan) {
            const double b = trail_lowmed(2 * p.wing, [&](int i) { return (double)m[trail_wing_idx(p, i)]; });
            const double sd = 1.4826 * trail_lowmed(2 * p.wing, [&](int i) { return fabs((double)m[trail_wing_idx(p, i)] - b); });
            A = -INFINITY;
            for (int ui = 0; ui < nu; ui++) A = fmax(A, (double)m[ui] - b);
            if (A > p.k_sig * sd && A > 0.0) {
                sig = 1;
                double sw = 0.0, su = 0.0;
                for (int ui = 0; ui < nu; ui++) {
                    const double wu = fmax(((double)m[ui] - b) - A * 0.5, 0.0);
                    sw = sw + wu;
                    su = su + (double)(ui - p.R) * wu;
                }
                c = su / sw;
            }
        }
        const size_t o = (size_t)s.slot * p.maxseg + sg;
        sA[o] = A; sC[o] = c; sSig[o] = sig;
    }
    __syncthreads();
    if (lane != 0) return;
    const size_t o0 = (size_t)s.slot * p.maxseg;
    int best0 = 0, bestn = 0, cur0 = 0, curn = 0;
    for (int sg = 0; sg < s.nseg; sg++) {
        if (sSig[o0 + sg]) {
            if (curn == 0) cur0 = sg;
            curn++;
            if (curn > bestn) { bestn = curn; best0 = cur0; }
        } else {
            curn = 0;
        }
    }
    if (bestn < 2) { s.status = 3; s.done = 1; st[k] = s; return; }   // LFDMI_TRAIL_TOO_FAINT
    s.s0 = best0; s.s1 = best0 + bestn - 1;
    if (last) { st[k] = s; return; }
    double S = 0.0, St = 0.0, Stt = 0.0, Sc = 0.0, Stc = 0.0;
    for (int sg = s.s0; sg <= s.s1; sg++) {
        const int ns = min(p.L, s.npos - sg * p.L);
        const double tm = (double)(s.tmin + sg * p.L) + (double)(ns - 1) * 0.5;
        const double wgt = sA[o0 + sg], c = sC[o0 + sg];
        S = S + wgt;
        St = St + wgt * tm;
        Stt = Stt + wgt * tm * tm;
        Sc = Sc + wgt * c;
        Stc = Stc + wgt * tm * c;
    }
    const double bb = (S * Stc - St * Sc) / (S * Stt - St * St);
    const double aa = (Sc - bb * St) / S;
    const double nx = s.dy, ny = -s.dx;
    s.fx = s.fx + aa * nx;
    s.fy = s.fy + aa * ny;
    const double ex = s.dx + bb * nx, ey = s.dy + bb * ny;
    const double len = sqrt(ex * ex + ey * ey);
    s.dx = ex / len;
    s.dy = ey / len;
    trail_range(p, s);
    trail_check(p, s);
    st[k] = s;
}

// raw profile m(u_k) over the extent: prof[frame * (2K+1) + k], valid counts cnt[slot * (2K+1) + k]
__device__ __forceinline__ uint32_t trail_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float trail_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ void __launch_bounds__(256)
k_trail_prof(const TrailState *st, int nact, const uint32_t *planes, float *prof, int *cnt, TrailDev p) {
    extern __shared__ uint32_t keys[];    // p.maxpos entries
    __shared__ int hist[256];
    __shared__ int nvalid, sel_digit, sel_rank;
    const int k = blockIdx.y, bin = blockIdx.x, nb = 2 * p.K + 1;
    if (k >= nact) return;
    const TrailState s = st[k];
    if (s.done) return;
    const uint32_t *plane = planes ? planes + (size_t)s.slot * p.h * p.wq : nullptr;
    const int j0 = s.s0 * p.L, j1 = min(s.s1 * p.L + p.L, s.npos);
    const double u = (double)(bin - p.K) * p.step;
    const double nx = s.dy, ny = -s.dx;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    for (int j = j0 + (int)threadIdx.x; j < j1; j += 256) {
        const double t = (double)(s.tmin + j);
        const double x = s.fx + t * s.dx + u * nx;
        const double y = s.fy + t * s.dy + u * ny;
        const float v = trail_sample(p, s.img, plane, x, y);
        if (!isnan(v)) keys[atomicAdd(&nvalid, 1)] = trail_key(v);
    }
    __syncthreads();
    const int m = nvalid;
    if (m == 0) {
        if (threadIdx.x == 0) { prof[(size_t)s.frame * nb + bin] = __builtin_nanf(""); cnt[(size_t)s.slot * nb + bin] = 0; }
        return;
    }
    // radix select of rank (m-1)/2, 8 bits per pass from the top
    uint32_t prefix = 0, mask = 0;
    int r = (m - 1) >> 1;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 256) {
            const uint32_t key = keys[i];
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (threadIdx.x < 64) {   // one wave: 4 bins per lane, inclusive scan across lanes
            const int l = threadIdx.x;
            const int c0 = hist[4 * l], c1 = hist[4 * l + 1], c2 = hist[4 * l + 2], c3 = hist[4 * l + 3];
            const int tot = c0 + c1 + c2 + c3;
            int inc = tot;
            for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(inc, off); if (l >= off) inc += t; }
            const int exc = inc - tot;
            if (r >= exc && r < inc) {   // exactly one lane holds the rank
                int rr = r - exc, d = 4 * l;
                if (rr >= c0) { rr -= c0; d++; if (rr >= c1) { rr -= c1; d++; if (rr >= c2) { rr -= c2; d++; } } }
                sel_digit = d;
                sel_rank = rr;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sel_digit << shift;
        mask |= 255u << shift;
        r = sel_rank;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        prof[(size_t)s.frame * nb + bin] = trail_unkey(prefix);
        cnt[(size_t)s.slot * nb + bin] = m;
    }
}

// lower median of mv[0 .. n) (LDS) by the 64 lanes of the workgroup: each ranks its candidates (ties broken by index), the
// one holding rank (n-1)/2 writes it to *med
__device__ void trail_lowmed_wave(const double *mv, int n, double *med) {
    const int r = (n - 1) >> 1;
    for (int i = threadIdx.x; i < n; i += 64) {
        const double vi = mv[i];
        int lt = 0;
        for (int j = 0; j < n; j++) lt += (mv[j] < vi) || (mv[j] == vi && j < i);
        if (lt == r) *med = vi;
    }
}

// the record's doubles (rec: 10 per frame: x1, y1, x2, y2, background, noise, peak, fwhm, fwhm_arcsec, depth; rho / theta
// are the host's) and the background-subtracted profile, in place.  One wave per slot: the two medians over the wing bins
// are ranked by all lanes, the rest runs in lane 0.
__global__ void __launch_bounds__(64)
k_trail_final(TrailState *st, int nact, float *prof, const int *cnt, double *rec, TrailDev p) {
    __shared__ float wv[2 * TRAIL_MAX_K + 1];
    __shared__ double mv[2 * TRAIL_MAX_K + 1];
    __shared__ double med;
    __shared__ int nw_s;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= nact) return;
    TrailState s = st[k];
    if (s.done) return;
    const int nb = 2 * p.K + 1;
    float *v = prof + (size_t)s.frame * nb;
    const int *c = cnt + (size_t)s.slot * nb;
    // the non-NaN wing bins (|u_k| >= P - wing), in index order
    const double lim = p.P - (double)p.wing;
    if (lane == 0) {
        int nw = 0;
        for (int b = 0; b < nb; b++)
            if (fabs((double)(b - p.K) * p.step) >= lim && !isnan(v[b])) wv[nw++] = v[b];
        nw_s = nw;
    }
    __syncthreads();
    const int nw = nw_s;
    for (int i = lane; i < nw; i += 64) mv[i] = (double)wv[i];
    __syncthreads();
    trail_lowmed_wave(mv, nw, &med);
    __syncthreads();
    const float bg = nw > 0 ? (float)med : __builtin_nanf("");
    for (int i = lane; i < nw; i += 64) { wv[i] = wv[i] - bg; mv[i] = fabs((double)wv[i]); }
    __syncthreads();
    trail_lowmed_wave(mv, nw, &med);
    __syncthreads();
    if (lane != 0) return;
    const double noise = nw > 0 ? 1.4826 * med : __builtin_nan("");
    int minv = 0x7FFFFFFF;
    for (int b = 0; b < nb; b++) minv = min(minv, c[b]);
    for (int b = 0; b < nb; b++) v[b] = v[b] - bg;
    float peak = -INFINITY;
    for (int b = 0; b < nb; b++) if (!isnan(v[b])) peak = fmaxf(peak, v[b]);
    s.done = 1;
    if (!(peak > 0.0f)) { s.status = 3; st[k] = s; return; }   // LFDMI_TRAIL_TOO_FAINT
    const float half = peak / 2.0f;
    int left = -1, right = -1;
    for (int b = 0; b < nb; b++) if (v[b] >= half) { if (left < 0) left = b; right = b; }
    const double fwhm = left == right ? 0.0 : fabs((double)(right - p.K) * p.step) + fabs((double)(left - p.K) * p.step);
    const double depth = ((double)peak - (double)v[p.K]) / (double)peak * 100.0;
    const int j0 = s.s0 * p.L, j1 = min(s.s1 * p.L + p.L, s.npos) - 1;
    const double ta = (double)(s.tmin + j0), tb = (double)(s.tmin + j1);
    double *r = rec + (size_t)s.frame * 10;
    r[0] = s.fx + ta * s.dx; r[1] = s.fy + ta * s.dy;
    r[2] = s.fx + tb * s.dx; r[3] = s.fy + tb * s.dy;
    r[4] = (double)bg; r[5] = noise; r[6] = (double)peak;
    r[7] = fwhm; r[8] = fwhm * p.pixscale; r[9] = depth;
    s.min_valid = minv;
    st[k] = s;
}
