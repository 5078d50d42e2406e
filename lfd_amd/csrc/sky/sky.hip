// sky.hip -- host side of the sky normalisation (include/lfdmi.h: sky normalisation; kernels in k_sky.h).  Its own translation
// unit in its own directory: the detection kernels' code object does not change with it.  The context's internals are reached
// through unit.h; the handle owns every byte of device and page-locked memory the pass uses.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../unit.h"
#include "k_sky.h"

#define SKY_PIN_SLOTS 4   // page-locked staging slots (one frame each) for LFDMI_HOST frames

struct lfdmi_sky {
    lfdmi_ctx *ctx = nullptr;   // lfdmi_sky_normalize only: destroy does not touch the context (it may be gone by then)
    int device = 0, max_frames = 0;
    SkyDev p;
    size_t N = 0, nc = 0, lds = 0;
    float *buf = nullptr;                 // max_frames frames: the handle's output buffer (and the upload target of host frames)
    float *cb = nullptr, *cs = nullptr, *fb = nullptr, *fs = nullptr, *mb = nullptr, *ms = nullptr;   // max_frames x ny x nx
    int *ne = nullptr;
    SkyRec *rec = nullptr;
    int *col_i = nullptr, *rstart = nullptr;
    float *col_tx = nullptr, *row_ty = nullptr;
    void *pin[SKY_PIN_SLOTS] = {};
    hipEvent_t pin_ev[SKY_PIN_SLOTS] = {};
    int64_t bytes = 0;
};

extern "C" void lfdmi_default_sky_params(lfdmi_sky_params *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->cell = 64; o->n_clip = 3; o->filter = 3; o->mode = LFDMI_SKY_NORMALISE;
    o->k_clip = 3.0; o->target_sigma = 0.025;
}

// definition step 6 along one axis: for every pixel position the cell index and the float32 weight; start[j] = first position of
// interval j (start[nc] = len)
static void axis_tables(int len, int cell, int nc, std::vector<int> &idx, std::vector<float> &t, std::vector<int> *start) {
    std::vector<double> centre(nc);
    for (int j = 0; j < nc; j++) {
        const int r0 = j * cell, r1 = std::min((j + 1) * cell, len);
        centre[j] = (double)(r0 + r1 - 1) * 0.5;
    }
    idx.assign(len, 0);
    t.assign(len, 0.0f);
    int j = 0;
    for (int y = 0; y < len; y++) {
        while (j + 1 < nc && centre[j + 1] <= (double)y) j++;
        const int j2 = std::min(j + 1, nc - 1);
        idx[y] = j;
        if (j2 != j && (double)y >= centre[j]) t[y] = (float)(((double)y - centre[j]) / (centre[j2] - centre[j]));
    }
    if (start) {
        start->assign(nc + 1, len);
        for (int y = len - 1; y >= 0; y--) (*start)[idx[y]] = y;
        for (int k = nc - 1; k >= 0; k--) (*start)[k] = std::min((*start)[k], (*start)[k + 1]);   // (an interval without rows is empty)
    }
}

extern "C" int lfdmi_sky_create(lfdmi_ctx *ctx, int h, int w, int max_frames, const lfdmi_sky_params *pp, lfdmi_sky **out) {
    if (!ctx) return LFDMI_ERR_ARG;
    if (!out) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    lfdmi_sky_params q;
    if (pp) q = *pp; else lfdmi_default_sky_params(&q);
    // (the launches put frames in grid.z, mesh rows times SKY_ROW_SPLIT in grid.y: both at most 65535)
    if (h < 1 || w < 1 || max_frames < 1 || max_frames > 65535 || (double)h * w > 1e9 || (h + std::max(q.cell, 16) - 1) / std::max(q.cell, 16) * SKY_ROW_SPLIT > 65535)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_sky_create: h, w must be positive (at most 16383 mesh rows, h * w at most 1e9), max_frames 1 .. 65535");
    if (q.cell < 16 || q.cell > 256 || q.n_clip < 0 || q.n_clip > 8 || (q.filter != 1 && q.filter != 3) ||
        (q.mode != LFDMI_SKY_SUBTRACT && q.mode != LFDMI_SKY_NORMALISE) || !std::isfinite(q.k_clip) || !(q.k_clip > 0) ||
        !std::isfinite(q.target_sigma) || !(q.target_sigma > 0))
        return ctx_fail(ctx, LFDMI_ERR_ARG, "sky params out of range (include/lfdmi.h: lfdmi_sky_params)");
    auto *s = new lfdmi_sky();
    s->ctx = ctx; s->device = ctx_device(ctx); s->max_frames = max_frames;
    SkyDev &p = s->p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.w = w; p.cell = q.cell; p.ny = (h + q.cell - 1) / q.cell; p.nx = (w + q.cell - 1) / q.cell;
    p.n_clip = q.n_clip; p.filter = q.filter; p.mode = q.mode; p.k_clip = q.k_clip; p.target_sigma = q.target_sigma;
    s->N = (size_t)h * w; s->nc = (size_t)p.ny * p.nx;
    const size_t cell_px = (size_t)std::min(q.cell, h) * std::min(q.cell, w);
    s->lds = cell_px <= SKY_LDS_MAX ? cell_px * sizeof(uint32_t) : 0;
    std::vector<int> ci, ri, rs;
    std::vector<float> col_t, rty;
    axis_tables(w, q.cell, p.nx, ci, col_t, nullptr);
    axis_tables(h, q.cell, p.ny, ri, rty, &rs);
    auto run = [&]() -> int {
        const size_t M = (size_t)max_frames * s->nc;
        UHIP(hipMalloc(&s->buf, (size_t)max_frames * s->N * sizeof(float)));
        for (float **m : {&s->cb, &s->cs, &s->fb, &s->fs, &s->mb, &s->ms}) UHIP(hipMalloc(m, M * sizeof(float)));
        UHIP(hipMalloc(&s->ne, M * sizeof(int)));
        UHIP(hipMalloc(&s->rec, (size_t)max_frames * sizeof(SkyRec)));
        UHIP(hipMalloc(&s->col_i, (size_t)w * sizeof(int)));
        UHIP(hipMalloc(&s->col_tx, (size_t)w * sizeof(float)));
        UHIP(hipMalloc(&s->rstart, (size_t)(p.ny + 1) * sizeof(int)));
        UHIP(hipMalloc(&s->row_ty, (size_t)h * sizeof(float)));
        s->bytes = (int64_t)((size_t)max_frames * s->N * 4 + M * 28 + (size_t)max_frames * sizeof(SkyRec) + (size_t)w * 8 +
                             (size_t)(p.ny + 1) * 4 + (size_t)h * 4);
        UHIP(hipMemcpy(s->col_i, ci.data(), (size_t)w * sizeof(int), hipMemcpyHostToDevice));
        UHIP(hipMemcpy(s->col_tx, col_t.data(), (size_t)w * sizeof(float), hipMemcpyHostToDevice));
        UHIP(hipMemcpy(s->rstart, rs.data(), (size_t)(p.ny + 1) * sizeof(int), hipMemcpyHostToDevice));
        UHIP(hipMemcpy(s->row_ty, rty.data(), (size_t)h * sizeof(float), hipMemcpyHostToDevice));
        if (s->lds > 48 * 1024)   // a 128 x 128 cell: 64 KB of the CU's 160 KB
            UHIP(hipFuncSetAttribute((const void *)k_sky_cells, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds));
        return 0;
    };
    rc = run();
    if (rc) { lfdmi_sky_destroy(s); return rc; }
    *out = s;
    return 0;
}

extern "C" void lfdmi_sky_destroy(lfdmi_sky *s) {
    if (!s) return;
    // lfdmi_sky_normalize returns after its stream has drained, so no work of the context still uses these buffers
    DeviceGuard on(s->device);   // the caller's current device stays what it was
    for (void *x : {(void *)s->buf, (void *)s->cb, (void *)s->cs, (void *)s->fb, (void *)s->fs, (void *)s->mb, (void *)s->ms, (void *)s->ne,
                    (void *)s->rec, (void *)s->col_i, (void *)s->col_tx, (void *)s->rstart, (void *)s->row_ty})
        if (x) hipFree(x);
    for (int k = 0; k < SKY_PIN_SLOTS; k++) {
        if (s->pin[k]) hipHostFree(s->pin[k]);
        if (s->pin_ev[k]) hipEventDestroy(s->pin_ev[k]);
    }
    delete s;
}

extern "C" int lfdmi_sky_dims(const lfdmi_sky *s, int32_t *ny, int32_t *nx, int64_t *bytes) {
    if (!s) return LFDMI_ERR_ARG;
    if (ny) *ny = s->p.ny;
    if (nx) *nx = s->p.nx;
    if (bytes) *bytes = s->bytes;
    return 0;
}

extern "C" void *lfdmi_sky_frames(lfdmi_sky *s) { return s ? (void *)s->buf : nullptr; }

extern "C" int lfdmi_sky_normalize(lfdmi_ctx *ctx, lfdmi_sky *s, const void *frames, int dtype, int n, int loc, void *out, int out_loc,
                                   lfdmi_sky_frame *rec, float *mesh_sky, float *mesh_sigma) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!s || s->ctx != ctx) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_sky_normalize: the handle belongs to another context");
    if (n < 0 || (n > 0 && (!frames || !rec))) return ctx_fail(ctx, LFDMI_ERR_ARG, "NULL argument");
    if ((rc = unit_dtype(ctx, "lfdmi_sky_normalize", dtype)) || (rc = unit_loc(ctx, loc))) return rc;
    if (out && out_loc != LFDMI_HOST && out_loc != LFDMI_DEVICE && out_loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad out_loc");
    const size_t N = s->N, nc = s->nc, FB = N * sizeof(float);
    const bool in_dev = loc == LFDMI_DEVICE, out_dev = out && out_loc == LFDMI_DEVICE, out_host = out && !out_dev;
    if (!out && n > s->max_frames)
        return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_sky_normalize: the handle's buffer holds max_frames frames; give an output buffer for more");
    if (in_dev && out_dev) {
        const char *a = (const char *)frames, *b = (const char *)out;
        if (a == b) {
            if (dtype != LFDMI_F32) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_sky_normalize: in place takes LFDMI_F32 device frames");
        } else if (a < b + (size_t)n * FB && b < a + (size_t)n * FB)
            return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_sky_normalize: the output overlaps the frames (in place: out == frames)");
    }
    if (n == 0) return 0;
    hipStream_t st = ctx_stream(ctx);
    if (loc == LFDMI_HOST)
        for (int k = 0; k < SKY_PIN_SLOTS && k < n; k++)
            if (!s->pin[k]) {
                UHIP(hipHostMalloc(&s->pin[k], FB, hipHostMallocDefault));
                UHIP(hipEventCreateWithFlags(&s->pin_ev[k], hipEventDisableTiming));
            }
    SkyDev p = s->p;
    p.be = dtype == LFDMI_F32_BE;
    std::vector<SkyRec> hrec(n);
    const int CH = s->max_frames;
    int staged = 0;   // host frames uploaded so far (a pinned slot is reused once its copy has been read)
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int nf = std::min(CH, n - c0);
        const uint32_t *src;
        if (in_dev) src = (const uint32_t *)frames + (size_t)c0 * N;
        else {
            for (int k = 0; k < nf; k++, staged++) {
                const char *from = (const char *)frames + (size_t)(c0 + k) * FB;
                if (loc == LFDMI_HOST) {
                    const int slot = staged % SKY_PIN_SLOTS;
                    if (staged >= SKY_PIN_SLOTS) UHIP(hipEventSynchronize(s->pin_ev[slot]));
                    memcpy(s->pin[slot], from, FB);
                    from = (const char *)s->pin[slot];
                    UHIP(hipMemcpyAsync(s->buf + (size_t)k * N, from, FB, hipMemcpyHostToDevice, st));
                    UHIP(hipEventRecord(s->pin_ev[slot], st));
                } else UHIP(hipMemcpyAsync(s->buf + (size_t)k * N, from, FB, hipMemcpyHostToDevice, st));
            }
            src = (const uint32_t *)s->buf;
        }
        // where the chunk's pixels are written: the caller's device buffer, or the handle's (copied to a host buffer afterwards)
        float *dst = out_dev ? (float *)out + (size_t)c0 * N : s->buf;
        const int vec_in = p.w % 4 == 0 && p.cell % 4 == 0 && ((uintptr_t)src % 16) == 0;
        k_sky_cells<<<dim3(p.nx, p.ny, nf), SKY_THREADS, s->lds, st>>>(src, N, p, vec_in, s->lds != 0, s->cb, s->cs, s->ne);
        ULAUNCH("k_sky_cells");
        k_sky_mesh<<<nf, SKY_THREADS, 0, st>>>(p, s->cb, s->cs, s->ne, s->fb, s->fs, s->mb, s->ms, s->rec);
        ULAUNCH("k_sky_mesh");
        const bool v4 = p.w % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
        const int span = SKY_THREADS * (v4 ? 4 : 1);
        const dim3 grid((p.w + span - 1) / span, p.ny * SKY_ROW_SPLIT, nf);
        if (v4) k_sky_apply<4><<<grid, SKY_THREADS, 0, st>>>(src, N, dst, N, p, s->mb, s->rec, s->col_i, s->col_tx, s->rstart, s->row_ty);
        else k_sky_apply<1><<<grid, SKY_THREADS, 0, st>>>(src, N, dst, N, p, s->mb, s->rec, s->col_i, s->col_tx, s->rstart, s->row_ty);
        ULAUNCH("k_sky_apply");
        if (out_host) UHIP(hipMemcpyAsync((char *)out + (size_t)c0 * FB, s->buf, (size_t)nf * FB, hipMemcpyDeviceToHost, st));
        UHIP(hipMemcpyAsync(hrec.data() + c0, s->rec, (size_t)nf * sizeof(SkyRec), hipMemcpyDeviceToHost, st));
        if (mesh_sky) UHIP(hipMemcpyAsync(mesh_sky + (size_t)c0 * nc, s->mb, (size_t)nf * nc * sizeof(float), hipMemcpyDeviceToHost, st));
        if (mesh_sigma) UHIP(hipMemcpyAsync(mesh_sigma + (size_t)c0 * nc, s->ms, (size_t)nf * nc * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    UHIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        lfdmi_sky_frame &o = rec[i];
        o.status = hrec[i].status; o.ny = p.ny; o.nx = p.nx; o.n_empty = hrec[i].n_empty;
        o.sky = (double)hrec[i].sky; o.sigma = (double)hrec[i].sigma; o.gain = (double)hrec[i].gain;
    }
    return 0;
}
