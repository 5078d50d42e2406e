// k_strip_geo.h -- step 2 of the trail strips on the host, shared by strip.hip and by the trail subtraction (sub/sub.hip), whose
// BAD_SEGMENT and TOO_LONG are decided exactly as the strips decide theirs: one function, so the two cannot drift apart.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../../include/lfdmi.h"
#include "k_strip.h"

// step 2 of the definition: LFDMI_STRIP_OK, LFDMI_STRIP_BAD_SEGMENT or LFDMI_STRIP_TOO_LONG; *K_out: K of a good segment
static inline int strip_geometry(const lfdmi_strip_segment &s, const lfdmi_strip_params &p, int max_sec, int max_cells, StripSeg &o, int *K_out) {
    const double c[4] = {s.x1, s.y1, s.x2, s.y2};
    for (double v : c)
        if (!std::isfinite(v) || fabs(v) > 1e6) return LFDMI_STRIP_BAD_SEGMENT;
    if (!std::isfinite(s.half) || !(s.half > 0.0)) return LFDMI_STRIP_BAD_SEGMENT;
    const double dx = s.x2 - s.x1, dy = s.y2 - s.y1;
    const double L = sqrt(dx * dx + dy * dy);
    if (L == 0.0) return LFDMI_STRIP_BAD_SEGMENT;
    const double inv_s = 1.0 / p.sec_len, inv_u = 1.0 / p.step;
    const double kk = ceil(s.half * inv_u - 0.5);
    if (2.0 * kk + 1.0 > (double)LFDMI_STRIP_MAX_OFF) return LFDMI_STRIP_BAD_SEGMENT;
    const int K = std::max(0, (int)kk), n_off = 2 * K + 1;
    const double ns = ceil(L * inv_s);
    if (ns > (double)max_sec) return LFDMI_STRIP_TOO_LONG;
    const int n_sec = std::max(1, (int)ns);
    if ((int64_t)n_sec * n_off > (int64_t)max_cells) return LFDMI_STRIP_TOO_LONG;
    o.x1 = s.x1; o.y1 = s.y1;
    o.ex = dx / L; o.ey = dy / L;
    o.nx = -o.ey; o.ny = o.ex;
    o.half = s.half; o.L = L;
    o.inv_s = inv_s; o.inv_u = inv_u; o.kc = (double)K + 0.5;
    o.n_sec = n_sec; o.n_off = n_off;
    o.base = 0;
    *K_out = K;
    return LFDMI_STRIP_OK;
}
