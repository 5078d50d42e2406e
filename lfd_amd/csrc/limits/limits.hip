// limits.hip -- lfdmi_debug_unit_limits and lfdmi_debug_unit_split (include/lfdmi.h), and what the measurement units read of them
// (limits.h).  Its own translation unit in its own directory, like the units: the detection kernels' code object does not change
// with it.  No kernel, no device memory: a table of the contexts on which one of the two entries has been called.  A context that
// never calls them has no entry: its unit calls find none, use the compiled limits and record their split nowhere that lasts.
#include <map>
#include <mutex>

#include "limits.h"

static_assert(sizeof(lfdmi_unit_limits) == LIM_KINDS * sizeof(int64_t), "a field per kind of limit");

namespace {
std::mutex g_lock;
std::map<lfdmi_ctx *, UnitState> g_table;   // (std::map: a reference to an entry stays valid while others come and go)

UnitState &entry_of(lfdmi_ctx *ctx) {
    std::lock_guard<std::mutex> hold(g_lock);
    return g_table[ctx];   // (a new entry is zeroed: no limit, no split)
}
}   // namespace

LFD_HIDDEN UnitState *ctx_unit(lfdmi_ctx *ctx) {
    static thread_local UnitState none;   // no entry: no limit, and a split nobody reads
    UnitState *e = &none;
    {
        std::lock_guard<std::mutex> hold(g_lock);
        auto it = g_table.find(ctx);
        if (it != g_table.end()) e = &it->second;
    }
    if (e == &none) none = UnitState();
    e->split = UnitSplit();
    return e;
}

extern "C" int lfdmi_debug_unit_limits(lfdmi_ctx *ctx, const lfdmi_unit_limits *lim) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!lim) {   // every default again, and the context's entry goes (lfdmi_ctx_destroy does not know of the table)
        std::lock_guard<std::mutex> hold(g_lock);
        g_table.erase(ctx);
        return 0;
    }
    const int64_t v[LIM_KINDS] = {lim->list_pairs, lim->stage_bytes, lim->cell_bytes, lim->render_blocks, lim->stars_rec_bytes, lim->stack_part_bytes};
    for (int64_t x : v)
        if (x < 0) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_debug_unit_limits: a limit is 0 (the default) or positive");
    UnitState &e = entry_of(ctx);
    for (int k = 0; k < LIM_KINDS; k++) e.limit[k] = v[k];
    return 0;
}

extern "C" int lfdmi_debug_unit_split(lfdmi_ctx *ctx, int64_t *out, int n) {
    if (!ctx) return LFDMI_ERR_ARG;
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!out || n < 0) return ctx_fail(ctx, LFDMI_ERR_ARG, "lfdmi_debug_unit_split: bad argument");
    const UnitSplit s = entry_of(ctx).split;
    const int64_t v[LFDMI_UNIT_SPLIT_COUNTS] = {s.chunks, s.batches, s.grid, s.launches};
    for (int k = 0; k < n; k++) out[k] = k < LFDMI_UNIT_SPLIT_COUNTS ? v[k] : 0;
    return 0;
}
