// limits.h -- the limits that split a measurement unit's call (lc/, mask/, strip/, sub/, inject/, stars/, stack/) and the record of
// the split, as the units see them (include/lfdmi.h: lfdmi_debug_unit_limits, lfdmi_debug_unit_split; definitions in limits.hip).
// Host side only, like ../unit.h.  A context's entry is kept beside the context, keyed by its handle, and not in lfdmi_ctx itself:
// lfdmi.hip and unit.h are part of the detection kernels' translation unit, which a test hook has no business changing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../unit.h"

enum { LIM_LIST_PAIRS, LIM_STAGE_BYTES, LIM_CELL_BYTES, LIM_RENDER_BLOCKS, LIM_STARS_REC_BYTES, LIM_STACK_PART_BYTES, LIM_KINDS };
struct UnitSplit {
    int64_t chunks;     // chunks of jobs (stars: of frames; stack: groups of frames)
    int64_t batches;    // strips: batches of cells
    int64_t grid;       // the largest grid of persistent blocks launched
    int64_t launches;   // stack: launches of the first pass of the first group
};
// what a context keeps for its unit calls: the lowered limits (0: none) and the split of the last call
struct UnitState {
    int64_t limit[LIM_KINDS];
    UnitSplit split;
    // a unit's compiled limit `compiled`, or the context's lower one of kind `which`
    size_t limit_of(int which, size_t compiled) const {
        const int64_t v = limit[which];
        return v > 0 && (uint64_t)v < compiled ? (size_t)v : compiled;
    }
};
// a unit call's start: the context's state with the split zeroed, which the unit fills in as it goes; valid until the context's
// next unit call or lfdmi_debug_unit_limits(ctx, NULL).  A context on which neither debug entry was called has no state: the
// call gets the thread's blank one (no limit; its split is read by nobody)
LFD_HIDDEN UnitState *ctx_unit(lfdmi_ctx *ctx);
