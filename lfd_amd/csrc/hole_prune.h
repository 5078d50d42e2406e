// hole_prune.h -- certain rejection of a hole border by lfd's rectangle filter, from three values of the hole alone.
// Plain C++ without includes: k_frame.h uses it on the device, tools/hole_prune_check.cpp compiles it for the host.
#pragma once

#if defined(__HIPCC__)
#define LFD_HOST_DEVICE __host__ __device__
#else
#define LFD_HOST_DEVICE
#endif

// A hole is a 4-connected component of 0-pixels that does not touch the frame.  n: its pixel count; wb, hb: the coordinate
// extents of its border, which is the hole's bounding box grown by one pixel on every side (xmax - xmin + 2, ymax - ymin + 2).
// True: the filter of rect_from_hull (`length > minLen && width > minLen && length / width > lwTresh` on the border's
// minAreaRect) cannot pass, whatever else the frame holds.  With D^2 = wb^2 + hb^2 (the border's bounding-box diagonal):
//  (a) the hull of the border contains the unit diamond |dx| + |dy| <= 1 around every hole pixel (its four neighbours are
//      hole or border pixels; islands inside the hole lie inside the border too); a point lies inside at most two such
//      diamonds of area 2, so the hull's area A >= n, and length / width = length^2 / (length * width) <= D^2 / A <= D^2 / n;
//  (b) an accepted rectangle has length > lwTresh * width > lwTresh * minLen, and length <= D.
// The 0.1 % margin is the one rect_from_hull's own D^2 / A test keeps over the float32 arithmetic of the rectangle.
LFD_HOST_DEVICE inline bool hole_border_rejected(int n, int wb, int hb, double minLen, double lwTresh) {
    if (!(lwTresh > 0)) return false; // (b) follows from `length / width > lwTresh` as well: neither bound holds without it
    const double d2 = (double)((long long)wb * wb + (long long)hb * hb);
    if (d2 < lwTresh * (double)n * 0.999) return true;
    if (minLen > 0) {
        const double f = lwTresh * minLen;
        if (d2 <= f * f * 0.999) return true;
    }
    return false;
}
