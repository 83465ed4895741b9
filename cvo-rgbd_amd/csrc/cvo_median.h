// cvo_median.h -- the device side of the median contract of include/cvo_frontend.h (at cvo_fe_depth_median) behind one
// enqueue function: what cvo_frontend.hip (every kind of frame) and cvo_fe_median_plane (any uint16 plane) share.
#ifndef CVO_MEDIAN_H
#define CVO_MEDIAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int FE_MEDIAN_TW = 64, FE_MEDIAN_TH = 16;   // the tile of one workgroup

// One plane's filter; w x h pixels, dense rows.  Every pointer is device memory; a and b are two planes.
struct FeMedianArgs {
    const uint16_t *a;    // w*h: A, 0 = none
    uint16_t *b;          // w*h: B
    uint8_t *flags;       // w*h: MEDIAN, CVO_FE_MEDIAN_*
    uint32_t *counts;     // two words per workgroup, (changed, filled) of its tile, workgroup (bx, by) at
                          // 2*(by*tiles_x + bx); or null.  Every word is written: nothing to zero beforehand.
    int w, h;
    int radius, fill_min;
};

inline int fe_median_tiles_x(int w) { return (w + FE_MEDIAN_TW - 1) / FE_MEDIAN_TW; }
inline int fe_median_tiles_y(int h) { return (h + FE_MEDIAN_TH - 1) / FE_MEDIAN_TH; }

// One launch, nothing that waits for the host, no memset: capturable.  The caller has checked the settings
// (cvo_fe_check_depth_median) and the sizes (1 .. 8192 each way).
void fe_median_enqueue(const FeMedianArgs &a, hipStream_t s);

#endif
