// cvo_infill.h -- the device side of the infill contract of include/cvo_frontend.h (at cvo_fe_depth_infill) behind one
// enqueue function: what cvo_frontend.hip (every kind of frame) and cvo_fe_infill_plane (any uint16 plane) share.
#ifndef CVO_INFILL_H
#define CVO_INFILL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int FE_INFILL_TW = 64, FE_INFILL_TH = 16;        // the tile of one workgroup
constexpr int FE_INFILL_GX_MAX = 15, FE_INFILL_GY_MAX = 31;   // the largest gap_x and gap_y (cvo_fe_check_depth_infill)

// One plane's stage; w x h pixels, dense rows.  Every pointer is device memory; s and f are two planes.
struct FeInfillArgs {
    const uint16_t *s;    // w*h: S, 0 = none
    uint16_t *f;          // w*h: F
    uint8_t *flags;       // w*h: INFILL, CVO_FE_INFILL_*
    uint32_t *counts;     // two words per workgroup, (filled by the row pass, filled by the column pass) of its tile,
                          // workgroup (bx, by) at 2*(by*tiles_x + bx); or null.  Every word is written: nothing to
                          // zero beforehand.
    int w, h;
    int gap_x, gap_y;
    float jump_rel;
};

inline int fe_infill_tiles_x(int w) { return (w + FE_INFILL_TW - 1) / FE_INFILL_TW; }
inline int fe_infill_tiles_y(int h) { return (h + FE_INFILL_TH - 1) / FE_INFILL_TH; }

// One launch, nothing that waits for the host, no memset: capturable.  The caller has checked the settings
// (cvo_fe_check_depth_infill) and the sizes (1 .. 8192 each way).
void fe_infill_enqueue(const FeInfillArgs &a, hipStream_t s);

#endif
