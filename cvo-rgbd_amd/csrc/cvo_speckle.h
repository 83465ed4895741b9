// cvo_speckle.h -- the device side of the speckle contract of include/cvo_frontend.h (at cvo_fe_speckle) behind one
// enqueue function: what cvo_frontend.hip (a stereo frame) and cvo_fe_filter_speckles (any uint16 plane) share.
#ifndef CVO_SPECKLE_H
#define CVO_SPECKLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// One plane's filter; w x h pixels, dense rows.  Every pointer is device memory.
struct FeSpeckleArgs {
    uint16_t *plane;      // w*h: Q, 0 = none; filtered in place
    uint8_t *flags;       // w*h: CVO_FE_STEREO_SPECKLE is ORed in where a pixel goes; or null
    uint16_t *depth;      // w*h: zeroed where a pixel goes; or null
    uint32_t *labels;     // w*h: the union-find's parents (a pixel's own index at a root, FE_SPECKLE_NONE where Q == 0)
    uint32_t *sums;       // w*h: a component's pixel count, at its root
    uint32_t *sizes;      // w*h: SIZE of the contract when the last kernel has run (a tile's partial counts before)
    uint32_t *removed;    // one word: the number of pixels that went
    int w, h;
    int max_size, max_diff;
};

// Four launches in stream order (three for a plane of one tile), nothing between them that waits for the host, no
// memset: capturable.  The caller has checked the settings (cvo_fe_check_speckle) and the sizes (1 .. 8192 each way).
void fe_speckle_enqueue(const FeSpeckleArgs &a, hipStream_t s);

#endif
