// cvo_bin.h -- the device side of the binning contract of include/cvo_frontend.h (at cvo_fe_binning) behind one enqueue
// function: what cvo_frontend.hip (every kind of frame) and cvo_fe_bin_image / cvo_fe_bin_depth (any image) share.
#ifndef CVO_BIN_H
#define CVO_BIN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// One frame's bin: `planes` planes (1 or 2) of the working size w x h, each from an input plane of factor*w x factor*h,
// dense rows.  Every pointer is device memory from an allocation of its own (so that it starts on a dword).
struct FeBinArgs {
    const void *src[2];   // plane p's input: B G R bytes (fw*fh*3), or uint16 depths (fw*fh)
    void *dst[2];         // ... and its output: w*h*3 bytes, or w*h uint16
    int is_depth[2];      // plane p is a depth plane
    int w, h;
    int factor;           // 2, 3 or 4
    int depth_min;        // of the contract; read for depth planes
    int planes;
};

// One launch for all planes, nothing that waits for the host, no memset: capturable.  The caller has checked the
// settings (cvo_fe_check_binning) and the sizes.
void fe_bin_enqueue(const FeBinArgs &a, hipStream_t s);

#endif
