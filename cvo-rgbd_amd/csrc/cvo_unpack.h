// cvo_unpack.h -- the device side of the unpack contract of include/cvo_frontend.h (at CVO_FE_PIXEL_*) behind one
// enqueue function: what cvo_frontend.hip (every colour image of every kind of frame) and cvo_fe_unpack_image (any
// packed image) share.
#ifndef CVO_UNPACK_H
#define CVO_UNPACK_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

constexpr int FE_UNPACK_TW = 64, FE_UNPACK_TH = 16;   // the tile of one workgroup of a Bayer instance

// One launch's images: `images` (1, or 2 for a stereo pair) of one format and one size, w x h pixels, dense rows
// (cvo_fe_pixel_layout: rows * row_bytes bytes each).  Every pointer is device memory from an allocation of its own
// (the kernel's dword accesses rely on a base address that is a multiple of four).
struct FeUnpackArgs {
    const uint8_t *src[2];   // the packed images
    uint8_t *dst[2];         // w*h*3 each: B, G, R
    int w, h;
    int format;              // CVO_FE_PIXEL_*, not CVO_FE_PIXEL_BGR8: that layout is not unpacked, it is the output
    int images;
};

// the layout table of the contract; false for an unknown format or a size the format does not fit
bool fe_unpack_layout(int format, int w, int h, size_t *row_bytes, int *rows);

// One launch, nothing that waits for the host, no memset: capturable.  The caller has checked the format against the
// size (cvo_fe_check_pixel_format) and the sizes (1 .. 8192 each way, or a context's).
void fe_unpack_enqueue(const FeUnpackArgs &a, hipStream_t s);

#endif
