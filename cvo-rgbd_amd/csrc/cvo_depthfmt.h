// cvo_depthfmt.h -- the device side of the depth-format contract of include/cvo_frontend.h (at CVO_FE_DEPTH_*) behind
// one enqueue function: what cvo_frontend.hip (the depth image of a frame, from the context's landing buffer or from a
// caller's device image read in place) and cvo_fe_convert_depth (any plane) share.
#ifndef CVO_DEPTHFMT_H
#define CVO_DEPTHFMT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// One launch: a w x h plane of float32 or float16 values, rows `src_pitch` BYTES apart, becomes w x h uint16, dense.
// `src` is aligned to the value size and `src_pitch` is a multiple of it (and at least the row); nothing more is
// asked of either: the kernel takes its wide loads and stores only where an address allows them.
struct FeDepthConvertArgs {
    const void *src;
    size_t src_pitch;
    uint16_t *dst;
    int w, h;
    int format;      // CVO_FE_DEPTH_F32 or CVO_FE_DEPTH_F16
    float unit;      // metres per input unit
    float scale;     // depth units per metre of whatever reads dst first
};

// bytes of one value of a format; 0 for an unknown one
size_t fe_depth_item(int format);
// what cvo_fe_check_depth_format accepts
bool fe_depth_format_ok(int format, float unit);

// One launch, nothing that waits for the host: capturable.  The caller has checked the format and the sizes
// (1 .. 8192 each way, or a context's).
void fe_depth_convert_enqueue(const FeDepthConvertArgs &a, hipStream_t s);

#endif
