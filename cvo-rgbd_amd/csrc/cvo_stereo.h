// cvo_stereo.h -- what cvo_frontend.hip and cvo_stereo.hip share: the grey formula of the front end (one copy:
// k_fe_level0 and the stereo matcher), and the device side of the stereo contract of include/cvo_frontend.h
// (at cvo_fe_stereo) behind one enqueue function.
#ifndef CVO_STEREO_H
#define CVO_STEREO_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// cv::cvtColor RGB2GRAY on 8-bit data, channel 0 taken as R (ref src/pcd_generator.cpp:389): STAGE_GRAY
__host__ __device__ inline int fe_grey(int c0, int c1, int c2)
{
    return (c0 * 4899 + c1 * 9617 + c2 * 1868 + (1 << 13)) >> 14;
}

// One stereo frame's planes; w x h pixels, D = max_disp.  Every pointer is device memory of the context.
struct FeStereoArgs {
    const uint8_t *left, *right;    // w*h*3: the two colour images
    uint8_t *gray_l, *gray_r;       // w*h
    uint64_t *census_l, *census_r;  // w*h
    uint16_t *sum;                  // w*h*D: S, index (y*w + x)*D + d
    uint32_t *win;                  // w*h: q | d* << 16 | dR << 23 | UNIQUE << 30, between the last two kernels
    const uint16_t *table;          // 16*D: U(q)
    uint16_t *disparity;            // w*h
    uint8_t *flags;                 // w*h: CVO_FE_STEREO_*
    uint16_t *depth;                // w*h: the depth plane the gate or level 0 reads
    const uint8_t *valid;           // w*h: bit 0 V_L, bit 1 V_R of the rig contract (k_fe_stereo_rectify's), or null: no rig
    int w, h, D;
    int min_disp, p1, p2, uniqueness, lr_max;
    uint32_t paths;                 // the path mask (cvo_fe_set_stereo_paths): bit b set, direction b of contract 4 is summed
};

// grey and census of both images, one path pass per set bit of `paths` in bit order, winner and right map, tests and
// lookup: four launches and one per path, in stream order (capturable).  With `valid` the last kernel is the instance that also applies the rig contract's
// OUTSIDE rule; without, the one that does not know of it.  The caller has checked the settings (cvo_fe_check_stereo,
// cvo_fe_check_stereo_paths) and the sizes.
void fe_stereo_enqueue(const FeStereoArgs &a, hipStream_t s);

#endif
