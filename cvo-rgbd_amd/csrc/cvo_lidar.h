// cvo_lidar.h -- the device side of the LiDAR contract of include/cvo_frontend.h (at cvo_fe_lidar) behind two enqueue
// functions: what cvo_frontend.hip (a frame of a context with a scan source) and cvo_fe_project_points (any scan,
// without a context) share.  Between the two launches stands k_fe_depth_final of cvo_frontend.hip, the depth camera's.
// Under the sweep contract (at cvo_fe_lidar_sweep) the projection is another instance of the same kernel template.
#ifndef CVO_LIDAR_H
#define CVO_LIDAR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvo_lidar_stage.h"   // FE_LIDAR_HEADER and the layout of a staged scan

constexpr int FE_LIDAR_TW = 64, FE_LIDAR_TH = 16;   // the tile of one workgroup of the cull
constexpr int FE_LIDAR_RMAX = 7;                    // the largest half-width of the occlusion window
constexpr int FE_LIDAR_MAX_POINTS = 1 << 21;

// A scan as the device holds it: a header whose first word is the number of points of THIS frame (cvo_lidar_stage.h),
// and behind it the points, three floats each, packed.  One buffer and one copy, so that a captured frame carries a
// count that changes.
struct FeLidarProjectArgs {
    const int32_t *count;   // the header: count[0] = n
    const float *points;    // 3 * capacity floats
    uint32_t *z;            // w * h, 0xFFFFFFFF where nothing was seen yet
    int capacity;           // the launch covers this many points; threads at or beyond n return
    int w, h, splat;
    float min_range, max_range;
    float R[9], T[3];
    float cam[5];           // the colour camera: depth scale, fx, fy, cx, cy
};

// The projection under the sweep contract: the arguments above and the sweep's.  The twist of THIS frame stands in the
// header behind the count (words FE_LIDAR_TWIST_WORD ..), so that a captured frame carries a twist that changes.  Under
// a field mode (CVO_FE_SWEEP_TIME_F32, CVO_FE_SWEEP_TIME_U32) `base.points` are records of four words, x y z and the
// raw time word, 16 bytes apart and aligned; under CVO_FE_SWEEP_AZIMUTH three floats, as above.
struct FeLidarSweepArgs {
    FeLidarProjectArgs base;
    float time_origin, time_scale, phase0, direction, s_ref;   // of cvo_fe_lidar_sweep; direction as a float, +1 or -1
    float *phase;   // n floats or NULL: s of every point (NaN for one skipped before it has a phase)
    float *moved;   // 3n floats or NULL: p' of every point (NaN likewise)
};

struct FeLidarCullArgs {
    const uint16_t *p0;   // w*h: P0
    uint16_t *p;          // w*h: P (another plane than p0)
    uint8_t *flags;       // w*h: CVO_FE_LIDAR_*
    int w, h, rx, ry;
    float occl_rel;
};

// One launch each, nothing that waits for the host, no memset: capturable.  The caller has checked the settings
// (cvo_fe_check_lidar, cvo_fe_check_lidar_sweep), the sizes (1 .. 8192 each way) and capacity >= 1.  `mode` is one of
// CVO_FE_SWEEP_*.
void fe_lidar_project_enqueue(const FeLidarProjectArgs &a, hipStream_t s);
void fe_lidar_project_sweep_enqueue(int mode, const FeLidarSweepArgs &a, hipStream_t s);
void fe_lidar_cull_enqueue(const FeLidarCullArgs &a, hipStream_t s);

#endif
