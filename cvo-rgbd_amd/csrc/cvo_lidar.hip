// cvo_lidar.hip -- a LiDAR scan in place of a depth image on MI355X (gfx950): the device side of the LiDAR contract of
// include/cvo_frontend.h (at cvo_fe_lidar).  The restatement tests/fe_lidar_ref.py holds the planes and the flags to it
// by bytes, so every parenthesis of the float32 arithmetic here is part of the contract (-ffp-contract=off: nothing
// is fused).
//
// k_fe_lidar_project, one thread per point: the point goes into the colour camera's frame, through its pinhole, and
//   posts its depth to the (2*splat+1)^2 pixels around its nearest pixel of a 32-bit z-buffer with an integer
//   atomicMin whose result nobody reads (no-return, relaxed, agent scope: integer minima commute, so the plane does
//   not depend on the order of the points).  Every write is bounded here: x in [0, w), y in [0, h).  The number of
//   points is read from device memory -- the header in front of the points, copied with them -- so that a frame whose
//   launches sit in a captured graph takes a count that changes from frame to frame: the grid covers the scan's
//   capacity and the threads at or beyond the count return.  The kernel is a template on the sweep mode: instance 0
//   is the above and nothing else; the instances CVO_FE_SWEEP_* put the sweep contract (at cvo_fe_lidar_sweep: the
//   point's phase, then the scanner's motion since the image's phase, from the twist in the same header) in front of
//   the projection, in the same pass.  The restatement tests/fe_lidar_sweep_ref.py holds them by bits.
// k_fe_depth_final of cvo_frontend.hip, the depth camera's, then turns the z-buffer into P0 and arms it again.
// k_fe_lidar_cull (only with occl_rel > 0), one workgroup per tile of 64 x 16 pixels: the tile of P0 with a halo of
//   (rx, ry) goes to LDS as 16-bit keys value - 1, so that "none" (0) becomes 65535 and sorts behind every depth, 65535
//   (key 65534) included; a cell outside the image is "none".  The minimum of the window is separable: along the rows
//   into a second LDS plane, then down the columns.  A pixel with a depth is in its own window, so its minimum is a
//   depth.  The comparison is one float32 multiplication and one comparison, the shape of the gate's jump test.  P goes
//   to another plane than P0: nothing is computed in place.
#include "cvo_lidar.h"

#include "cvo_frontend.h"

namespace {

constexpr int LD_BLOCK = 256;
constexpr int LD_TW = FE_LIDAR_TW, LD_TH = FE_LIDAR_TH, LD_R = FE_LIDAR_RMAX;
constexpr int LD_S = LD_TW + 2 * LD_R + 2;   // 80 cells per LDS row of keys
constexpr int LD_ROWS = LD_TH + 2 * LD_R;    // 30 rows at the most
static_assert(LD_TW * LD_TH == 4 * LD_BLOCK, "four pixels of the tile per thread");

// a1*b2 - a2*b1 by components
__device__ __forceinline__ void ld_cross(const float a[3], const float b[3], float c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a point that has no phase: NaN where the stand-alone entry asked for phase and p'
__device__ __forceinline__ void ld_no_phase(const FeLidarSweepArgs &a, const int i)
{
    const float nan = __uint_as_float(0x7FC00000u);
    if (a.phase) a.phase[i] = nan;
    if (a.moved) a.moved[3 * (size_t)i] = a.moved[3 * (size_t)i + 1] = a.moved[3 * (size_t)i + 2] = nan;
}

// The sweep contract on point i: its phase and the move.  False: the point is skipped (step 1, or a time that is not
// finite); else (x, y, z) is p'.  The words of the header -- the frame's twist -- and the arguments are the same for
// every lane of a wave.  The arguments and the count arrive through scalar loads; the twist does under the azimuth
// mode, and under the field modes as two vector loads of one address for the whole wave (one line, 24 bytes), which is
// how the compiler orders them behind the branch that stores NaN.  The point's own words are vector loads, one
// 16-byte load under a field mode.
template <int MODE>
__device__ __forceinline__ bool ld_sweep_point(const FeLidarSweepArgs &args, const int i, float &x, float &y, float &z)
{
    const FeLidarProjectArgs &a = args.base;
    // (read first, in front of every store of the thread: the loads are then scalar ones, like the count's)
    const float *header = reinterpret_cast<const float *>(a.count) + FE_LIDAR_TWIST_WORD;
    const float twist[6] = {header[0], header[1], header[2], header[3], header[4], header[5]};
    float p[3];
    uint32_t word = 0u;
    if constexpr (MODE == CVO_FE_SWEEP_AZIMUTH) {
        p[0] = a.points[3 * (size_t)i]; p[1] = a.points[3 * (size_t)i + 1]; p[2] = a.points[3 * (size_t)i + 2];
    } else {
        const float4 rec = reinterpret_cast<const float4 *>(a.points)[i];
        p[0] = rec.x; p[1] = rec.y; p[2] = rec.z;
        word = __float_as_uint(rec.w);
    }
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) { ld_no_phase(args, i); return false; }
    // the phase
    float s;
    if constexpr (MODE == CVO_FE_SWEEP_TIME_F32) {
        const float t = __uint_as_float(word);
        if (!isfinite(t)) { ld_no_phase(args, i); return false; }
        s = (t - args.time_origin) * args.time_scale;
        s = fminf(fmaxf(s, 0.0f), 1.0f);
    } else if constexpr (MODE == CVO_FE_SWEEP_TIME_U32) {
        s = (float)word * args.time_scale;
        s = fminf(fmaxf(s, 0.0f), 1.0f);
    } else {
        const float ax = fabsf(p[0]), ay = fabsf(p[1]);
        const float lo = fminf(ax, ay), hi = fmaxf(ax, ay);
        const float r = hi > 0.0f ? lo / hi : 0.0f;
        const float r2 = r * r;
        float q = ((((CVO_FE_SWEEP_ATAN_C5 * r2 + CVO_FE_SWEEP_ATAN_C4) * r2 + CVO_FE_SWEEP_ATAN_C3) * r2 + CVO_FE_SWEEP_ATAN_C2) * r2 +
                   CVO_FE_SWEEP_ATAN_C1) * r2 + CVO_FE_SWEEP_ATAN_C0;
        q = q * r;
        if (ay > ax) q = 0.25f - q;
        if (p[0] < 0.0f) q = 0.5f - q;
        if (p[1] < 0.0f) q = -q;
        s = args.direction * q + args.phase0;
        s = s - floorf(s);
    }
    // the move
    const float am = s - args.s_ref;
    float w[3], tau[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[k] = am * twist[k]; tau[k] = am * twist[3 + k]; }
    const float t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float A = ((((CVO_FE_SWEEP_A5 * t2 + CVO_FE_SWEEP_A4) * t2 + CVO_FE_SWEEP_A3) * t2 + CVO_FE_SWEEP_A2) * t2 + CVO_FE_SWEEP_A1) * t2 + CVO_FE_SWEEP_A0;
    const float B = ((((CVO_FE_SWEEP_B5 * t2 + CVO_FE_SWEEP_B4) * t2 + CVO_FE_SWEEP_B3) * t2 + CVO_FE_SWEEP_B2) * t2 + CVO_FE_SWEEP_B1) * t2 + CVO_FE_SWEEP_B0;
    const float Cc = (((CVO_FE_SWEEP_C4 * t2 + CVO_FE_SWEEP_C3) * t2 + CVO_FE_SWEEP_C2) * t2 + CVO_FE_SWEEP_C1) * t2 + CVO_FE_SWEEP_C0;
    float c1[3], c2[3], d1[3], d2[3], m[3];
    ld_cross(w, p, c1);
    ld_cross(w, c1, c2);
    ld_cross(w, tau, d1);
    ld_cross(w, d1, d2);
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = ((p[k] + A * c1[k]) + B * c2[k]) + ((tau[k] + B * d1[k]) + Cc * d2[k]);
    if (args.phase) args.phase[i] = s;
    if (args.moved) { args.moved[3 * (size_t)i] = m[0]; args.moved[3 * (size_t)i + 1] = m[1]; args.moved[3 * (size_t)i + 2] = m[2]; }
    x = m[0]; y = m[1]; z = m[2];
    return true;
}

template <int MODE> struct LdArgs { using type = FeLidarSweepArgs; };
template <> struct LdArgs<0> { using type = FeLidarProjectArgs; };
__device__ __forceinline__ const FeLidarProjectArgs &ld_base(const FeLidarProjectArgs &a) { return a; }
__device__ __forceinline__ const FeLidarProjectArgs &ld_base(const FeLidarSweepArgs &a) { return a.base; }

// MODE 0: the LiDAR contract alone, what a context without a sweep launches.  MODE CVO_FE_SWEEP_*: phase, move and
// projection of the sweep contract in one pass over the points.
template <int MODE>
__global__ void __launch_bounds__(LD_BLOCK) k_fe_lidar_project(const typename LdArgs<MODE>::type args)
{
    const FeLidarProjectArgs &a = ld_base(args);
    const int i = blockIdx.x * LD_BLOCK + threadIdx.x;
    if (i >= a.capacity || i >= a.count[0]) return;
    float x, y, z;
    if constexpr (MODE == 0) {
        x = a.points[3 * (size_t)i]; y = a.points[3 * (size_t)i + 1]; z = a.points[3 * (size_t)i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
    } else {
        if (!ld_sweep_point<MODE>(args, i, x, y, z)) return;
    }
    float Q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Q[k] = ((a.R[3 * k] * x + a.R[3 * k + 1] * y) + a.R[3 * k + 2] * z) + a.T[k];
    if (!(Q[2] > 0.0f)) return;   // (also a sum that is not a number)
    if ((a.min_range > 0.0f && Q[2] < a.min_range) || (a.max_range > 0.0f && Q[2] > a.max_range)) return;
    const float u = a.cam[1] * (Q[0] / Q[2]) + a.cam[3], v = a.cam[2] * (Q[1] / Q[2]) + a.cam[4];
    if (!(isfinite(u) && isfinite(v))) return;
    const float qf = rintf(Q[2] * a.cam[0]);
    if (!(qf >= 1.0f && qf <= 65535.0f)) return;
    const uint32_t q = (uint32_t)qf;
    // (clamped before the conversion: a point far outside lands 8 pixels outside, beyond any splat)
    const int xi = (int)rintf(fminf(fmaxf(u, -8.0f), (float)(a.w + 8)));
    const int yi = (int)rintf(fminf(fmaxf(v, -8.0f), (float)(a.h + 8)));
    const int x0 = max(xi - a.splat, 0), x1 = min(xi + a.splat, a.w - 1);
    const int y0 = max(yi - a.splat, 0), y1 = min(yi + a.splat, a.h - 1);
    for (int py = y0; py <= y1; ++py)
        for (int px = x0; px <= x1; ++px)
            (void)__hip_atomic_fetch_min(a.z + ((size_t)py * a.w + px), q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(LD_BLOCK) k_fe_lidar_cull(const FeLidarCullArgs a)
{
    __shared__ uint16_t s_k[LD_ROWS * LD_S];    // keys of P0: the tile and its halo
    __shared__ uint16_t s_r[LD_ROWS * LD_TW];   // the minima along the rows, for the tile's columns
    const int tid = (int)threadIdx.x;
    const int tx0 = blockIdx.x * LD_TW, ty0 = blockIdx.y * LD_TH;
    const int rows = LD_TH + 2 * a.ry, cols = LD_TW + 2 * a.rx;   // (rx, ry in [0, 7]: cvo_fe_check_lidar)
    // phase 1: LDS cell (r, c) is pixel (tx0 - rx + c, ty0 - ry + r).  A fixed number of steps over whole LDS rows: the
    // divisor is a constant, and a thread's loads are all in flight before the first is stored.  The cells beyond `cols`
    // hold "none" and are not read.
    constexpr int STEPS = (LD_ROWS * LD_S + LD_BLOCK - 1) / LD_BLOCK;
    uint32_t v[STEPS];
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int idx = k * LD_BLOCK + tid;
        const int r = idx / LD_S, c = idx - r * LD_S;
        const int x = tx0 - a.rx + c, y = ty0 - a.ry + r;
        const bool inside = r < rows && c < cols && x >= 0 && x < a.w && y >= 0 && y < a.h;
        v[k] = inside ? (uint32_t)a.p0[(size_t)y * a.w + x] : 0u;
    }
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int idx = k * LD_BLOCK + tid;
        if (idx < rows * LD_S) s_k[idx] = (uint16_t)(v[k] - 1u);
    }
    __syncthreads();
    // phase 2: along the rows; the widest window's fifteen cells are read (they lie in the row) and those of this window count
    const uint32_t nx = 2u * (uint32_t)a.rx, ny = 2u * (uint32_t)a.ry;
    for (int idx = tid; idx < rows * LD_TW; idx += LD_BLOCK) {
        const int r = idx / LD_TW, c = idx - r * LD_TW;
        uint32_t m = 0xFFFFu;
#pragma unroll
        for (uint32_t j = 0; j <= 2u * LD_R; ++j) {
            const uint32_t cell = s_k[r * LD_S + c + (int)j];
            m = min(m, j <= nx ? cell : 0xFFFFu);
        }
        s_r[r * LD_TW + c] = (uint16_t)m;
    }
    __syncthreads();
    // phase 3: down the columns, and the test
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = k * LD_BLOCK + tid;
        const int r = idx / LD_TW, c = idx - r * LD_TW;
        const int x = tx0 + c, y = ty0 + r;
        if (x >= a.w || y >= a.h) continue;
        const uint32_t own = (uint32_t)(uint16_t)(s_k[(r + a.ry) * LD_S + c + a.rx] + 1u);
        uint32_t out = 0u, fl = 0u;
        if (own != 0u) {
            uint32_t mk = 0xFFFFu;
#pragma unroll
            for (uint32_t j = 0; j <= 2u * LD_R; ++j) {   // (row r + 14 at the most: inside s_r)
                const uint32_t cell = s_r[(r + (int)j) * LD_TW + c];
                mk = min(mk, j <= ny ? cell : 0xFFFFu);
            }
            const uint32_t m = mk + 1u;   // (a depth: the pixel counts itself)
            const bool occluded = (float)(int)(own - m) > a.occl_rel * (float)m;
            out = occluded ? 0u : own;
            fl = (uint32_t)CVO_FE_LIDAR_HIT | (occluded ? (uint32_t)CVO_FE_LIDAR_OCCLUDED : 0u);
        }
        const size_t i = (size_t)y * a.w + x;
        a.p[i] = (uint16_t)out;
        a.flags[i] = (uint8_t)fl;
    }
}

}   // namespace

void fe_lidar_project_enqueue(const FeLidarProjectArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_fe_lidar_project<0>, dim3((a.capacity + LD_BLOCK - 1) / LD_BLOCK), dim3(LD_BLOCK), 0, s, a);
}

void fe_lidar_project_sweep_enqueue(int mode, const FeLidarSweepArgs &a, hipStream_t s)
{
    const dim3 grid((a.base.capacity + LD_BLOCK - 1) / LD_BLOCK), block(LD_BLOCK);
    if (mode == CVO_FE_SWEEP_TIME_F32) hipLaunchKernelGGL(k_fe_lidar_project<CVO_FE_SWEEP_TIME_F32>, grid, block, 0, s, a);
    else if (mode == CVO_FE_SWEEP_TIME_U32) hipLaunchKernelGGL(k_fe_lidar_project<CVO_FE_SWEEP_TIME_U32>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_fe_lidar_project<CVO_FE_SWEEP_AZIMUTH>, grid, block, 0, s, a);
}

void fe_lidar_cull_enqueue(const FeLidarCullArgs &a, hipStream_t s)
{
    const dim3 tiles((a.w + LD_TW - 1) / LD_TW, (a.h + LD_TH - 1) / LD_TH);
    hipLaunchKernelGGL(k_fe_lidar_cull, tiles, dim3(LD_BLOCK), 0, s, a);
}
