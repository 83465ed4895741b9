// cvo_frontend.hip -- the RGB-D front end on MI355X (gfx950): C-ABI of
// include/cvo_frontend.h.  One frame = ~20 small launches on one stream; every
// kernel is a per-pixel or per-cell pass over a 640x480-class image (0.3 M pixels,
// ~1 MB per plane), i.e. launch- and latency-bound, not bandwidth-bound; the
// data-dependent decisions of the selector (second pass or not, sub-sampling
// threshold) are taken by one-thread kernels on the device so that the host does
// not have to look at the frame before the cloud is ready.
//
// What each kernel restates is cited at the kernel.  The arithmetic contract of the
// library holds here too (-ffp-contract=off, correctly rounded sqrt / divide).
//
// This file holds every kernel and everything that launches one: a frame's sequence, submit and collect, the stage
// reader, the stand-alone projection, and the context's creation and end.  The context itself is cvo_fe_ctx.h's, the
// settings are cvo_fe_settings.cpp's and the host-only calibration helpers cvo_fe_calib.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "cvo_bin.h"
#include "cvo_fe_ctx.h"
#include "cvo_fe_rules.h"
#include "cvo_infill.h"
#include "cvo_lidar.h"
#include "cvo_lock.h"
#include "cvo_median.h"
#include "cvo_speckle.h"
#include "cvo_stereo.h"
#include "cvo_unpack.h"
#include "cvo_input.h"

using namespace cvo_fe;
using cvo_fe_rules::lidar_ok;
using cvo_fe_rules::sweep_ok;
using cvo_fe_rules::twist_ok;

namespace {

constexpr int FE_BLOCK = 256;
constexpr int FE_CHUNK = 4 * FE_BLOCK;   // pixels per block of the ordered (scan) kernels

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// exclusive scan of one int per thread over a 256-thread block; *total = block sum
__device__ __forceinline__ int block_excl_scan(int v, int *total)
{
    __shared__ int s_w[FE_BLOCK / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();   // (s_w may still be read by a previous call)
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < FE_BLOCK / 64; ++q) {
        if (q < wid) base += s_w[q];
        tot += s_w[q];
    }
    *total = tot;
    return base + inc - v;
}

// sum of cnt[0 .. b) by the whole block
__device__ __forceinline__ int block_base(const int *cnt, int b)
{
    __shared__ int s_r[FE_BLOCK / 64];
    int v = 0;
    for (int q = threadIdx.x; q < b; q += FE_BLOCK) v += cnt[q];
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int q = 0; q < FE_BLOCK / 64; ++q) s += s_r[q];
    return s;
}

// The first stage of a frame whose camera has a lens distortion: both images resampled through
// the context's map (the rectification contract of include/cvo_frontend.h; the map itself is
// cvo_fe_rectify_map's, made on the host once per model).  Colour: bilinear at 1/32 pixel in
// integers over four taps with replicated borders; depth: the nearest sample, 0 outside the
// image.  A thread owns four consecutive output pixels: two 16-byte loads of the map, three
// dword stores of colour and one 8-byte store of depth, so that a wave writes whole lines
// instead of single bytes; the taps are gathers (neighbouring pixels share cache lines: the
// map is smooth).  The last, partial group of an image whose size is no multiple of four goes
// pixel by pixel.  No tap leaves the images whatever the map holds: every coordinate is
// clamped or tested here.  A null `dsrc` (a context with a depth camera: k_fe_depth_warp brings
// the raw depth into the rectified frame itself) leaves the depth plane alone.
// (the depth rule of the rectification contract: the nearest sample of a map entry, and whether it lies inside the image)
__device__ __forceinline__ bool fe_nearest(int qu, int qv, int w, int h, int *xn, int *yn)
{
    *xn = (qu + 16) >> 5;
    *yn = (qv + 16) >> 5;
    return *xn >= 0 && *xn < w && *yn >= 0 && *yn < h;
}

__device__ __forceinline__ void fe_rectify_pixel(const uint8_t *src, const uint16_t *dsrc, int w, int h, int qu, int qv,
                                                 int out[3], uint16_t *dout)
{
    const int x0 = qu >> 5, y0 = qv >> 5;   // floor: arithmetic shift
    const int ax = qu & 31, ay = qv & 31;
    const int xa = min(max(x0, 0), w - 1), xb = min(max(x0 + 1, 0), w - 1);
    const int ya = min(max(y0, 0), h - 1), yb = min(max(y0 + 1, 0), h - 1);
    const uint8_t *p00 = src + 3 * ((size_t)ya * w + xa), *p01 = src + 3 * ((size_t)ya * w + xb);
    const uint8_t *p10 = src + 3 * ((size_t)yb * w + xa), *p11 = src + 3 * ((size_t)yb * w + xb);
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 512) >> 10;
    int xn, yn;
    const bool inside = fe_nearest(qu, qv, w, h, &xn, &yn);
    *dout = (dsrc && inside) ? dsrc[(size_t)yn * w + xn] : (uint16_t)0;
}

__global__ void __launch_bounds__(FE_BLOCK) k_fe_rectify(const uint8_t *src, const uint16_t *dsrc, const int32_t *qu,
                                                         const int32_t *qv, int w, int h, uint8_t *dst, uint16_t *ddst)
{
    const int np = w * h;
    const int i0 = 4 * (blockIdx.x * FE_BLOCK + threadIdx.x);
    if (i0 >= np) return;
    if (i0 + 4 <= np) {
        const int4 u4 = *reinterpret_cast<const int4 *>(qu + i0), v4 = *reinterpret_cast<const int4 *>(qv + i0);
        const int us[4] = {u4.x, u4.y, u4.z, u4.w}, vs[4] = {v4.x, v4.y, v4.z, v4.w};
        uint32_t b[12];
        uint16_t d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int c[3];
            fe_rectify_pixel(src, dsrc, w, h, us[q], vs[q], c, &d[q]);
            b[3 * q] = (uint32_t)c[0]; b[3 * q + 1] = (uint32_t)c[1]; b[3 * q + 2] = (uint32_t)c[2];
        }
        uint32_t *o = reinterpret_cast<uint32_t *>(dst + 3 * (size_t)i0);   // 12 * (i0 / 4): dword aligned
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        if (dsrc)
            *reinterpret_cast<uint2 *>(ddst + i0) =
                make_uint2((uint32_t)d[0] | ((uint32_t)d[1] << 16), (uint32_t)d[2] | ((uint32_t)d[3] << 16));
    } else {
        for (int i = i0; i < np; ++i) {
            int c[3];
            uint16_t d;
            fe_rectify_pixel(src, dsrc, w, h, qu[i], qv[i], c, &d);
            dst[3 * (size_t)i] = (uint8_t)c[0]; dst[3 * (size_t)i + 1] = (uint8_t)c[1]; dst[3 * (size_t)i + 2] = (uint8_t)c[2];
            if (dsrc) ddst[i] = d;
        }
    }
}

// The first stage of a frame under a stereo rig (the rig contract of include/cvo_frontend.h, at cvo_fe_stereo_rig):
// both raw images resampled through their maps (cvo_fe_stereo_rig_map's, made on the host once per rig) in ONE
// launch, blockIdx.y the image, and the validity plane written.  The shape is k_fe_rectify's: a thread owns four
// consecutive output pixels of one image, loads its map entries as two 16-byte words, gathers the taps with
// fe_rectify_pixel (the one copy of the tap arithmetic; without a depth source) and stores three packed dwords of
// colour.  The validity byte of a pixel holds a bit of either camera, so one thread must write it: the left image's
// threads read the right map's entries of their four pixels as well (two more 16-byte loads, no taps) and store the
// four bytes as one dword.  No tap leaves the images whatever the maps hold (fe_rectify_pixel clamps every
// coordinate), and validity only tests coordinates.
struct StereoRectifyArgs {
    const uint8_t *raw_l, *raw_r;    // w*h*3 each: the pair as uploaded
    const int32_t *qu_l, *qv_l, *qu_r, *qv_r;   // w*h each, 16-byte aligned
    uint8_t *dst_l, *dst_r;          // w*h*3 each: the rectified pair
    uint8_t *valid;                  // w*h: bit 0 V_L, bit 1 V_R
    int w, h;
};

__device__ __forceinline__ uint32_t fe_nearest_inside(int qu, int qv, int w, int h)
{
    int xn, yn;
    return fe_nearest(qu, qv, w, h, &xn, &yn) ? 1u : 0u;
}

__global__ void __launch_bounds__(FE_BLOCK) k_fe_stereo_rectify(const StereoRectifyArgs a)
{
    const bool right = blockIdx.y != 0;
    const uint8_t *src = right ? a.raw_r : a.raw_l;
    const int32_t *qu = right ? a.qu_r : a.qu_l, *qv = right ? a.qv_r : a.qv_l;
    uint8_t *dst = right ? a.dst_r : a.dst_l;
    const int w = a.w, h = a.h, np = w * h;
    const int i0 = 4 * (blockIdx.x * FE_BLOCK + threadIdx.x);
    if (i0 >= np) return;
    if (i0 + 4 <= np) {
        const int4 u4 = *reinterpret_cast<const int4 *>(qu + i0), v4 = *reinterpret_cast<const int4 *>(qv + i0);
        const int us[4] = {u4.x, u4.y, u4.z, u4.w}, vs[4] = {v4.x, v4.y, v4.z, v4.w};
        uint32_t b[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int c[3];
            uint16_t none;
            fe_rectify_pixel(src, nullptr, w, h, us[q], vs[q], c, &none);
            b[3 * q] = (uint32_t)c[0]; b[3 * q + 1] = (uint32_t)c[1]; b[3 * q + 2] = (uint32_t)c[2];
        }
        uint32_t *o = reinterpret_cast<uint32_t *>(dst + 3 * (size_t)i0);   // 12 * (i0 / 4): dword aligned
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        if (!right) {
            const int4 ru = *reinterpret_cast<const int4 *>(a.qu_r + i0), rv = *reinterpret_cast<const int4 *>(a.qv_r + i0);
            const int rus[4] = {ru.x, ru.y, ru.z, ru.w}, rvs[4] = {rv.x, rv.y, rv.z, rv.w};
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                v |= (fe_nearest_inside(us[q], vs[q], w, h) | (fe_nearest_inside(rus[q], rvs[q], w, h) << 1)) << (8 * q);
            *reinterpret_cast<uint32_t *>(a.valid + i0) = v;
        }
    } else {
        for (int i = i0; i < np; ++i) {
            int c[3];
            uint16_t none;
            fe_rectify_pixel(src, nullptr, w, h, qu[i], qv[i], c, &none);
            dst[3 * (size_t)i] = (uint8_t)c[0]; dst[3 * (size_t)i + 1] = (uint8_t)c[1]; dst[3 * (size_t)i + 2] = (uint8_t)c[2];
            if (!right)
                a.valid[i] = (uint8_t)(fe_nearest_inside(qu[i], qv[i], w, h) | (fe_nearest_inside(a.qu_r[i], a.qv_r[i], w, h) << 1));
        }
    }
}

// The first stage of a frame whose context has a depth camera (the registration contract of
// include/cvo_frontend.h, at cvo_fe_depth_camera): a forward warp of the raw depth image into the
// colour camera's frame with a z-buffer, nearest surface wins.  One thread per depth pixel: it lifts
// the two opposite corners of its cell along the rig's rays (cvo_fe_depth_rays' table, interleaved as
// float2 so that a wave reads whole lines), carries them into the colour frame, projects them, and
// posts its depth to every colour pixel whose centre lies inside the projected cell -- at most 8 x 8
// of them -- with an integer atomicMin whose result nobody reads (no-return, relaxed, agent scope:
// integer minima commute, so the plane does not depend on the order of arrival).  Every write is
// bounded here: x in [0, w), y in [0, h).
constexpr uint32_t FE_Z_EMPTY = 0xFFFFFFFFu;   // a z-buffer entry nothing was written to
constexpr int FE_FOOT = 8;                     // the footprint's cap per axis

struct DepthWarpArgs {
    const uint16_t *depth;   // dw * dh
    const float2 *rays;      // (dh + 1) * (dw + 1): (xn, yn) of the cell corners
    uint32_t *z;             // w * h, FE_Z_EMPTY where nothing was seen yet
    int dw, dh, w, h;
    float scale, min_range, max_range;
    float R[9], T[3];
    float cam[5];            // the colour camera: depth scale, fx, fy, cx, cy
};

__device__ __forceinline__ void fe_depth_corner(const DepthWarpArgs &a, float2 ray, float z, float Q[3])
{
    const float X = ray.x * z, Y = ray.y * z;
#pragma unroll
    for (int k = 0; k < 3; ++k) Q[k] = ((a.R[3 * k] * X + a.R[3 * k + 1] * Y) + a.R[3 * k + 2] * z) + a.T[k];
}

__device__ __forceinline__ void fe_depth_span(float pa, float pb, int n, int *lo, int *hi)
{
    const float top = (float)(n + 1);
    const int p0 = (int)ceilf(fminf(fmaxf(fminf(pa, pb), -1.0f), top));
    int p1 = (int)ceilf(fminf(fmaxf(fmaxf(pa, pb), -1.0f), top));
    p1 = min(p1, p0 + FE_FOOT);
    *lo = max(p0, 0);
    *hi = min(p1, n);
}

__global__ void __launch_bounds__(FE_BLOCK) k_fe_depth_warp(const DepthWarpArgs a)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i >= a.dw * a.dh) return;
    const uint16_t d = a.depth[i];
    if (d == 0) return;
    const float z = (float)d / a.scale;
    if ((a.min_range > 0.0f && z < a.min_range) || (a.max_range > 0.0f && z > a.max_range)) return;
    const int v = i / a.dw, u = i - v * a.dw;
    const size_t c = (size_t)v * (a.dw + 1) + u;
    float Qa[3], Qb[3];
    fe_depth_corner(a, a.rays[c], z, Qa);
    fe_depth_corner(a, a.rays[c + a.dw + 2], z, Qb);
    if (!(Qa[2] > 0.0f && Qb[2] > 0.0f)) return;   // (also a ray that is not a number)
    const float ua = a.cam[1] * (Qa[0] / Qa[2]) + a.cam[3], va = a.cam[2] * (Qa[1] / Qa[2]) + a.cam[4];
    const float ub = a.cam[1] * (Qb[0] / Qb[2]) + a.cam[3], vb = a.cam[2] * (Qb[1] / Qb[2]) + a.cam[4];
    if (!(isfinite(ua) && isfinite(va) && isfinite(ub) && isfinite(vb))) return;
    const float qf = rintf((0.5f * (Qa[2] + Qb[2])) * a.cam[0]);
    if (!(qf >= 1.0f && qf <= 65535.0f)) return;
    const uint32_t q = (uint32_t)qf;
    int x0, x1, y0, y1;
    fe_depth_span(ua, ub, a.w, &x0, &x1);
    fe_depth_span(va, vb, a.h, &y0, &y1);
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x)
            (void)__hip_atomic_fetch_min(a.z + ((size_t)y * a.w + x), q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ... and its second half: the z-buffer becomes the uint16 depth plane every later stage reads (0 where
// nothing was written) and is armed again for the next frame in the same pass, so that a frame needs no
// memset of its own.  Four pixels per thread: a 16-byte load, an 8-byte store of depth and a 16-byte
// store of FE_Z_EMPTY; the last, partial group goes pixel by pixel.
__global__ void __launch_bounds__(FE_BLOCK) k_fe_depth_final(uint32_t *z, int np, uint16_t *ddst)
{
    const int i0 = 4 * (blockIdx.x * FE_BLOCK + threadIdx.x);
    if (i0 >= np) return;
    if (i0 + 4 <= np) {
        const uint4 q = *reinterpret_cast<const uint4 *>(z + i0);
        const uint32_t d0 = q.x == FE_Z_EMPTY ? 0u : q.x, d1 = q.y == FE_Z_EMPTY ? 0u : q.y;
        const uint32_t d2 = q.z == FE_Z_EMPTY ? 0u : q.z, d3 = q.w == FE_Z_EMPTY ? 0u : q.w;
        *reinterpret_cast<uint2 *>(ddst + i0) = make_uint2(d0 | (d1 << 16), d2 | (d3 << 16));
        *reinterpret_cast<uint4 *>(z + i0) = make_uint4(FE_Z_EMPTY, FE_Z_EMPTY, FE_Z_EMPTY, FE_Z_EMPTY);
    } else {
        for (int i = i0; i < np; ++i) {
            const uint32_t q = z[i];
            ddst[i] = q == FE_Z_EMPTY ? (uint16_t)0 : (uint16_t)q;
            z[i] = FE_Z_EMPTY;
        }
    }
}

// The last stage in front of level 0 while a gate or a mask is set (the gate contract of
// include/cvo_frontend.h, at cvo_fe_depth_gate): the depth plane U that k_fe_rectify, k_fe_depth_final or
// the upload left becomes the plane every later stage reads, with 0 where a pixel is out of range, on or
// within `grow` of a depth jump, or masked; the reasons go to a plane of flags.
// A workgroup owns a tile of 64 x 16 pixels; a thread owns four consecutive pixels of one tile row, so
// 16 threads cover a row and FE_BLOCK threads the tile, and the depth goes out as one 8-byte store and the
// flags as one dword per thread, as in the sibling kernels.  The tile is wide and flat because the halo
// costs per row and per column alike while only the rows are contiguous in memory: 64 x 16 with the
// largest halo reads 72 x 24 = 1.69 cells per pixel in lines of 144 bytes; 32 x 32 would read 1.56 in
// lines of 80.
//   phase 1: U of the tile and a halo of grow + 1 into LDS, row by row (consecutive lanes, consecutive
//            uint16: a wave reads whole lines).  Every address is tested against the image; a cell outside
//            holds 0 and is told from a hole by its coordinates in phase 2, never by its value.
//   phase 2: J of the tile and a halo of grow into LDS bytes, from the eight neighbours in LDS.
//   phase 3: each thread ORs J over the (2 grow + 1)^2 windows of its four pixels -- the window rows read as
//            dwords and folded into one bit row first, then four shifts -- applies range and mask, writes.
// U is read from memory once per cell of tile + halo; the mask and, under a distorting model, qu / qv
// once per pixel.  LDS: 24 x 72 uint16 + 22 x 72 bytes = 5 KiB per workgroup, no limit on occupancy.  The
// U rows are 36 dwords apart and the J rows 18: a lane's neighbours above and below sit 4 (18) banks to
// the side, not on its own bank, and consecutive lanes walk consecutive banks, two (four) cells to a
// dword.  A group of four that is cut by the right border, or whose first pixel is no multiple of four in
// the plane (a width that is none), goes pixel by pixel.
constexpr int FG_TW = 64, FG_TH = 16;            // the tile; FG_TW / 4 * FG_TH == FE_BLOCK
constexpr int FG_HALO = FE_GATE_MAX_GROW + 1;    // the largest grow + 1
constexpr int FG_UW = FG_TW + 2 * FG_HALO, FG_UH = FG_TH + 2 * FG_HALO;               // 72 x 24 cells of U
constexpr int FG_JW = FG_TW + 2 * (FG_HALO - 1), FG_JH = FG_TH + 2 * (FG_HALO - 1);   // 70 x 22 cells of J
constexpr int FG_JS = 72;                        // ... in rows of this many bytes
static_assert((FG_TW / 4) * FG_TH == FE_BLOCK, "one thread per four pixels of the tile");

struct GateArgs {
    const uint16_t *u;       // w * h: the plane the gate reads
    uint16_t *depth;         // w * h: the plane every later stage reads
    uint8_t *flags;          // w * h: CVO_FE_GATE_*
    const uint8_t *mask;     // w * h on the grid of the image as uploaded, or null: no mask
    const int32_t *qu, *qv;  // the rectification map if the mask goes through it, or null
    int w, h;
    float scale, min_range, max_range, jump_rel;
    int grow, hole_border;
};

__device__ __forceinline__ bool fe_gate_masked(const GateArgs &a, size_t i, int qu, int qv)
{
    if (!a.qu) return a.mask[i] != 0;
    int xn, yn;
    if (!fe_nearest(qu, qv, a.w, a.h, &xn, &yn)) return true;
    return a.mask[(size_t)yn * a.w + xn] != 0;
}

__device__ __forceinline__ uint32_t fe_gate_flags(const GateArgs &a, uint32_t u, bool near, bool masked)
{
    if (u == 0) return 0u;
    const float z = (float)u / a.scale;
    const bool range = (a.min_range > 0.0f && z < a.min_range) || (a.max_range > 0.0f && z > a.max_range);
    return (masked ? (uint32_t)CVO_FE_GATE_MASKED : 0u) | (range ? (uint32_t)CVO_FE_GATE_RANGE : 0u) |
           (near ? (uint32_t)CVO_FE_GATE_JUMP : 0u);
}

// (G is grow, 0..3, a template argument: every loop below has constant bounds and is unrolled, so that a thread's
// loads from memory and from LDS are in flight together instead of one latency after the other)
template <int G>
__global__ void __launch_bounds__(FE_BLOCK) k_fe_depth_gate(const GateArgs a)
{
    __shared__ __align__(8) uint16_t s_u[FG_UH * FG_UW];             // (phase 3 reads a thread's four cells at once)
    __shared__ uint32_t s_jw[FG_JH * FG_JS / 4];                     // bytes, read as dwords in phase 3
    uint8_t *s_j = reinterpret_cast<uint8_t *>(s_jw);
    const int tx0 = blockIdx.x * FG_TW, ty0 = blockIdx.y * FG_TH;
    constexpr int g = G;
    const bool jumps = a.jump_rel > 0.0f || a.hole_border != 0;      // (else J is 0 everywhere)
    // phase 1: LDS cell (r, c) is pixel (tx0 - FG_HALO + c, ty0 - FG_HALO + r); the rows the halo of grow + 1 needs
    {
        constexpr int r0 = FG_HALO - (g + 1), n = (FG_TH + 2 * (g + 1)) * FG_UW;
#pragma unroll
        for (int k = 0; k < (n + FE_BLOCK - 1) / FE_BLOCK; ++k) {
            const int idx = k * FE_BLOCK + (int)threadIdx.x;
            if (idx < n) {
                const int r = r0 + idx / FG_UW, c = idx % FG_UW;
                const int x = tx0 - FG_HALO + c, y = ty0 - FG_HALO + r;
                uint16_t v = 0;
                if (x >= 0 && x < a.w && y >= 0 && y < a.h) v = a.u[(size_t)y * a.w + x];
                s_u[r * FG_UW + c] = v;
            }
        }
    }
    __syncthreads();
    // phase 2: J cell (r, c) is pixel (tx0 - 3 + c, ty0 - 3 + r), i.e. U cell (r + 1, c + 1); the nine cells are
    // read first (all of them lie in the LDS image, whatever the pixel), then judged
    if (jumps) {
        constexpr int r0 = FG_HALO - 1 - g, n = (FG_TH + 2 * g) * FG_JW;
#pragma unroll
        for (int k = 0; k < (n + FE_BLOCK - 1) / FE_BLOCK; ++k) {
            const int idx = k * FE_BLOCK + (int)threadIdx.x;
            if (idx < n) {
                const int r = r0 + idx / FG_JW, c = idx % FG_JW;
                const int x = tx0 - (FG_HALO - 1) + c, y = ty0 - (FG_HALO - 1) + r;
                uint32_t u9[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) u9[q] = s_u[(r + q / 3) * FG_UW + c + q % 3];
                const uint32_t up = u9[4];
                bool mark = false;
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    if (q == 4) continue;
                    const int xq = x + q % 3 - 1, yq = y + q / 3 - 1;
                    const bool inside = xq >= 0 && xq < a.w && yq >= 0 && yq < a.h;
                    const uint32_t uq = u9[q], m = min(up, uq), D = max(up, uq) - m;
                    const bool by = uq == 0 ? a.hole_border != 0 : (a.jump_rel > 0.0f && (float)D > a.jump_rel * (float)m);
                    mark = mark || (inside && by);
                }
                // (a pixel outside the image marks nobody, and neither does one without depth)
                mark = mark && up != 0 && x >= 0 && x < a.w && y >= 0 && y < a.h;
                s_j[r * FG_JS + c] = mark ? 1 : 0;
            }
        }
    }
    __syncthreads();
    // phase 3
    const int ry = threadIdx.x / (FG_TW / 4), cx = 4 * (threadIdx.x % (FG_TW / 4));
    const int x0 = tx0 + cx, y = ty0 + ry;
    if (x0 >= a.w || y >= a.h) return;
    // the window rows of the four pixels ORed as three dwords -- J columns cx .. cx + 11, of which the windows
    // reach cx + 3 - g .. cx + 6 + g -- and their bytes (0 / 1) gathered into bits: bit j of `cols` is column cx + j
    uint32_t cols = 0;
    if (jumps) {
        uint32_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
        for (int dy = -g; dy <= g; ++dy) {
            const uint32_t *row = s_jw + ((ry + FG_HALO - 1 + dy) * FG_JS + cx) / 4;
            c0 |= row[0]; c1 |= row[1];
            if (g >= 2) c2 |= row[2];
        }
        auto bits = [](uint32_t v) { return (v & 1u) | ((v >> 7) & 2u) | ((v >> 14) & 4u) | ((v >> 21) & 8u); };
        cols = (bits(c0) | (bits(c1) << 4) | (bits(c2) << 8)) >> (FG_HALO - 1 - g);   // bit j: column cx + 3 - g + j
    }
    const uint32_t win = (1u << (2 * g + 1)) - 1u;
    const uint2 own2 = *reinterpret_cast<const uint2 *>(s_u + (ry + FG_HALO) * FG_UW + cx + FG_HALO);   // (8-byte aligned)
    const uint32_t own[4] = {own2.x & 0xFFFFu, own2.x >> 16, own2.y & 0xFFFFu, own2.y >> 16};
    const size_t i0 = (size_t)y * a.w + x0;
    if (x0 + 4 <= a.w && (i0 & 3) == 0) {
        bool masked[4] = {false, false, false, false};
        if (a.mask) {
            if (a.qu) {
                const int4 u4 = *reinterpret_cast<const int4 *>(a.qu + i0), v4 = *reinterpret_cast<const int4 *>(a.qv + i0);
                masked[0] = fe_gate_masked(a, i0, u4.x, v4.x); masked[1] = fe_gate_masked(a, i0 + 1, u4.y, v4.y);
                masked[2] = fe_gate_masked(a, i0 + 2, u4.z, v4.z); masked[3] = fe_gate_masked(a, i0 + 3, u4.w, v4.w);
            } else {
                const uint32_t m4 = *reinterpret_cast<const uint32_t *>(a.mask + i0);
#pragma unroll
                for (int k = 0; k < 4; ++k) masked[k] = ((m4 >> (8 * k)) & 255u) != 0;
            }
        }
        uint32_t d[4], f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t u = own[k];
            f[k] = fe_gate_flags(a, u, ((cols >> k) & win) != 0, masked[k]);
            d[k] = f[k] ? 0u : u;
        }
        *reinterpret_cast<uint2 *>(a.depth + i0) = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
        *reinterpret_cast<uint32_t *>(a.flags + i0) = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
    } else {
        const int n = min(4, a.w - x0);
        for (int k = 0; k < n; ++k) {
            const size_t i = i0 + k;
            const uint32_t u = own[k];
            const bool masked = a.mask && fe_gate_masked(a, i, a.qu ? a.qu[i] : 0, a.qu ? a.qv[i] : 0);
            const uint32_t f = fe_gate_flags(a, u, ((cols >> k) & win) != 0, masked);
            a.depth[i] = f ? (uint16_t)0 : (uint16_t)u;
            a.flags[i] = (uint8_t)f;
        }
    }
}

// Level 0 in one pass.  load_image: cv::cvtColor RGB2GRAY and RGB2HSV on 8-bit data,
// channel 0 taken as R (ref src/pcd_generator.cpp:389-390), OpenCV's fixed-point
// definitions; the grey image as float is level 0 of the pyramid (ref :53-61); its
// central differences on the flattened image for idx in [w, w*(h-1)) (ref :95-113; the
// rest is zero here).  The four neighbours' grey values are recomputed from the colour
// image instead of waiting for another launch.
__global__ void __launch_bounds__(FE_BLOCK) k_fe_level0(const uint8_t *img, int w, int h, const int *sdiv,
                                                        const int *hdiv, uint8_t *gray, uint32_t *hsv, float *I0,
                                                        float *ag, float *dx_out, float *dy_out)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    const int np = w * h;
    if (i >= np) return;
    auto grey = [&](int j) { return fe_grey(img[3 * j], img[3 * j + 1], img[3 * j + 2]); };
    const int r = img[3 * i], g = img[3 * i + 1], b = img[3 * i + 2];
    const int gr = fe_grey(r, g, b);
    gray[i] = (uint8_t)gr;
    I0[i] = (float)gr;
    int v = max(b, max(g, r)), vmin = min(b, min(g, r));
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int hh = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    hh = (hh * hdiv[diff] + (1 << 11)) >> 12;
    hh += hh < 0 ? 180 : 0;
    hh = min(max(hh, 0), 255);
    hsv[i] = (uint32_t)hh | ((uint32_t)s << 8) | ((uint32_t)v << 16);
    float dx = 0.0f, dy = 0.0f, a = 0.0f;
    if (i >= w && i < w * (h - 1)) {
        dx = 0.5f * ((float)grey(i + 1) - (float)grey(i - 1));
        dy = 0.5f * ((float)grey(i + w) - (float)grey(i - w));
        a = dx * dx + dy * dy;
    }
    ag[i] = a;
    dx_out[i] = dx;
    dy_out[i] = dy;
}

// Level l > 0 in one pass: the 2x2 mean of level l-1 (ref src/pcd_generator.cpp:79-93)
// and its squared gradient magnitude (ref :95-113); the neighbours' means are recomputed.
__global__ void __launch_bounds__(FE_BLOCK) k_fe_level(const float *prev, int pw, float *cur, int wl, int hl, float *ag)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i >= wl * hl) return;
    auto mean = [&](int j) {
        const int y = j / wl, x = j - y * wl;
        const float *p = prev + 2 * x + 2 * y * pw;
        return 0.25f * (((p[0] + p[1]) + p[pw]) + p[pw + 1]);
    };
    cur[i] = mean(i);
    float a = 0.0f;
    if (i >= wl && i < wl * (hl - 1)) {
        float dx = 0.5f * (mean(i + 1) - mean(i - 1));
        float dy = 0.5f * (mean(i + wl) - mean(i - wl));
        if (!isfinite(dx)) dx = 0.0f;
        if (!isfinite(dy)) dy = 0.0f;
        a = dx * dx + dy * dy;
    }
    ag[i] = a;
}

// PixelSelector::makeHists, first half (ref thirdparty/PixelSelector2.cpp:70-104): one
// block per 32x32 cell; histogram of the integer gradient magnitudes, its median + 7
__global__ void __launch_bounds__(FE_BLOCK) k_fe_hist(const float *ag0, int w, int h, int w32, float *ths)
{
    __shared__ int hist[50];
    const int cx = blockIdx.x % w32, cy = blockIdx.x / w32;
    if (threadIdx.x < 50) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < 1024; q += FE_BLOCK) {
        const int it = (q & 31) + 32 * cx, jt = (q >> 5) + 32 * cy;
        if (it > w - 2 || jt > h - 2 || it < 1 || jt < 1) continue;
        int g = (int)sqrtf(ag0[it + jt * w]);
        if (g > 48) g = 48;
        atomicAdd(&hist[g + 1], 1);
        atomicAdd(&hist[0], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // computeHistQuantil(hist, 0.5) (ref :58-67; bins past the 50 cleared ones are empty)
        int th = (int)(hist[0] * 0.5f + 0.5f);
        int res = 90;
        for (int i = 0; i < 90; ++i) {
            th -= (i + 1 < 50) ? hist[i + 1] : 0;
            if (th < 0) { res = i; break; }
        }
        ths[blockIdx.x] = (float)(res + 7);
    }
}

// makeHists, second half (ref thirdparty/PixelSelector2.cpp:106-131): squared 3x3 mean
__global__ void __launch_bounds__(FE_BLOCK) k_fe_smooth(const float *ths, int w32, int h32, float *out)
{
    const int c = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (c >= w32 * h32) return;
    const int x = c % w32, y = c / w32;
    float sum = 0, num = 0;
    if (x > 0) {
        if (y > 0) { num++; sum += ths[x - 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x - 1 + (y + 1) * w32]; }
        num++; sum += ths[x - 1 + y * w32];
    }
    if (x < w32 - 1) {
        if (y > 0) { num++; sum += ths[x + 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x + 1 + (y + 1) * w32]; }
        num++; sum += ths[x + 1 + y * w32];
    }
    if (y > 0) { num++; sum += ths[x + (y - 1) * w32]; }
    if (y < h32 - 1) { num++; sum += ths[x + (y + 1) * w32]; }
    num++; sum += ths[x + y * w32];
    out[c] = (sum / num) * (sum / num);
}

struct SelectArgs {
    const float *ag0, *ag1, *ag2, *ths;
    float *map;
    FeCtrl *ctrl;
    int *blk_cnt;   // [block][3]: pixels chosen at level 0 / 1 / 2 by that block
    int w, h, w32, ncell, pass;
    const uint16_t *depth;   // the final depth plane: read by the DEPTH instance only (the selection contract)
};

// PixelSelector::select (ref thirdparty/PixelSelector2.cpp:240-437), direction
// distribution off (PixelSelector2.h:31).  The reference walks every block B4 of
// 4pot x 4pot pixels through its four 2pot blocks B3 and their four pot blocks B2 with
// three running maxima and two sticky "-2" marks; with the random directions unused
// that walk computes, for the pixels inside the margin (ref :313):
//   * every B2 holding a pixel with ag0 > th0 keeps the first largest ag0 among them
//     (map 1);
//   * every B3 WITHOUT such a pixel that holds a pixel with ag1 > th1 keeps the first
//     largest ag1 among those (map 2) -- the first level-0 hit of a B3 sets
//     bestIdx3 = -2 for good (ref :325,:328,:366);
//   * a B4 without either kind that holds a pixel with ag2 > th2 keeps the first largest
//     ag2 (map 4) -- any level-0 or level-1 improvement sets bestIdx4 = -2 (ref :325,:338);
// "first" in the reference's visiting order (B3s, their B2s, rows, columns).  One wave
// takes one B4: its lanes test the pixels (coalesced rows) and post (value, order) keys
// to 21 LDS slots with 64-bit atomic max; 21 lanes then write the picks.
// DEPTH (CVO_FE_SELECT_DEPTH, the selection contract): a pixel without depth leaves where a pixel
// outside the margin leaves -- its depth is loaded beside its ag0 in the same sweep, and the test
// is one more term of the margin's `continue`; the instance without it is the code it was.
template <bool DEPTH>
__global__ void __launch_bounds__(FE_BLOCK) k_fe_select(const SelectArgs a)
{
    if (a.pass == 1 && !a.ctrl->redo) return;
    __shared__ unsigned long long s_slot[FE_BLOCK / 64][24];
    __shared__ int s_n[FE_BLOCK / 64][3];
    const int pot = a.ctrl->pot[a.pass];
    const int w = a.w, h = a.h, side = 4 * pot;
    const int cw = (w + side - 1) / side, ch = (h + side - 1) / side;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int cell = blockIdx.x * (FE_BLOCK / 64) + wid;
    const bool live = cell < cw * ch;
    unsigned long long *slot = s_slot[wid];
    if (lane < 24) slot[lane] = 0ull;
    __syncthreads();
    const int y4 = live ? (cell / cw) * side : 0, x4 = live ? (cell % cw) * side : 0;
    if (live) {
        const int w1 = w / 2, w2 = w / 4;
        const float dw1 = 0.75f, dw2 = dw1 * dw1, thFactor = 1.0f;
        for (int q = lane; q < side * side; q += 64) {
            const int ly = q / side, lx = q - ly * side;
            const int xf = x4 + lx, yf = y4 + ly;
            if (xf >= w || yf >= h) continue;
            const int idx = xf + w * yf;
            a.map[idx] = 0.0f;   // (ref :276)
            if (DEPTH) {
                if (xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4 || a.depth[idx] == 0) continue;
            } else if (xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4) continue;
            const int bx3 = lx / (2 * pot), by3 = ly / (2 * pot);
            const int rx = lx - bx3 * 2 * pot, ry = ly - by3 * 2 * pot;
            const int bx2 = rx / pot, by2 = ry / pot;
            const int x1 = rx - bx2 * pot, y1 = ry - by2 * pot;
            const int b3 = by3 * 2 + bx3, b2 = b3 * 4 + by2 * 2 + bx2;
            const unsigned order = ~(unsigned)((b2 * pot + y1) * pot + x1);   // earlier pixel = larger key
            const int cellth = min((xf >> 5) + (yf >> 5) * a.w32, a.ncell - 1);
            const float th0 = a.ths[cellth];
            const float th1 = th0 * dw1;
            const float th2 = th1 * dw2;
            const float a0 = a.ag0[idx];
            const float a1 = a.ag1[(int)(xf * 0.5f + 0.25f) + (int)(yf * 0.5f + 0.25f) * w1];
            const float a2 = a.ag2[(int)(xf * 0.25f + 0.125f) + (int)(yf * 0.25f + 0.125f) * w2];
            if (a0 > th0 * thFactor)
                atomicMax(&slot[b2], ((unsigned long long)__float_as_uint(a0) << 32) | order);
            if (a1 > th1 * thFactor)
                atomicMax(&slot[16 + b3], ((unsigned long long)__float_as_uint(a1) << 32) | order);
            if (a2 > th2 * thFactor)
                atomicMax(&slot[20], ((unsigned long long)__float_as_uint(a2) << 32) | order);
        }
    }
    __syncthreads();
    int pick = 0;   // 1 / 2 / 4: this lane writes a pick of that level
    if (live && lane < 21) {
        unsigned long long v = 0ull;
        if (lane < 16) {
            v = slot[lane];
            pick = v ? 1 : 0;
        } else if (lane < 20) {
            const int b3 = lane - 16;
            const bool lvl0 = (slot[4 * b3] | slot[4 * b3 + 1] | slot[4 * b3 + 2] | slot[4 * b3 + 3]) != 0ull;
            v = slot[lane];
            pick = (!lvl0 && v) ? 2 : 0;
        } else {
            unsigned long long any = 0ull;
            for (int q = 0; q < 20; ++q) any |= slot[q];
            v = slot[20];
            pick = (!any && v) ? 4 : 0;
        }
        if (pick) {
            const int r = (int)~(unsigned)v;   // visiting order -> pixel
            const int x1 = r % pot, y1 = (r / pot) % pot, b2 = r / (pot * pot);
            const int b3 = b2 >> 2, bx3 = b3 & 1, by3 = b3 >> 1, bx2 = b2 & 1, by2 = (b2 >> 1) & 1;
            const int xf = x4 + bx3 * 2 * pot + bx2 * pot + x1, yf = y4 + by3 * 2 * pot + by2 * pot + y1;
            a.map[xf + w * yf] = (float)pick;
        }
    }
    const int n2 = __popcll(__ballot(pick == 1)), n3 = __popcll(__ballot(pick == 2)), n4 = __popcll(__ballot(pick == 4));
    if (lane == 0) { s_n[wid][0] = n2; s_n[wid][1] = n3; s_n[wid][2] = n4; }
    __syncthreads();
    if (threadIdx.x < 3)
        a.blk_cnt[3 * blockIdx.x + threadIdx.x] =
            (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
}

// PixelSelector::makeMaps, the decisions (ref thirdparty/PixelSelector2.cpp:137-207):
// stage 0 after the first selection pass (re-select with another potential?), stage 1
// after the second (sub-sample?).  One block: it first adds up the per-block counts of
// the selection pass that just ran (`nb` blocks).
__global__ void __launch_bounds__(FE_BLOCK) k_fe_decide(FeCtrl *c, const int *blk_cnt, int nb, int stage,
                                                        float num_want_f)
{
    __shared__ int s_r[FE_BLOCK / 64][3];
    __shared__ int s_skip;
    if (threadIdx.x == 0) s_skip = (stage == 1 && !c->redo) ? 1 : 0;
    __syncthreads();
    if (!s_skip) {   // (pass 1 did not run: its counts are stale)
        int v[3] = {0, 0, 0};
        for (int q = threadIdx.x; q < nb; q += FE_BLOCK)
            for (int k = 0; k < 3; ++k) v[k] += blk_cnt[3 * q + k];
        for (int k = 0; k < 3; ++k) v[k] = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 3; ++k) s_r[threadIdx.x >> 6][k] = v[k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 3; ++k) c->n[stage][k] = (s_r[0][k] + s_r[1][k]) + (s_r[2][k] + s_r[3][k]);
    }
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        const int pot = c->pot[0];
        const float numHave = (float)(c->n[0][0] + c->n[0][1] + c->n[0][2]);
        const float quotia = num_want_f / numHave;
        const float K = numHave * (float)(pot + 1) * (float)(pot + 1);
        int ideal = (int)(sqrtf(K / num_want_f) - 1);
        if (ideal < 1) ideal = 1;
        int redo = 0;
        if (quotia > 1.25f && pot > 1) {
            if (ideal >= pot) ideal = pot - 1;
            redo = 1;
        } else if (quotia < 0.25f) {
            if (ideal <= pot) ideal = pot + 1;
            redo = 1;
        }
        c->redo = redo;
        c->pot[1] = ideal;
    } else {
        const int p = c->redo ? 1 : 0;
        const int have = c->n[p][0] + c->n[p][1] + c->n[p][2];
        const float quotia = num_want_f / (float)have;
        c->num_have = have;
        c->do_sub = ((double)quotia < 0.95) ? 1 : 0;
        c->char_th = c->do_sub ? (int)(unsigned char)(255 * quotia) : 255;
    }
}

// Ordered passes over the map.  Block b owns pixels [b*FE_CHUNK, (b+1)*FE_CHUNK),
// thread t of it the 4 consecutive ones from 4t: a count kernel, then a kernel in
// which every block sums the counts of the blocks before it.
// MODE 0: map != 0 (the sub-sampling's running index, ref PixelSelector2.cpp:213-226)
// MODE 1: map != 0 and depth != 0 (the cloud's point index, ref pcd_generator.cpp:304-321)
template <int MODE>
__device__ __forceinline__ int fe_flags(const float *map, const uint16_t *depth, int np, int i0)
{
    int f = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + q;
        if (i < np && map[i] != 0.0f && (MODE == 0 || depth[i] != 0)) f |= 1 << q;
    }
    return f;
}

template <int MODE>
__global__ void __launch_bounds__(FE_BLOCK) k_fe_count(const float *map, const uint16_t *depth, int np,
                                                       const FeCtrl *c, int *cnt)
{
    if (MODE == 0 && !c->do_sub) return;
    __shared__ int s_w[2][FE_BLOCK / 64];
    const int i0 = blockIdx.x * FE_CHUNK + 4 * threadIdx.x;
    const int f = fe_flags<MODE>(map, depth, np, i0);
    const int v = wave_sum(__popc(f));
    // MODE 1 also counts the pixels in the map, with or without depth (cnt[gridDim.x + b]):
    // their total is the selector's result (num_selected)
    const int u = MODE == 1 ? wave_sum(__popc(fe_flags<0>(map, depth, np, i0))) : 0;
    if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = v; s_w[1][threadIdx.x >> 6] = u; }
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = (s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]);
    if (MODE == 1 && threadIdx.x == 1) cnt[gridDim.x + blockIdx.x] = (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]);
}

// makeMaps, sub-sampling (ref thirdparty/PixelSelector2.cpp:209-226): the rn-th chosen
// pixel in scan order is dropped if the rn-th random byte exceeds the threshold
__global__ void __launch_bounds__(FE_BLOCK) k_fe_subsample(float *map, int np, const uint8_t *pattern,
                                                           const int *cnt, FeCtrl *c)
{
    if (!c->do_sub) return;
    const int i0 = blockIdx.x * FE_CHUNK + 4 * threadIdx.x;
    const int f = fe_flags<0>(map, nullptr, np, i0);
    int total;
    int rn = block_base(cnt, blockIdx.x) + block_excl_scan(__popc(f), &total);
    const int th = c->char_th;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (f & (1 << q)) {
            if ((int)pattern[rn] > th) map[i0 + q] = 0.0f;
            rn++;
        }
    // (num_selected = what is left: counted by the next pass, k_fe_count<1>)
}

struct EmitArgs {
    const float *map;
    const uint16_t *depth;
    const uint8_t *img;
    const uint32_t *hsv;
    const float *dx0, *dy0;
    const int *cnt;
    FeCtrl *ctrl;
    float *pos, *feat;
    int np, w, cap, feature_type, nblocks;
    float cam[5];
};

// get_points_from_pixels + get_features (ref src/pcd_generator.cpp:297-321, 336-380)
__global__ void __launch_bounds__(FE_BLOCK) k_fe_emit(const EmitArgs a)
{
    const int i0 = blockIdx.x * FE_CHUNK + 4 * threadIdx.x;
    const int f = fe_flags<1>(a.map, a.depth, a.np, i0);
    int total;
    int idx = block_base(a.cnt, blockIdx.x) + block_excl_scan(__popc(f), &total);
    if (blockIdx.x == a.nblocks - 1 && threadIdx.x == FE_BLOCK - 1) a.ctrl->num_points = idx + __popc(f);
    if (blockIdx.x == 0) {   // (uniform per block) the size of the map
        const int in_map = block_base(a.cnt + a.nblocks, a.nblocks);
        if (threadIdx.x == 0) a.ctrl->in_map = in_map;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (f & (1 << q)) {
            const int p = i0 + q;
            if (idx < a.cap) {
                const int y = p / a.w, x = p - y * a.w;
                const float z = (float)a.depth[p] / a.cam[0];
                a.pos[3 * idx + 2] = z;
                a.pos[3 * idx + 0] = ((float)x - a.cam[3]) * z / a.cam[1];
                a.pos[3 * idx + 1] = ((float)y - a.cam[4]) * z / a.cam[2];
                float *ft = a.feat + 5 * (size_t)idx;
                if (a.feature_type == 0) {
                    const uint32_t hv = a.hsv[p];
                    ft[0] = (float)((double)(hv & 255u) / 180.0);
                    ft[1] = (float)((double)((hv >> 8) & 255u) / 255.0);
                    ft[2] = (float)((double)((hv >> 16) & 255u) / 255.0);
                    ft[3] = (float)((double)a.dx0[p] / 255.0 * 2);
                    ft[4] = (float)((double)a.dy0[p] / 255.0 * 2);
                } else {
                    ft[0] = (float)a.img[3 * p];
                    ft[1] = (float)a.img[3 * p + 1];
                    ft[2] = (float)a.img[3 * p + 2];
                    ft[3] = a.dx0[p];
                    ft[4] = a.dy0[p];
                }
            }
            idx++;
        }
}

// ---- the Canny top-up (ref src/pcd_generator.cpp:143-175), only when ctrl->canny ----

__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// cv::blur 3x3, 8-bit (BORDER_REFLECT_101, rounded to nearest)
__global__ void __launch_bounds__(FE_BLOCK) k_fe_blur(const uint8_t *src, int w, int h, uint8_t *dst)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    int s = 0;
    for (int j = -1; j <= 1; ++j)
        for (int k = -1; k <= 1; ++k) s += src[reflect101(y + j, h) * w + reflect101(x + k, w)];
    dst[i] = (uint8_t)__double2int_rn((double)s * (1.0 / 9.0));
}

// cv::Canny, gradients: 3x3 Sobel with replicated borders, L1 magnitude
__global__ void __launch_bounds__(FE_BLOCK) k_fe_sobel(const uint8_t *src, int w, int h, short2 *g, int *mag)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    auto px = [&](int xx, int yy) { return (int)src[min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1)]; };
    const int dx = (px(x + 1, y - 1) + 2 * px(x + 1, y) + px(x + 1, y + 1)) -
                   (px(x - 1, y - 1) + 2 * px(x - 1, y) + px(x - 1, y + 1));
    const int dy = (px(x - 1, y + 1) + 2 * px(x, y + 1) + px(x + 1, y + 1)) -
                   (px(x - 1, y - 1) + 2 * px(x, y - 1) + px(x + 1, y - 1));
    g[i] = make_short2((short)dx, (short)dy);
    mag[i] = abs(dx) + abs(dy);
}

// cv::Canny, non-maximum suppression: 0 candidate, 1 not an edge, 2 edge (above `high`)
__global__ void __launch_bounds__(FE_BLOCK) k_fe_nms(const short2 *g, const int *mag, int w, int h, int low, int high,
                                                     uint8_t *st)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    auto mg = [&](int xx, int yy) { return (xx < 0 || xx >= w || yy < 0 || yy >= h) ? 0 : mag[yy * w + xx]; };
    const int m = mag[i];
    bool is_max = false;
    if (m > low) {
        const int TG22 = 13573;   // (int)(0.41421356... * (1 << 15) + 0.5)
        const int xs = g[i].x, ys = g[i].y;
        const int ax = abs(xs), ay = abs(ys) << 15;
        const int tg22x = ax * TG22;
        if (ay < tg22x) {
            is_max = m > mg(x - 1, y) && m >= mg(x + 1, y);
        } else {
            const int tg67x = tg22x + (ax << 16);
            if (ay > tg67x) {
                is_max = m > mg(x, y - 1) && m >= mg(x, y + 1);
            } else {
                const int s = (xs ^ ys) < 0 ? -1 : 1;
                is_max = m > mg(x - s, y - 1) && m > mg(x + s, y + 1);
            }
        }
    }
    st[i] = !is_max ? 1 : (m > high ? 2 : 0);
}

// cv::Canny, hysteresis: one sweep -- a 32x32 tile (with a one-pixel halo) is brought to
// its local fixed point in LDS; the host repeats sweeps until none changed anything
__global__ void __launch_bounds__(FE_BLOCK) k_fe_hyst(uint8_t *st, int w, int h, int tiles_x, FeCtrl *c)
{
    __shared__ uint8_t t[34][36];
    __shared__ int s_changed, s_any;
    const int tx = (blockIdx.x % tiles_x) * 32, ty = (blockIdx.x / tiles_x) * 32;
    for (int q = threadIdx.x; q < 34 * 34; q += FE_BLOCK) {
        const int lx = q % 34, ly = q / 34, gx = tx + lx - 1, gy = ty + ly - 1;
        t[ly][lx] = (gx < 0 || gx >= w || gy < 0 || gy >= h) ? 1 : st[gy * w + gx];
    }
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    for (;;) {
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (int q = threadIdx.x; q < 1024; q += FE_BLOCK) {
            const int lx = (q & 31) + 1, ly = (q >> 5) + 1;
            if (t[ly][lx] != 0) continue;
            bool strong = false;
            for (int j = -1; j <= 1; ++j)
                for (int k = -1; k <= 1; ++k) strong = strong || t[ly + j][lx + k] == 2;
            if (strong) { t[ly][lx] = 2; s_changed = 1; }
        }
        __syncthreads();
        const int ch = s_changed;
        __syncthreads();
        if (!ch) break;
        if (threadIdx.x == 0) s_any = 1;
    }
    __syncthreads();
    if (s_any) {
        for (int q = threadIdx.x; q < 1024; q += FE_BLOCK) {
            const int lx = (q & 31) + 1, ly = (q >> 5) + 1, gx = tx + lx - 1, gy = ty + ly - 1;
            if (gx < w && gy < h && t[ly][lx] == 2) st[gy * w + gx] = 2;
        }
        if (threadIdx.x == 0) c->changed = 1;
    }
}

// select_point, the top-up itself (ref src/pcd_generator.cpp:153-174): one thread per
// 8x8 block, first free edge pixel in row order (DEPTH, the selection contract: the first
// one that also has a depth)
template <bool DEPTH>
__global__ void __launch_bounds__(FE_BLOCK) k_fe_topup(const uint8_t *st, int w, int h, float *map, const uint16_t *depth)
{
    const int bw = (w + 7) / 8, bh = (h + 7) / 8;
    const int b = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (b >= bw * bh) return;
    const int x = (b % bw) * 8, y = (b / bw) * 8;
    for (int j = 0; j < 8; ++j)
        for (int i = 0; i < 8; ++i) {
            if (x + i >= w || y + j >= h) continue;
            const int p = (y + j) * w + x + i;
            if (st[p] == 2 && map[p] == 0.0f && (!DEPTH || depth[p] != 0)) { map[p] = 1.0f; return; }
        }
}

__global__ void __launch_bounds__(FE_BLOCK) k_fe_edges(const uint8_t *st, int np, uint8_t *edges)
{
    const int i = blockIdx.x * FE_BLOCK + threadIdx.x;
    if (i < np) edges[i] = st[i] == 2 ? 255 : 0;
}

// ---- the C library's rand() after srand(seed): additive feedback generator of degree
// 31, separation 3 (glibc random_r.c TYPE_3), restated so that no global state is touched
struct LibcRand {
    int32_t st[34];
    int f, r;
    explicit LibcRand(unsigned seed)
    {
        int32_t word = seed ? (int32_t)seed : 1;
        st[0] = word;
        for (int i = 1; i < 31; ++i) {
            const long hi = word / 127773, lo = word % 127773;
            word = (int32_t)(16807 * lo - 2836 * hi);
            if (word < 0) word += 2147483647;
            st[i] = word;
        }
        f = 3; r = 0;
        for (int i = 0; i < 310; ++i) next();
    }
    int next()
    {
        const uint32_t v = (uint32_t)st[f] + (uint32_t)st[r];
        st[f] = (int32_t)v;
        f = f + 1 == 31 ? 0 : f + 1;
        r = r + 1 == 31 ? 0 : r + 1;
        return (int)(v >> 1);
    }
};

const float kCameras[6][5] = {{1000.0f, 616.368f, 616.745f, 319.935f, 243.639f},   // ref pcd_generator.cpp:243-249
                              {5000.0f, 517.3f, 516.5f, 318.6f, 255.3f},            // fr1 :250-256
                              {5000.0f, 520.9f, 521.0f, 325.1f, 249.7f},            // fr2 :257-263
                              {5000.0f, 535.4f, 539.2f, 320.1f, 247.6f},            // fr3 :264-270
                              {2000.0f, 718.856f, 718.856f, 607.1928f, 185.2157f},  // kitti 15 :271-277
                              {2000.0f, 707.0912f, 707.0912f, 601.8873f, 183.1104f}};   // kitti 05 :279-285

inline int blocks(int n) { return (n + FE_BLOCK - 1) / FE_BLOCK; }

// The projection of a staged scan (a header whose first word is the number of points, then `capacity` records) into
// `z`, for a frame and for cvo_fe_project_points alike: the arguments from the scan source and the camera, and with a
// sweep (the sweep contract: another instance of the same kernel; the twist is in the scan's header) its words and
// the two optional outputs.
void enqueue_lidar_project(const cvo_fe_lidar &l, const float cam[5], const uint8_t *scan, int capacity, uint32_t *z, int w,
                           int h, const cvo_fe_lidar_sweep *sw, float *phase, float *moved, hipStream_t s)
{
    FeLidarProjectArgs a{};
    a.count = (const int32_t *)scan; a.points = (const float *)(scan + FE_LIDAR_HEADER);
    a.z = z; a.capacity = capacity; a.w = w; a.h = h; a.splat = l.splat;
    a.min_range = l.min_range; a.max_range = l.max_range;
    for (int q = 0; q < 9; ++q) a.R[q] = l.R[q];
    for (int q = 0; q < 3; ++q) a.T[q] = l.T[q];
    for (int q = 0; q < 5; ++q) a.cam[q] = cam[q];
    if (!sw) {
        fe_lidar_project_enqueue(a, s);
        return;
    }
    FeLidarSweepArgs sa{};
    sa.base = a;
    sa.time_origin = sw->time_origin; sa.time_scale = sw->time_scale; sa.phase0 = sw->phase0;
    sa.direction = (float)sw->direction; sa.s_ref = sw->s_ref;
    sa.phase = phase; sa.moved = moved;
    fe_lidar_project_sweep_enqueue(sw->mode, sa, s);
}

// the points of the cloud that follow the control block to the host before their number is known: enough for
// any normal frame (none when the consumer takes the cloud from device memory: cvo_fe_set_device_output)
inline int optimistic_copy(const cvo_fe_ctx *ctx)
{
    return ctx->device_output ? 0 : std::min(ctx->cap, std::max(4096, 2 * ctx->num_want));
}

// the `scale` of the depth-format contract: of whatever reads the uploaded depth image first
inline float depth_format_scale(const cvo_fe_ctx *ctx, int dataset_seq)
{
    if (ctx->has_rig) return ctx->rig.depth_scale;
    float cam[5];
    camera_in_force(ctx, dataset_seq, cam);
    return cam[0];
}

// the depth-format contract on the float image at `src`: in front of everything else that reads the depth image
inline void enqueue_depth_convert(const cvo_fe_ctx *ctx, const void *src, size_t pitch, int dataset_seq)
{
    FeDepthConvertArgs a{};
    a.src = src; a.src_pitch = pitch; a.dst = depth_input(ctx);
    a.w = ctx->dw; a.h = ctx->dh; a.format = ctx->depthfmt; a.unit = ctx->depth_unit;
    a.scale = depth_format_scale(ctx, dataset_seq);
    fe_depth_convert_enqueue(a, ctx->stream);
}

// the Canny path of a frame whose selection came out short (host loop: rare)
int run_canny(cvo_fe_ctx *ctx)
{
    const int w = ctx->d.w, h = ctx->d.h, np = ctx->np;
    hipStream_t s = ctx->stream;
    uint8_t *st8 = ctx->st8.get();
    hipLaunchKernelGGL(k_fe_blur, dim3(blocks(np)), dim3(FE_BLOCK), 0, s, ctx->gray.get(), w, h, ctx->tmp8.get());
    hipLaunchKernelGGL(k_fe_sobel, dim3(blocks(np)), dim3(FE_BLOCK), 0, s, ctx->tmp8.get(), w, h, ctx->grad.get(),
                       ctx->mag.get());
    hipLaunchKernelGGL(k_fe_nms, dim3(blocks(np)), dim3(FE_BLOCK), 0, s, ctx->grad.get(), ctx->mag.get(), w, h, 0, 25, st8);
    const int tiles_x = (w + 31) / 32, tiles_y = (h + 31) / 32;
    for (int sweep = 0; sweep < w + h; ++sweep) {
        FE_HIP(hipMemsetAsync(&ctx->ctrl->changed, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_fe_hyst, dim3(tiles_x * tiles_y), dim3(FE_BLOCK), 0, s, st8, w, h, tiles_x, ctx->ctrl.get());
        FE_HIP(hipMemcpyAsync(ctx->h_ctrl.get(), ctx->ctrl.get(), sizeof(FeCtrl), hipMemcpyDeviceToHost, s));
        FE_HIP(hipStreamSynchronize(s));
        if (!ctx->h_ctrl->changed) break;
    }
    hipLaunchKernelGGL(k_fe_edges, dim3(blocks(np)), dim3(FE_BLOCK), 0, s, st8, np, ctx->edges.get());
    const dim3 topup_grid(blocks(((w + 7) / 8) * ((h + 7) / 8)));
    if (ctx->select_mode == CVO_FE_SELECT_DEPTH)
        hipLaunchKernelGGL(k_fe_topup<true>, topup_grid, dim3(FE_BLOCK), 0, s, st8, w, h, ctx->map.get(), ctx->depth.get());
    else
        hipLaunchKernelGGL(k_fe_topup<false>, topup_grid, dim3(FE_BLOCK), 0, s, st8, w, h, ctx->map.get(),
                           (const uint16_t *)nullptr);
    FE_HIP(hipGetLastError());
    return CVO_HIP_OK;
}

int run_emit(cvo_fe_ctx *ctx, int dataset_seq, int feature_type)
{
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_fe_count<1>, dim3(ctx->nchunks), dim3(FE_BLOCK), 0, s, ctx->map.get(), ctx->depth.get(), ctx->np,
                       ctx->ctrl.get(), ctx->cnt.get());
    EmitArgs e{};
    e.map = ctx->map.get(); e.depth = ctx->depth.get(); e.img = ctx->img.get(); e.hsv = ctx->hsv.get();
    e.dx0 = ctx->dx0.get(); e.dy0 = ctx->dy0.get();
    e.cnt = ctx->cnt.get(); e.ctrl = ctx->ctrl.get(); e.pos = ctx->pos.get(); e.feat = ctx->feat.get();
    e.np = ctx->np; e.w = ctx->d.w; e.cap = ctx->cap; e.feature_type = feature_type; e.nblocks = ctx->nchunks;
    camera_in_force(ctx, dataset_seq, e.cam);
    hipLaunchKernelGGL(k_fe_emit, dim3(ctx->nchunks), dim3(FE_BLOCK), 0, s, e);
    FE_HIP(hipMemcpyAsync(ctx->h_ctrl.get(), ctx->ctrl.get(), sizeof(FeCtrl), hipMemcpyDeviceToHost, s));
    // the cloud follows optimistically (its size is not known yet)
    ctx->copied = optimistic_copy(ctx);
    if (!ctx->copied) return CVO_HIP_OK;
    FE_HIP(hipMemcpyAsync(ctx->h_pos.get(), ctx->pos.get(), (size_t)ctx->copied * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    FE_HIP(hipMemcpyAsync(ctx->h_feat.get(), ctx->feat.get(), (size_t)ctx->copied * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
    return CVO_HIP_OK;
}

// one frame's device work, in stream order (also what a captured graph holds)
int enqueue_frame(cvo_fe_ctx *ctx, int dataset_seq, int feature_type)
{
    const int w = ctx->d.w, h = ctx->d.h, np = ctx->np;
    hipStream_t s = ctx->stream;
    uint8_t *img = ctx->img.get();
    const int32_t *qu = ctx->rect_map.get(), *qv = qu ? qu + rect_plane(np) : nullptr;   // (read under a distorting model)
    // a distorting camera: the images land in the raw buffers and k_fe_rectify fills img / depth
    // (a stereo rig: the pair lands in the rig's raw buffers and k_fe_stereo_rectify fills img / right_img)
    // (a pixel format: the packed images land in buffers of their own and k_fe_unpack fills what is named above)
    const size_t img_bytes = img_row(ctx) * (size_t)img_rows(ctx);
    // (a frame from device memory: its images were brought to these buffers in front of the frame, and its depth image,
    // under a float format, converted from where it lies; this sequence then holds no copy of them)
    const bool upload = !ctx->dev_in;
    if (upload)
        FE_HIP(hipMemcpyAsync(unpacks(ctx) ? ctx->packed.get() : img_input(ctx), img_staging(ctx), img_bytes, hipMemcpyHostToDevice, s));
    // a depth camera: the depth image lands in a raw buffer of its size and the warp fills depth
    // (a gate or a mask: whatever fills the depth plane fills the gate's input, and k_fe_depth_gate fills depth)
    // (stereo: the right image is uploaded in place of a depth image, and the matcher fills that plane)
    // (a median filter: whatever fills the depth plane fills the stage's input, and k_fe_median fills what is named above)
    // (the infill stage: likewise in front of the median stage, and k_fe_infill fills what is named above)
    uint16_t *plane = source_plane(ctx);
    // (a scan source: the scan is uploaded in place of a depth image, its count in front, and the projection fills that plane)
    // (a float depth format: the float image lands in a buffer of its own and k_fe_depth_convert fills what is named above)
    if (ctx->has_stereo) {
        if (upload)
            FE_HIP(hipMemcpyAsync(unpacks(ctx) ? ctx->packed_r.get() : right_input(ctx), right_staging(ctx), img_bytes,
                                  hipMemcpyHostToDevice, s));
    } else if (ctx->has_lidar)
        FE_HIP(hipMemcpyAsync(ctx->d_scan.get(), ctx->h_scan.get(), lidar_scan_bytes(ctx->lidar.max_points, ctx->scan_record),
                              hipMemcpyHostToDevice, s));
    else if (upload && converts(ctx))
        FE_HIP(hipMemcpyAsync(ctx->fdepth.get(), ctx->h_fdepth.get(), (size_t)ctx->dw * ctx->dh * depth_item(ctx), hipMemcpyHostToDevice, s));
    else if (upload)
        FE_HIP(hipMemcpyAsync(depth_input(ctx), ctx->h_depth.get(), (size_t)ctx->dw * ctx->dh * 2, hipMemcpyHostToDevice, s));
    FE_HIP(hipMemcpyAsync(ctx->ctrl.get(), ctx->h_ctrl.get(), sizeof(FeCtrl), hipMemcpyHostToDevice, s));
    if (upload && converts(ctx) && !ctx->has_stereo && !ctx->has_lidar)   // (the depth-format contract)
        enqueue_depth_convert(ctx, ctx->fdepth.get(), (size_t)ctx->dw * depth_item(ctx), dataset_seq);
    if (unpacks(ctx)) {   // (the unpack contract: in front of everything else in the frame, one launch for a pair)
        FeUnpackArgs u{};
        u.src[0] = ctx->packed.get(); u.dst[0] = img_input(ctx);
        u.src[1] = ctx->has_stereo ? ctx->packed_r.get() : nullptr; u.dst[1] = ctx->has_stereo ? right_input(ctx) : nullptr;
        u.w = ctx->iw; u.h = ctx->ih; u.format = ctx->pixfmt; u.images = ctx->has_stereo ? 2 : 1;
        fe_unpack_enqueue(u, s);
    }
    if (ctx->has_photo) {   // (the photometric contract: behind the unpack, in front of the bin, in place, one launch for a pair)
        FE_HIP(hipMemcpyAsync(ctx->photo_hdr.get(), ctx->h_photo_hdr.get(), sizeof(FePhotoHeader), hipMemcpyHostToDevice, s));
        FePhotoArgs p{};
        p.img[0] = img_input(ctx); p.img[1] = ctx->has_stereo ? right_input(ctx) : nullptr;
        p.images = ctx->has_stereo ? 2 : 1; p.w = ctx->iw; p.h = ctx->ih;
        p.response = ctx->photo_response.get(); p.vignette = ctx->photo_vignette.get();
        p.hdr = ctx->photo_hdr.get(); p.state = ctx->photo_state.get(); p.set = ctx->photo;
        fe_photo_enqueue(p, s);
        if (ctx->photo.flags & CVO_FE_PHOTO_AUTO)   // (the frame's record, read at collect())
            FE_HIP(hipMemcpyAsync(ctx->h_photo_rec.get(), &ctx->photo_state.get()->rec, sizeof(cvo_fe_photometric_frame),
                                  hipMemcpyDeviceToHost, s));
    }
    if (ctx->has_bin) {   // (the binning contract: behind those two, in front of everything else, one launch for all planes)
        FeBinArgs b{};
        b.src[0] = ctx->full_img.get(); b.dst[0] = img_landing(ctx);
        if (ctx->has_stereo) {
            b.src[1] = ctx->full_right.get(); b.dst[1] = right_landing(ctx);
        } else if (bins_depth(ctx)) {
            b.src[1] = ctx->full_depth.get(); b.dst[1] = depth_upload(ctx); b.is_depth[1] = 1;
        }
        b.w = w; b.h = h; b.factor = ctx->bin.factor; b.depth_min = ctx->bin.depth_min; b.planes = b.src[1] ? 2 : 1;
        fe_bin_enqueue(b, s);
    }
    const int32_t *srig_qu = ctx->srig_map.get();   // (read under a stereo rig: qu, qv left, qu, qv right)
    if (ctx->has_srig) {
        const size_t plane = rect_plane(np);
        StereoRectifyArgs r{};
        r.raw_l = ctx->srig_raw_l.get(); r.raw_r = ctx->srig_raw_r.get();
        r.qu_l = srig_qu; r.qv_l = srig_qu + plane; r.qu_r = srig_qu + 2 * plane; r.qv_r = srig_qu + 3 * plane;
        r.dst_l = img; r.dst_r = ctx->right_img.get(); r.valid = ctx->srig_valid.get();
        r.w = w; r.h = h;
        hipLaunchKernelGGL(k_fe_stereo_rectify, dim3(blocks((np + 3) / 4), 2), dim3(FE_BLOCK), 0, s, r);
    }
    if (ctx->has_stereo) {   // (neither a distorting model nor a depth camera beside it: cvo_fe_set_stereo)
        const cvo_fe_stereo &st = ctx->stereo;
        FeStereoArgs a{};
        a.valid = ctx->has_srig ? ctx->srig_valid.get() : nullptr;
        a.left = img; a.right = ctx->right_img.get();
        a.gray_l = ctx->gray.get();   // (k_fe_level0 writes the same bytes again)
        a.gray_r = ctx->right_gray.get();
        a.census_l = ctx->census.get(); a.census_r = ctx->census.get() + np;
        a.sum = ctx->sgm_sum.get(); a.win = ctx->stereo_win.get(); a.table = ctx->depth_table.get();
        a.disparity = ctx->disparity.get(); a.flags = ctx->stereo_flags.get(); a.depth = plane;
        a.w = w; a.h = h; a.D = st.max_disp;
        a.min_disp = st.min_disp; a.p1 = st.p1; a.p2 = st.p2; a.uniqueness = st.uniqueness; a.lr_max = st.lr_max;
        a.paths = ctx->stereo_paths;
        fe_stereo_enqueue(a, s);
        if (ctx->has_speckle) {   // (the speckle contract: on the plane the gate, if any, and level 0 read next)
            FeSpeckleArgs f{};
            f.plane = a.disparity; f.flags = a.flags; f.depth = plane;
            f.labels = ctx->speckle_words.get(); f.sums = f.labels + np; f.sizes = f.sums + np; f.removed = f.sizes + np;
            f.w = w; f.h = h; f.max_size = ctx->speckle.max_size; f.max_diff = ctx->speckle.max_diff;
            fe_speckle_enqueue(f, s);
        }
    }
    if (ctx->rectify)
        hipLaunchKernelGGL(k_fe_rectify, dim3(blocks((np + 3) / 4)), dim3(FE_BLOCK), 0, s, ctx->raw_img.get(),
                           ctx->has_rig || ctx->has_lidar ? (const uint16_t *)nullptr : ctx->raw_depth.get(), qu, qv, w, h, img,
                           plane);
    if (ctx->has_rig) {
        const cvo_fe_depth_camera &r = ctx->rig;
        DepthWarpArgs a{};
        a.depth = ctx->rig_depth.get(); a.rays = ctx->rays.get(); a.z = ctx->zbuf.get();
        a.dw = r.width; a.dh = r.height; a.w = w; a.h = h;
        a.scale = r.depth_scale; a.min_range = r.min_range; a.max_range = r.max_range;
        for (int q = 0; q < 9; ++q) a.R[q] = r.R[q];
        for (int q = 0; q < 3; ++q) a.T[q] = r.T[q];
        camera_in_force(ctx, dataset_seq, a.cam);
        hipLaunchKernelGGL(k_fe_depth_warp, dim3(blocks(a.dw * a.dh)), dim3(FE_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_fe_depth_final, dim3(blocks((np + 3) / 4)), dim3(FE_BLOCK), 0, s, ctx->zbuf.get(), np, plane);
    }
    if (ctx->has_lidar) {   // (the LiDAR contract; neither stereo nor a depth camera beside it: cvo_fe_set_lidar)
        const cvo_fe_lidar &l = ctx->lidar;
        float cam[5];
        camera_in_force(ctx, dataset_seq, cam);
        enqueue_lidar_project(l, cam, ctx->d_scan.get(), l.max_points, ctx->zbuf.get(), w, h,
                              ctx->has_sweep ? &ctx->sweep : nullptr, nullptr, nullptr, s);
        const bool cull = l.occl_rel > 0.0f;   // (without the test P is P0, written where P goes)
        hipLaunchKernelGGL(k_fe_depth_final, dim3(blocks((np + 3) / 4)), dim3(FE_BLOCK), 0, s, ctx->zbuf.get(), np,
                           cull ? ctx->lidar_p0.get() : plane);
        if (cull) {
            FeLidarCullArgs c{};
            c.p0 = ctx->lidar_p0.get(); c.p = plane; c.flags = ctx->lidar_flags.get();
            c.w = w; c.h = h; c.rx = l.occl_rx; c.ry = l.occl_ry; c.occl_rel = l.occl_rel;
            fe_lidar_cull_enqueue(c, s);
        }
    }
    if (ctx->has_infill) {   // (the infill contract: directly behind the producers, for every kind of frame)
        FeInfillArgs f{};
        f.s = plane; f.f = filled_plane(ctx); f.flags = ctx->infill_flags.get();
        f.w = w; f.h = h; f.gap_x = ctx->infill.gap_x; f.gap_y = ctx->infill.gap_y; f.jump_rel = ctx->infill.jump_rel;
        fe_infill_enqueue(f, s);
    }
    if (ctx->has_median) {   // (the median contract: directly in front of the gate, for every kind of frame)
        FeMedianArgs m{};
        m.a = filled_plane(ctx); m.b = depth_plane(ctx); m.flags = ctx->median_flags.get();
        m.w = w; m.h = h; m.radius = ctx->median.radius; m.fill_min = ctx->median.fill_min;
        fe_median_enqueue(m, s);
    }
    if (gate_active(ctx)) {
        GateArgs g{};
        g.u = ctx->ungated.get(); g.depth = ctx->depth.get(); g.flags = ctx->gate_flags.get();
        g.mask = ctx->has_mask ? ctx->d_mask.get() : nullptr;
        // the mask lies on the grid of the image as uploaded: under a distorting model it follows the map, under a
        // stereo rig the left camera's
        g.qu = !ctx->has_mask ? nullptr : ctx->has_srig ? srig_qu : ctx->rectify ? qu : nullptr;
        g.qv = !g.qu ? nullptr : ctx->has_srig ? srig_qu + rect_plane(np) : qv;
        g.w = w; g.h = h;
        float cam[5];
        camera_in_force(ctx, dataset_seq, cam);
        g.scale = cam[0];
        if (ctx->has_gate) {
            g.min_range = ctx->gate.min_range; g.max_range = ctx->gate.max_range; g.jump_rel = ctx->gate.jump_rel;
            g.grow = ctx->gate.grow; g.hole_border = ctx->gate.hole_border;
        }
        const dim3 tiles((w + FG_TW - 1) / FG_TW, (h + FG_TH - 1) / FG_TH);
        switch (g.grow) {   // (0..3: cvo_fe_check_depth_gate)
        case 0: hipLaunchKernelGGL(k_fe_depth_gate<0>, tiles, dim3(FE_BLOCK), 0, s, g); break;
        case 1: hipLaunchKernelGGL(k_fe_depth_gate<1>, tiles, dim3(FE_BLOCK), 0, s, g); break;
        case 2: hipLaunchKernelGGL(k_fe_depth_gate<2>, tiles, dim3(FE_BLOCK), 0, s, g); break;
        default: hipLaunchKernelGGL(k_fe_depth_gate<3>, tiles, dim3(FE_BLOCK), 0, s, g); break;
        }
    }

    const FeDims &d = ctx->d;
    hipLaunchKernelGGL(k_fe_level0, dim3(blocks(np)), dim3(FE_BLOCK), 0, s, img, w, h, ctx->sdiv.get(), ctx->hdiv.get(),
                       ctx->gray.get(), ctx->hsv.get(), ctx->I[0].get(), ctx->ag[0].get(), ctx->dx0.get(), ctx->dy0.get());
    for (int l = 1; l < FE_LEVELS; ++l)
        hipLaunchKernelGGL(k_fe_level, dim3(blocks(d.wl[l] * d.hl[l])), dim3(FE_BLOCK), 0, s, ctx->I[l - 1].get(),
                           2 * d.wl[l] /* the reference's row stride of the level above, also when
                                           that level is one pixel wider (ref src/pcd_generator.cpp:82) */,
                           ctx->I[l].get(), d.wl[l], d.hl[l], ctx->ag[l].get());
    const int ncell = d.w32 * d.h32;
    float *map = ctx->map.get();
    FeCtrl *ctrl = ctx->ctrl.get();
    int *blk_cnt = ctx->blk_cnt.get(), *cnt = ctx->cnt.get();
    hipLaunchKernelGGL(k_fe_hist, dim3(ncell), dim3(FE_BLOCK), 0, s, ctx->ag[0].get(), w, h, d.w32, ctx->ths.get());
    hipLaunchKernelGGL(k_fe_smooth, dim3(blocks(ncell)), dim3(FE_BLOCK), 0, s, ctx->ths.get(), d.w32, d.h32, ctx->ths_s.get());
    // the selection contract: among the pixels of the final depth plane, which is complete here
    const bool by_depth = ctx->select_mode == CVO_FE_SELECT_DEPTH;
    SelectArgs sa{ctx->ag[0].get(), ctx->ag[1].get(), ctx->ag[2].get(), ctx->ths_s.get(), map, ctrl, blk_cnt, w, h, d.w32, ncell, 0,
                  by_depth ? ctx->depth.get() : nullptr};
    const auto select = by_depth ? k_fe_select<true> : k_fe_select<false>;
    const int nb0 = (((w + 11) / 12) * ((h + 11) / 12) + 3) / 4;   // potential 3: one wave per 12 x 12 block
    hipLaunchKernelGGL(select, dim3(nb0), dim3(FE_BLOCK), 0, s, sa);
    hipLaunchKernelGGL(k_fe_decide, dim3(1), dim3(FE_BLOCK), 0, s, ctrl, blk_cnt, nb0, 0, (float)ctx->num_want);
    sa.pass = 1;
    const int nb1 = (((w + 3) / 4) * ((h + 3) / 4) + 3) / 4;       // any potential >= 1
    hipLaunchKernelGGL(select, dim3(nb1), dim3(FE_BLOCK), 0, s, sa);
    hipLaunchKernelGGL(k_fe_decide, dim3(1), dim3(FE_BLOCK), 0, s, ctrl, blk_cnt, nb1, 1, (float)ctx->num_want);
    hipLaunchKernelGGL(k_fe_count<0>, dim3(ctx->nchunks), dim3(FE_BLOCK), 0, s, map, ctx->depth.get(), np, ctrl, cnt);
    hipLaunchKernelGGL(k_fe_subsample, dim3(ctx->nchunks), dim3(FE_BLOCK), 0, s, map, np, ctx->pattern.get(), cnt, ctrl);
    FE_HIP(hipGetLastError());
    // the cloud is emitted at once; a frame that needs the edge top-up (rare: a nearly
    // texture-free image) is noticed at collect(), when the control block has arrived, and
    // emitted again
    return run_emit(ctx, dataset_seq, feature_type);
}

int collect_impl(cvo_fe_ctx *ctx, float *positions, float *features, int capacity, int *num_points, bool to_host)
{
    if (!ctx->pending) return fail(ctx, CVO_HIP_ERR_INVALID, "collect: no frame was submitted");
    ctx->pending = false;
    FE_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    FE_HIP(hipStreamSynchronize(s));
    int rc = CVO_HIP_OK;
    // ref src/pcd_generator.cpp:141-144: fewer than a third of what was asked for?
    const int num_selected = ctx->h_ctrl->in_map;   // (before any top-up: that is what the reference tests)
    const bool canny = num_selected < ctx->num_want / 3;
    if (canny) {
        rc = run_canny(ctx);
        if (!rc) rc = run_emit(ctx, ctx->p_seq, ctx->p_ftype);
        if (rc) return rc;
        FE_HIP(hipStreamSynchronize(s));
    }
    const FeCtrl &c = *ctx->h_ctrl;
    ctx->info.num_selected = num_selected;
    ctx->info.reselected = c.redo;
    ctx->info.pot_used = c.pot[c.redo ? 1 : 0];
    ctx->info.canny_used = canny ? 1 : 0;
    ctx->info.num_points = c.num_points;
    if (ctx->has_photo) {   // (no setter runs while a frame is in flight: the setting is the frame's)
        if (ctx->photo.flags & CVO_FE_PHOTO_AUTO) ctx->photo_frame = *ctx->h_photo_rec;
        else fe_photo_plain_record(*ctx->h_photo_hdr, &ctx->photo_frame);
    }
    *num_points = c.num_points;
    const int ncopy = std::min(std::min(c.num_points, capacity), ctx->cap);
    float *h_pos = ctx->h_pos.get(), *h_feat = ctx->h_feat.get();
    if (to_host && ncopy > ctx->copied) {   // an unusually large cloud: fetch the rest
        const size_t from = (size_t)ctx->copied, more = (size_t)(ncopy - ctx->copied);
        FE_HIP(hipMemcpyAsync(h_pos + from * 3, ctx->pos.get() + from * 3, more * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        FE_HIP(hipMemcpyAsync(h_feat + from * 5, ctx->feat.get() + from * 5, more * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
        FE_HIP(hipStreamSynchronize(s));
    }
    if (to_host && ncopy > 0) {
        std::memcpy(positions, h_pos, (size_t)ncopy * 3 * sizeof(float));
        std::memcpy(features, h_feat, (size_t)ncopy * 5 * sizeof(float));
    }
    if (c.num_points > ncopy) return fail(ctx, CVO_HIP_ERR_INVALID, "create_pointcloud: more points than capacity");
    return CVO_HIP_OK;
}

}   // namespace

extern "C" {

int cvo_fe_random_pattern(int n, uint8_t *out)
{
    if (n < 0 || (n > 0 && !out)) return CVO_HIP_ERR_INVALID;
    LibcRand g(3141592u);
    for (int i = 0; i < n; ++i) out[i] = (uint8_t)(g.next() & 0xFF);
    return CVO_HIP_OK;
}

int cvo_fe_camera(int dataset_seq, float cam[5])
{
    if (!cam) return CVO_HIP_ERR_INVALID;
    const int k = (dataset_seq >= 0 && dataset_seq <= 5) ? dataset_seq : 0;   // default: RealSense (ref :287-294)
    for (int q = 0; q < 5; ++q) cam[q] = kCameras[k][q];
    return CVO_HIP_OK;
}

const char *cvo_fe_last_error(const cvo_fe_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cvo_fe_destroy(cvo_fe_ctx *ctx)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    drop_graphs(ctx);
    const hipStream_t own = ctx->own_stream ? ctx->stream : nullptr;
    delete ctx;   // (every buffer goes with its owner)
    if (own) (void)hipStreamDestroy(own);
    return CVO_HIP_OK;
}

int cvo_fe_create(int device, void *stream, int width, int height, cvo_fe_ctx **out)
{
    cvo_lock::Api api_guard;
    if (!out || width < 64 || height < 64 || (long long)width * height > (1ll << 26)) return CVO_HIP_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return CVO_HIP_ERR_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CVO_HIP_ERR_NODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CVO_HIP_ERR_NODEVICE;
    cvo_fe_ctx *ctx = new (std::nothrow) cvo_fe_ctx;
    if (!ctx) return CVO_HIP_ERR_NOMEM;
    ctx->device = device;
    auto bail = [&](int code) { cvo_fe_destroy(ctx); return code; };
    if (hipSetDevice(device) != hipSuccess) return bail(CVO_HIP_ERR_HIP);
    if (stream) ctx->stream = (hipStream_t)stream;
    else {
        // lowest priority: when a frame is prepared while the previous one is being registered
        // (submit / collect), the registration's latency-bound launch chain goes first
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, least) != hipSuccess)
            return bail(CVO_HIP_ERR_HIP);
        ctx->own_stream = true;
    }
    FeDims &d = ctx->d;
    d.w = width; d.h = height; d.w32 = width / 32; d.h32 = height / 32;
    ctx->dw = width; ctx->dh = height;
    ctx->iw = width; ctx->ih = height;
    int wl = width, hl = height;
    for (int l = 0; l < FE_LEVELS; ++l) { d.wl[l] = wl; d.hl[l] = hl; wl /= 2; hl /= 2; }
    const size_t np = (size_t)width * height;
    ctx->np = (int)np;
    ctx->nchunks = (int)((np + FE_CHUNK - 1) / FE_CHUNK);
    ctx->cap = (int)np;   // (a selection can never hold more points than the image has pixels)
    const size_t cap = np, ncell = (size_t)d.w32 * d.h32 + 1;
    bool ok = dev_alloc(ctx->img, np * 3) && dev_alloc(ctx->gray, np) && dev_alloc(ctx->pattern, np) &&
              dev_alloc(ctx->tmp8, np) && dev_alloc(ctx->st8, np) && dev_alloc(ctx->edges, np) &&
              dev_alloc(ctx->depth, np) && dev_alloc(ctx->hsv, np);
    for (int l = 0; l < FE_LEVELS; ++l) {
        const size_t nl = (size_t)d.wl[l] * d.hl[l] + 8;
        ok = ok && dev_alloc(ctx->I[l], nl) && dev_alloc(ctx->ag[l], nl);
    }
    ok = ok && dev_alloc(ctx->dx0, np) && dev_alloc(ctx->dy0, np) && dev_alloc(ctx->map, np) &&
         dev_alloc(ctx->ths, ncell) && dev_alloc(ctx->ths_s, ncell) && dev_alloc(ctx->pos, cap * 3) &&
         dev_alloc(ctx->feat, cap * 5) && dev_alloc(ctx->sdiv, 256) && dev_alloc(ctx->hdiv, 256) &&
         dev_alloc(ctx->cnt, 2 * (size_t)ctx->nchunks) && dev_alloc(ctx->mag, np) && dev_alloc(ctx->grad, np) &&
         dev_alloc(ctx->ctrl, 1) &&
         dev_alloc(ctx->blk_cnt, 3 * ((size_t)((width + 3) / 4) * ((height + 3) / 4) / 4 + 2)) &&
         pin_alloc(ctx->h_img, np * 3) && pin_alloc(ctx->h_depth, np) && pin_alloc(ctx->h_ctrl, 1) &&
         pin_alloc(ctx->h_pos, cap * 3) && pin_alloc(ctx->h_feat, cap * 5);
    if (!ok) return bail(CVO_HIP_ERR_NOMEM);
    // OpenCV's reciprocal tables of the 8-bit HSV conversion (12-bit fixed point)
    int sdiv[256], hdiv[256];
    sdiv[0] = hdiv[0] = 0;
    for (int i = 1; i < 256; ++i) {
        sdiv[i] = (int)std::lrint((255 << 12) / (1. * i));
        hdiv[i] = (int)std::lrint((180 << 12) / (6. * i));
    }
    // the selector's pattern does not depend on the frame: made once (the reference
    // re-seeds and redraws it for every frame, ref thirdparty/PixelSelector2.cpp:33-37)
    cvo_fe_random_pattern((int)np, ctx->h_img.get());
    if (hipMemcpy(ctx->pattern.get(), ctx->h_img.get(), np, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ctx->sdiv.get(), sdiv, sizeof(sdiv), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ctx->hdiv.get(), hdiv, sizeof(hdiv), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(ctx->edges.get(), 0, np) != hipSuccess || hipMemset(ctx->map.get(), 0, np * sizeof(float)) != hipSuccess)
        return bail(CVO_HIP_ERR_HIP);
    *out = ctx;
    return CVO_HIP_OK;
}

int cvo_fe_host_buffers(cvo_fe_ctx *ctx, uint8_t **img, uint16_t **depth)
{
    if (!ctx || !img || !depth) return CVO_HIP_ERR_INVALID;
    *img = img_staging(ctx);
    *depth = (uint16_t *)depth_staging(ctx);
    return CVO_HIP_OK;
}

}   // extern "C"

namespace {

// submit() of any kind of frame: `second` is the depth image (uint16 rows) of a depth frame, the right colour image of
// a stereo frame (`stereo`), and the `num_points` records of a scan, second_stride bytes apart, of a LiDAR frame
// (`lidar`); the kind must be the one the context is set up for
// An image a caller hands over in device memory (the device-input contract of cvo_frontend.h): device memory of the
// context's device, and, where the runtime knows the allocation's range, inside it.  Nothing is enqueued before every
// image of the frame has passed.
int device_image_ok(cvo_fe_ctx *ctx, const void *p, size_t stride, size_t row, int rows, const char *refused)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device) {
        (void)hipGetLastError();   // (an unknown pointer is an error of the runtime's: taken, so that the next frame does not find it)
        return fail(ctx, CVO_HIP_ERR_INVALID, refused);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_OK;   // (no answer: the image is taken at the caller's word)
    }
    if ((uintptr_t)p < (uintptr_t)base || !input_fits((uintptr_t)p - (uintptr_t)base, size, (size_t)rows, stride, row))
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit_device: an image ends past the end of its allocation");
    return CVO_HIP_OK;
}

// `device`: img and second are device memory (cvo_fe_submit_device, cvo_fe_submit_stereo_device)
int submit_frame(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const void *second, size_t second_stride,
                 int dataset_seq, int feature_type, bool stereo, bool lidar = false, int num_points = 0, bool device = false)
{
    const int np = ctx->np;
    const int dw = ctx->dw, dh = ctx->dh;   // (the depth camera's image, if the context has one)
    if (lidar != ctx->has_lidar)
        return fail(ctx, CVO_HIP_ERR_INVALID, lidar ? "submit_lidar: no scan source (cvo_fe_set_lidar)"
                                                    : "submit: a scan source is set, a frame is an image and a scan (cvo_fe_submit_lidar)");
    if (stereo != ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, stereo ? "submit_stereo: no stereo settings (cvo_fe_set_stereo)"
                                                     : "submit: stereo is set, a frame is a stereo pair (cvo_fe_submit_stereo)");
    if (lidar && (num_points < 0 || num_points > ctx->lidar.max_points || !lidar_stride_ok(second_stride) ||
                  (!second && num_points > 0)))
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit_lidar: num_points in [0, max_points], a stride of at least 12 bytes "
                                              "and a multiple of 4, points not null");
    const int time_offset = lidar && ctx->has_sweep ? sweep_time_offset(&ctx->sweep) : -1;
    if (time_offset >= 0 && (size_t)time_offset + 4 > second_stride)
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit_lidar: the sweep's time_offset + 4 is beyond the stride");
    const size_t row = img_row(ctx);   // (of the pixel format in force: w * 3 without one)
    const size_t ditem = depth_item(ctx), drow = (size_t)dw * ditem;   // (of the depth format in force: dw * 2 without one)
    if (!img || (!second && !lidar) || img_stride < row ||
        (!lidar && second_stride < (stereo ? row : drow)) ||
        (feature_type != CVO_FE_FEATURES_HSV && feature_type != CVO_FE_FEATURES_RGB))
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit: bad argument");
    if (!lidar && !stereo && (converts(ctx) || device) && second_stride % ditem != 0)
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit: the depth stride is not a multiple of the size of a depth value");
    if (ctx->pending) return fail(ctx, CVO_HIP_ERR_INVALID, "submit: the previous frame was not collected");
    FE_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (device) {   // (every image is checked before anything is enqueued)
        if (!stereo && (uintptr_t)second % ditem != 0)
            return fail(ctx, CVO_HIP_ERR_INVALID, "submit_device: the depth image is not aligned to the size of a depth value");
        int rc = device_image_ok(ctx, img, img_stride, row, img_rows(ctx),
                                 "submit_device: the colour image is not device memory of the context's device");
        if (!rc)
            rc = device_image_ok(ctx, second, second_stride, stereo ? row : drow, stereo ? img_rows(ctx) : dh,
                                 stereo ? "submit_stereo_device: the right image is not device memory of the context's device"
                                        : "submit_device: the depth image is not device memory of the context's device");
        if (rc) return rc;
    }
    // pinned staging (not when the caller decoded into the staging image itself: cvo_fe_host_buffers)
    if (!device && !(img == img_staging(ctx) && img_stride == row)) copy_rows(img_staging(ctx), img, img_stride, row, img_rows(ctx));
    if (stereo) {
        if (!device) copy_rows(right_staging(ctx), second, second_stride, row, img_rows(ctx));
        // the table U(q) of the camera in force, if the device holds another's: in front of the frame, outside the
        // captured graph (its address is the graph's), as the mask below
        float cam[5];
        camera_in_force(ctx, dataset_seq, cam);
        if (cam[1] != ctx->table_fx || cam[0] != ctx->table_scale) {
            cvo_fe_stereo st = ctx->stereo;
            if (ctx->has_srig) st.baseline = ctx->srig.baseline;   // (the rig's: the settings' is not read under a rig)
            if (cvo_fe_stereo_depth_table(&st, cam[1], cam[0], ctx->h_depth_table.get()) != CVO_HIP_OK)
                return fail(ctx, CVO_HIP_ERR_INVALID, "submit_stereo: depth table");
            FE_HIP(hipMemcpyAsync(ctx->depth_table.get(), ctx->h_depth_table.get(), (size_t)16 * ctx->stereo.max_disp * 2,
                                  hipMemcpyHostToDevice, s));
            ctx->table_fx = cam[1];
            ctx->table_scale = cam[0];
        }
    } else if (lidar)
        lidar_stage(ctx->h_scan.get(), second, second_stride, num_points, time_offset, ctx->lidar_twist);
    else if (!device && !(second == depth_staging(ctx) && second_stride == drow))
        copy_rows(depth_staging(ctx), second, second_stride, drow, dh);
    if (device) {
        // The caller's images: in front of the frame, outside the captured graph (a graph must not hold a caller's
        // pointer), as the mask below.  One pitched copy per image into the buffer its upload lands in; a float depth
        // image is not copied: the conversion reads it where it lies.
        const size_t rows = (size_t)img_rows(ctx);
        FE_HIP(hipMemcpy2DAsync(unpacks(ctx) ? ctx->packed.get() : img_input(ctx), row, img, img_stride, row, rows,
                                hipMemcpyDeviceToDevice, s));
        if (stereo)
            FE_HIP(hipMemcpy2DAsync(unpacks(ctx) ? ctx->packed_r.get() : right_input(ctx), row, second, second_stride, row, rows,
                                    hipMemcpyDeviceToDevice, s));
        else if (converts(ctx)) {
            enqueue_depth_convert(ctx, second, second_stride, ctx->custom || ctx->has_srig ? 0 : dataset_seq);
            FE_HIP(hipGetLastError());
        } else
            FE_HIP(hipMemcpy2DAsync(depth_input(ctx), drow, second, second_stride, drow, (size_t)dh, hipMemcpyDeviceToDevice, s));
    }
    ctx->dev_in = device;   // (read by enqueue_frame: such a frame's sequence holds no upload of the images)
    FeCtrl c0{};
    c0.pot[0] = 3;   // a selector starts every frame at potential 3 (ref PixelSelector2.cpp:39)
    *ctx->h_ctrl = c0;
    if (ctx->has_photo) {   // (the frame's gains and the lock's opening travel in the header the sequence copies)
        fe_photo_header(ctx->photo, ctx->photo_gain, ctx->photo_rearm, ctx->h_photo_hdr.get());
        ctx->photo_rearm = false;
    }
    // a mask set since the last frame: in front of the frame, outside the captured graph (its address is the graph's)
    if (ctx->has_mask && ctx->mask_dirty) {
        FE_HIP(hipMemcpyAsync(ctx->d_mask.get(), ctx->h_mask.get(), (size_t)np, hipMemcpyHostToDevice, s));
        ctx->mask_dirty = false;
    }
    // Everything from here to the copies back is the same sequence for every frame (fixed
    // buffers, fixed pinned staging): captured once per (camera, feature type, num_want,
    // output mode) and launched as one hipGraph -- 3 copies in, 11 kernels, the copies out.
    static const bool no_graph = getenv("CVO_FE_NO_GRAPH") != nullptr;
    const int seq_given = dataset_seq;
    if (ctx->custom || ctx->has_srig) dataset_seq = 0;   // (ignored: one key whatever the caller passed)
    const uint64_t key = ((uint64_t)(uint32_t)dataset_seq << 40) ^ ((uint64_t)feature_type << 36) ^
                         ((uint64_t)ctx->device_output << 32) ^ ((uint64_t)device << 33) ^ (uint64_t)(uint32_t)ctx->num_want;
    int rc = CVO_HIP_OK;
    FeGraph *g = nullptr;
    for (auto &e : ctx->graphs)
        if (e.key == key && e.cam_gen == ctx->cam_gen) g = &e;
    if (!no_graph && !g && ctx->graphs.size() < 8) {
        FeGraph ng;
        ng.key = key;
        ng.cam_gen = ctx->cam_gen;
        cvo_lock::Capture alone;   // (see cvo_lock.h)
        if (alone.ok && hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
            rc = enqueue_frame(ctx, dataset_seq, feature_type);
            const hipError_t e = hipStreamEndCapture(s, &ng.graph);
            if (!rc && e == hipSuccess && ng.graph &&
                hipGraphInstantiate(&ng.exec, ng.graph, nullptr, nullptr, 0) == hipSuccess) {
                ctx->graphs.push_back(ng);
                g = &ctx->graphs.back();
            } else {
                if (ng.graph) (void)hipGraphDestroy(ng.graph);
                (void)hipGetLastError();
                rc = CVO_HIP_OK;
            }
        }
    }
    ctx->copied = optimistic_copy(ctx);   // (a launched graph does not pass run_emit)
    if (g) {
        FE_HIP(hipGraphLaunch(g->exec, s));
    } else {
        rc = enqueue_frame(ctx, dataset_seq, feature_type);
        if (rc) return rc;
    }
    ctx->pending = true;
    ctx->p_seq = seq_given;
    ctx->p_ftype = feature_type;
    return CVO_HIP_OK;
}

}   // namespace

extern "C" {

int cvo_fe_submit(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const uint16_t *depth,
                  size_t depth_stride, int dataset_seq, int feature_type)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    return submit_frame(ctx, img, img_stride, depth, depth_stride, dataset_seq, feature_type, false);
}

int cvo_fe_submit_stereo(cvo_fe_ctx *ctx, const uint8_t *left, size_t left_stride, const uint8_t *right,
                         size_t right_stride, int dataset_seq, int feature_type)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    return submit_frame(ctx, left, left_stride, right, right_stride, dataset_seq, feature_type, true);
}

int cvo_fe_submit_device(cvo_fe_ctx *ctx, const void *d_img, size_t img_stride, const void *d_depth, size_t depth_stride,
                         int dataset_seq, int feature_type)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (ctx->has_lidar)
        return fail(ctx, CVO_HIP_ERR_INVALID, "submit_device: a scan source is set; a scan is staged by the host (cvo_fe_submit_lidar)");
    return submit_frame(ctx, (const uint8_t *)d_img, img_stride, d_depth, depth_stride, dataset_seq, feature_type, false, false, 0,
                        true);
}

int cvo_fe_submit_stereo_device(cvo_fe_ctx *ctx, const void *d_left, size_t left_stride, const void *d_right,
                                size_t right_stride, int dataset_seq, int feature_type)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    return submit_frame(ctx, (const uint8_t *)d_left, left_stride, d_right, right_stride, dataset_seq, feature_type, true, false, 0,
                        true);
}

int cvo_fe_submit_lidar(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const void *points, size_t stride_bytes,
                        int num_points, int dataset_seq, int feature_type)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    return submit_frame(ctx, img, img_stride, points, stride_bytes, dataset_seq, feature_type, false, true, num_points);
}

int cvo_fe_collect(cvo_fe_ctx *ctx, float *positions, float *features, int capacity, int *num_points)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!num_points || capacity < 0 || (capacity > 0 && (!positions || !features)))
        return fail(ctx, CVO_HIP_ERR_INVALID, "collect: bad argument");
    return collect_impl(ctx, positions, features, capacity, num_points, true);
}

int cvo_fe_collect_device(cvo_fe_ctx *ctx, const float **d_positions, const float **d_features, int *num_points)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!d_positions || !d_features || !num_points) return fail(ctx, CVO_HIP_ERR_INVALID, "collect_device: bad argument");
    const int rc = collect_impl(ctx, nullptr, nullptr, ctx->cap, num_points, false);
    *d_positions = ctx->pos.get();
    *d_features = ctx->feat.get();
    return rc;
}

int cvo_fe_create_pointcloud(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const uint16_t *depth,
                             size_t depth_stride, int dataset_seq, int feature_type, float *positions,
                             float *features, int capacity, int *num_points)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!num_points || capacity < 0 || (capacity > 0 && (!positions || !features)))
        return fail(ctx, CVO_HIP_ERR_INVALID, "create_pointcloud: bad argument");
    const int rc = cvo_fe_submit(ctx, img, img_stride, depth, depth_stride, dataset_seq, feature_type);
    if (rc) return rc;
    return cvo_fe_collect(ctx, positions, features, capacity, num_points);
}

int cvo_fe_create_pointcloud_stereo(cvo_fe_ctx *ctx, const uint8_t *left, size_t left_stride, const uint8_t *right,
                                    size_t right_stride, int dataset_seq, int feature_type, float *positions,
                                    float *features, int capacity, int *num_points)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!num_points || capacity < 0 || (capacity > 0 && (!positions || !features)))
        return fail(ctx, CVO_HIP_ERR_INVALID, "create_pointcloud_stereo: bad argument");
    const int rc = cvo_fe_submit_stereo(ctx, left, left_stride, right, right_stride, dataset_seq, feature_type);
    if (rc) return rc;
    return cvo_fe_collect(ctx, positions, features, capacity, num_points);
}

int cvo_fe_create_pointcloud_lidar(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const void *points,
                                   size_t stride_bytes, int num_points, int dataset_seq, int feature_type,
                                   float *positions, float *features, int capacity, int *num_points_out)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!num_points_out || capacity < 0 || (capacity > 0 && (!positions || !features)))
        return fail(ctx, CVO_HIP_ERR_INVALID, "create_pointcloud_lidar: bad argument");
    const int rc = cvo_fe_submit_lidar(ctx, img, img_stride, points, stride_bytes, num_points, dataset_seq, feature_type);
    if (rc) return rc;
    return cvo_fe_collect(ctx, positions, features, capacity, num_points_out);
}

int cvo_fe_get_info(const cvo_fe_ctx *ctx, cvo_fe_info *out)
{
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    *out = ctx->info;
    return CVO_HIP_OK;
}

int cvo_fe_read_stage(cvo_fe_ctx *ctx, int stage, void *out, size_t bytes)
{
    cvo_lock::Api api_guard;
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    const FeDims &d = ctx->d;
    const size_t np = (size_t)ctx->np;
    const void *src = nullptr;
    size_t need = 0;
    switch (stage) {
    case CVO_FE_STAGE_GRAY: src = ctx->gray.get(); need = np; break;
    case CVO_FE_STAGE_HSV: src = ctx->hsv.get(); need = np * 3; break;
    case CVO_FE_STAGE_MAP: src = ctx->map.get(); need = np * 4; break;
    case CVO_FE_STAGE_AG0: src = ctx->ag[0].get(); need = np * 4; break;
    case CVO_FE_STAGE_AG1: src = ctx->ag[1].get(); need = (size_t)d.wl[1] * d.hl[1] * 4; break;
    case CVO_FE_STAGE_AG2: src = ctx->ag[2].get(); need = (size_t)d.wl[2] * d.hl[2] * 4; break;
    case CVO_FE_STAGE_THS: src = ctx->ths_s.get(); need = (size_t)d.w32 * d.h32 * 4; break;
    case CVO_FE_STAGE_DX0: src = ctx->dx0.get(); need = np * 4; break;
    case CVO_FE_STAGE_DY0: src = ctx->dy0.get(); need = np * 4; break;
    case CVO_FE_STAGE_EDGES: src = ctx->edges.get(); need = np; break;
    case CVO_FE_STAGE_RECT_BGR: src = ctx->img.get(); need = np * 3; break;
    case CVO_FE_STAGE_RECT_DEPTH: src = ctx->depth.get(); need = np * 2; break;
    // (under binning without a depth camera dw x dh is the input size, and the plane the bin wrote is the context's)
    case CVO_FE_STAGE_RAW_DEPTH: src = depth_upload(ctx); need = ctx->has_rig ? (size_t)ctx->dw * ctx->dh * 2 : np * 2; break;
    case CVO_FE_STAGE_UNGATED_DEPTH: src = depth_plane(ctx); need = np * 2; break;
    case CVO_FE_STAGE_GATE: src = gate_active(ctx) ? ctx->gate_flags.get() : nullptr; need = np; break;
    case CVO_FE_STAGE_RIGHT_GRAY: src = ctx->right_gray.get(); need = np; break;
    case CVO_FE_STAGE_CENSUS_L: src = ctx->census.get(); need = np * 8; break;
    case CVO_FE_STAGE_CENSUS_R: src = ctx->census ? ctx->census.get() + np : nullptr; need = np * 8; break;
    case CVO_FE_STAGE_SGM_SUM: src = ctx->sgm_sum.get(); need = np * (size_t)ctx->stereo.max_disp * 2; break;
    case CVO_FE_STAGE_DISPARITY: src = ctx->disparity.get(); need = np * 2; break;
    case CVO_FE_STAGE_STEREO: src = ctx->stereo_flags.get(); need = np; break;
    case CVO_FE_STAGE_RIGHT_BGR: src = ctx->right_img.get(); need = np * 3; break;
    case CVO_FE_STAGE_STEREO_VALID: src = ctx->srig_valid.get(); need = np; break;
    case CVO_FE_STAGE_SPECKLE_SIZE: src = ctx->speckle_words ? ctx->speckle_words.get() + 2 * np : nullptr; need = np * 4; break;
    case CVO_FE_STAGE_UNFILTERED_DEPTH: src = ctx->unfiltered.get(); need = np * 2; break;
    case CVO_FE_STAGE_MEDIAN: src = ctx->median_flags.get(); need = np; break;
    // (without the occlusion test P0 is P, and the flags are made from it below: no plane of their own)
    case CVO_FE_STAGE_LIDAR_DEPTH: src = ctx->lidar_p0 ? ctx->lidar_p0.get() : source_plane(ctx); need = np * 2; break;
    case CVO_FE_STAGE_LIDAR: src = ctx->lidar_flags.get(); need = np; break;
    case CVO_FE_STAGE_SPARSE_DEPTH: src = ctx->sparse.get(); need = np * 2; break;
    case CVO_FE_STAGE_INFILL: src = ctx->infill_flags.get(); need = np; break;
    case CVO_FE_STAGE_INPUT_BGR: src = img_landing(ctx); need = np * 3; break;
    case CVO_FE_STAGE_INPUT_RIGHT_BGR: src = right_landing(ctx); need = np * 3; break;
    case CVO_FE_STAGE_FULL_BGR: src = ctx->full_img.get(); need = (size_t)ctx->iw * ctx->ih * 3; break;
    case CVO_FE_STAGE_FULL_RIGHT_BGR: src = ctx->full_right.get(); need = (size_t)ctx->iw * ctx->ih * 3; break;
    case CVO_FE_STAGE_FULL_DEPTH: src = ctx->full_depth.get(); need = (size_t)ctx->iw * ctx->ih * 2; break;
    default: return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: unknown stage");
    }
    if (stage >= CVO_FE_STAGE_FULL_BGR && stage <= CVO_FE_STAGE_FULL_DEPTH && !ctx->has_bin)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: an input-size plane, and input binning is not set");
    if (stage == CVO_FE_STAGE_FULL_RIGHT_BGR && !ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: the input-size right image, and the context has no stereo");
    if (stage == CVO_FE_STAGE_FULL_DEPTH && !bins_depth(ctx))
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: the input-size depth image, and a depth camera, stereo or a scan source is set");
    if ((stage == CVO_FE_STAGE_UNFILTERED_DEPTH || stage == CVO_FE_STAGE_MEDIAN) && !ctx->has_median)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: a plane of the median filter, and no filter is set");
    if ((stage == CVO_FE_STAGE_SPARSE_DEPTH || stage == CVO_FE_STAGE_INFILL) && !ctx->has_infill)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: a plane of the infill stage, and the stage is not set");
    if ((stage == CVO_FE_STAGE_INPUT_BGR || stage == CVO_FE_STAGE_INPUT_RIGHT_BGR) && !unpacks(ctx) && !ctx->has_bin && !ctx->has_photo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: an unpacked image, and the context's pixel format is BGR8");
    if (stage == CVO_FE_STAGE_INPUT_RIGHT_BGR && !ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: the unpacked right image, and the context has no stereo");
    if ((stage == CVO_FE_STAGE_LIDAR_DEPTH || stage == CVO_FE_STAGE_LIDAR) && !ctx->has_lidar)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: a plane of a scan source, and none is set");
    if (stage >= CVO_FE_STAGE_RIGHT_GRAY && stage <= CVO_FE_STAGE_SPECKLE_SIZE && !ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: a stage of a stereo frame, and stereo is not set");
    if (stage == CVO_FE_STAGE_STEREO_VALID && !ctx->has_srig)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: the validity plane of a stereo rig, and no rig is set");
    if (stage == CVO_FE_STAGE_SPECKLE_SIZE && !ctx->has_speckle)
        return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: the sizes of the speckle filter, and no filter is set");
    if (bytes < need) return fail(ctx, CVO_HIP_ERR_INVALID, "read_stage: buffer too small");
    FE_HIP(hipSetDevice(ctx->device));
    FE_HIP(hipStreamSynchronize(ctx->stream));
    if (stage == CVO_FE_STAGE_LIDAR && !src) {   // (no occlusion test: HIT where the plane holds a depth)
        std::vector<uint16_t> p0;
        try { p0.resize(np); } catch (const std::bad_alloc &) { return fail(ctx, CVO_HIP_ERR_NOMEM, "read_stage"); }
        FE_HIP(hipMemcpy(p0.data(), source_plane(ctx), np * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < np; ++i) ((uint8_t *)out)[i] = p0[i] ? (uint8_t)CVO_FE_LIDAR_HIT : (uint8_t)0;
        return CVO_HIP_OK;
    }
    if (!src) {   // (the flags of a context without gate and mask: there is no such plane, and nothing is flagged)
        std::memset(out, 0, need);
        return CVO_HIP_OK;
    }
    if (stage == CVO_FE_STAGE_HSV) {   // packed words on the device, 3 bytes per pixel for the caller
        uint32_t *tmp = new (std::nothrow) uint32_t[np];
        if (!tmp) return fail(ctx, CVO_HIP_ERR_NOMEM, "read_stage");
        const hipError_t e = hipMemcpy(tmp, src, np * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            for (size_t i = 0; i < np; ++i) {
                ((uint8_t *)out)[3 * i] = (uint8_t)(tmp[i] & 255u);
                ((uint8_t *)out)[3 * i + 1] = (uint8_t)((tmp[i] >> 8) & 255u);
                ((uint8_t *)out)[3 * i + 2] = (uint8_t)((tmp[i] >> 16) & 255u);
            }
        delete[] tmp;
        if (e != hipSuccess) return fail(ctx, CVO_HIP_ERR_HIP, "read_stage copy", e);
        return CVO_HIP_OK;
    }
    FE_HIP(hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return CVO_HIP_OK;
}

}   // extern "C"

namespace {

// the device memory and the stream of one cvo_fe_project_points call
struct ProjectCall {
    Dev<uint8_t> scan, flags;
    Dev<float> phase;   // n phases, then 3n floats of p', where the caller asked for either
    Dev<uint32_t> z;
    Dev<uint16_t> planes;
    hipStream_t s = nullptr;
    ~ProjectCall()
    {
        if (s) (void)hipStreamDestroy(s);
    }
};

// cvo_fe_project_points (sw NULL) and cvo_fe_project_points_sweep
int project_points(int device, const void *points, size_t stride_bytes, int n, const cvo_fe_lidar *l, const float cam[5],
                   int width, int height, uint16_t *plane, uint16_t *unculled, uint8_t *flags, int *hits, int *occluded,
                   const cvo_fe_lidar_sweep *sw, const float *twist, float *phase, float *moved)
{
    cvo_lock::Api api_guard;
    if (sw ? (!sweep_ok(*sw) || !twist || !twist_ok(twist)) : (phase || moved)) return CVO_HIP_ERR_INVALID;
    const int time_offset = sweep_time_offset(sw);
    if (time_offset >= 0 && (size_t)time_offset + 4 > stride_bytes) return CVO_HIP_ERR_INVALID;
    if (!plane || !cam || !hits || !occluded || n < 0 || n > FE_LIDAR_MAX_POINTS || (!points && n > 0) ||
        !lidar_stride_ok(stride_bytes) || width < 1 || height < 1 || width > 8192 || height > 8192)
        return CVO_HIP_ERR_INVALID;
    for (int q = 0; q < 5; ++q)
        if (!std::isfinite(cam[q])) return CVO_HIP_ERR_INVALID;
    if (!(cam[0] > 0.0f && cam[1] > 0.0f && cam[2] > 0.0f)) return CVO_HIP_ERR_INVALID;
    if (!l) return CVO_HIP_ERR_INVALID;
    cvo_fe_lidar checked = *l;
    checked.max_points = 1;   // (not read beyond n <= 2^21)
    if (!lidar_ok(checked)) return CVO_HIP_ERR_INVALID;
    *hits = 0;
    *occluded = 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define LD_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const int np = width * height;
    const size_t cells = rect_plane(np), scan_bytes = lidar_scan_bytes(n, lidar_record_bytes(time_offset));
    const bool cull = l->occl_rel > 0.0f;
    std::vector<uint8_t> scan, fl;
    std::vector<uint16_t> p0;
    try { scan.resize(scan_bytes); fl.resize((size_t)np); p0.resize((size_t)np); } catch (const std::bad_alloc &) { return CVO_HIP_ERR_NOMEM; }
    lidar_stage(scan.data(), points, stride_bytes, n, time_offset, sw ? twist : nullptr);
    ProjectCall c;
    const bool outputs = n > 0 && (phase || moved);
    if (outputs && !dev_alloc(c.phase, (size_t)4 * n)) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    if (!dev_alloc(c.scan, scan_bytes) || !dev_alloc(c.z, cells) || !dev_alloc(c.planes, 2 * cells) || !dev_alloc(c.flags, cells)) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    uint16_t *d_p0 = c.planes.get(), *d_p = c.planes.get() + cells;
    LD_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    LD_TRY(hipMemcpyAsync(c.scan.get(), scan.data(), scan_bytes, hipMemcpyHostToDevice, c.s));
    LD_TRY(hipMemsetAsync(c.z.get(), 0xFF, cells * sizeof(uint32_t), c.s));
    if (n > 0)
        enqueue_lidar_project(*l, cam, c.scan.get(), n, c.z.get(), width, height, sw, phase ? c.phase.get() : nullptr,
                              moved ? c.phase.get() + n : nullptr, c.s);
    hipLaunchKernelGGL(k_fe_depth_final, dim3(blocks((np + 3) / 4)), dim3(FE_BLOCK), 0, c.s, c.z.get(), np, d_p0);
    if (cull) {
        FeLidarCullArgs g{};
        g.p0 = d_p0; g.p = d_p; g.flags = c.flags.get();
        g.w = width; g.h = height; g.rx = l->occl_rx; g.ry = l->occl_ry; g.occl_rel = l->occl_rel;
        fe_lidar_cull_enqueue(g, c.s);
    }
    LD_TRY(hipGetLastError());
    LD_TRY(hipMemcpyAsync(p0.data(), d_p0, (size_t)np * 2, hipMemcpyDeviceToHost, c.s));
    LD_TRY(hipMemcpyAsync(plane, cull ? d_p : d_p0, (size_t)np * 2, hipMemcpyDeviceToHost, c.s));
    if (cull) LD_TRY(hipMemcpyAsync(fl.data(), c.flags.get(), (size_t)np, hipMemcpyDeviceToHost, c.s));
    if (outputs && phase) LD_TRY(hipMemcpyAsync(phase, c.phase.get(), (size_t)n * 4, hipMemcpyDeviceToHost, c.s));
    if (outputs && moved) LD_TRY(hipMemcpyAsync(moved, c.phase.get() + n, (size_t)n * 12, hipMemcpyDeviceToHost, c.s));
    LD_TRY(hipStreamSynchronize(c.s));
#undef LD_TRY
    int nh = 0, no = 0;
    for (int i = 0; i < np; ++i) {
        if (!cull) fl[i] = p0[i] ? (uint8_t)CVO_FE_LIDAR_HIT : (uint8_t)0;
        nh += (fl[i] & CVO_FE_LIDAR_HIT) ? 1 : 0;
        no += (fl[i] & CVO_FE_LIDAR_OCCLUDED) ? 1 : 0;
    }
    if (unculled) std::memcpy(unculled, p0.data(), (size_t)np * 2);
    if (flags) std::memcpy(flags, fl.data(), (size_t)np);
    *hits = nh;
    *occluded = no;
    return CVO_HIP_OK;
}

}   // namespace

extern "C" int cvo_fe_project_points(int device, const void *points, size_t stride_bytes, int n, const cvo_fe_lidar *l,
                                     const float cam[5], int width, int height, uint16_t *plane, uint16_t *unculled,
                                     uint8_t *flags, int *hits, int *occluded)
{
    return project_points(device, points, stride_bytes, n, l, cam, width, height, plane, unculled, flags, hits, occluded,
                          nullptr, nullptr, nullptr, nullptr);
}

extern "C" int cvo_fe_project_points_sweep(int device, const void *points, size_t stride_bytes, int n, const cvo_fe_lidar *l,
                                           const float cam[5], int width, int height, uint16_t *plane, uint16_t *unculled,
                                           uint8_t *flags, int *hits, int *occluded, const cvo_fe_lidar_sweep *sw,
                                           const float twist[6], float *phase, float *moved)
{
    return project_points(device, points, stride_bytes, n, l, cam, width, height, plane, unculled, flags, hits, occluded,
                          sw, twist, phase, moved);
}
