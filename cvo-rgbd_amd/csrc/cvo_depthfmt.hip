// cvo_depthfmt.hip -- the depth-format stage of the front end on MI355X (gfx950): the device side of the depth-format
// contract of include/cvo_frontend.h (at CVO_FE_DEPTH_*).  A depth image of float32 or float16 values in the caller's
// unit becomes the uint16 plane every later stage reads.  The restatement tests/fe_depthfmt_ref.py holds the plane to
// the contract by bytes.
//
// One kernel, k_fe_depth_convert<FORMAT>, element-wise and memory-bound: one thread per four consecutive pixels of a
// row, no LDS, nothing kept between pixels.  The source is read through a pointer and a pitch in bytes, so that the
// same kernel serves the context's landing buffer and a caller's device image read in place.
//   A thread whose four pixels lie inside the row and whose source address is a multiple of 16 (F32) or 8 (F16) takes
//   them in one load; where its destination address is a multiple of 8 it stores them in one store.  Either test is
//   the thread's own address: a pitch that is no multiple of 16, a base aligned to the value size only and a width
//   that is no multiple of four each make some rows, or all, take the narrow path, value by value, and the last
//   w % 4 pixels of a row always do.  The two choices are independent.
// The arithmetic is three float32 operations per pixel, each rounded on its own (the Makefile's -ffp-contract=off;
// there is no addition to contract anyway), and comparisons that give the same answer whether or not the device
// flushes subnormals: a subnormal and the zero it may be flushed to both fail `>= 2^-126`.
#include "cvo_depthfmt.h"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_input.h"
#include "cvo_lock.h"

namespace {

constexpr int DF_BLOCK = 256;

// the contract, for one value already widened to float32
__device__ __forceinline__ uint32_t df_convert(float v, float unit, float scale)
{
    const bool ok = v >= FLT_MIN && v <= FLT_MAX;   // finite and a normal positive number (NaN fails both)
    const float t = v * unit;
    const float q = rintf(t * scale);               // ties to even
    return ok && t >= FLT_MIN && q >= 1.0f && q <= 65535.0f ? (uint32_t)q : 0u;
}

// a float16's 16 bits, widened exactly
__device__ __forceinline__ float df_half(uint32_t bits)
{
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}

template <int F> __global__ __launch_bounds__(DF_BLOCK) void k_fe_depth_convert(FeDepthConvertArgs a)
{
    constexpr size_t ITEM = F == CVO_FE_DEPTH_F32 ? 4 : 2;
    const int qw = (a.w + 3) >> 2;   // threads of a row
    const int t = (int)(blockIdx.x * DF_BLOCK + threadIdx.x);
    if (t >= qw * a.h) return;   // (at most 2048 * 8192 threads)
    const int y = t / qw, x0 = (t - y * qw) * 4;
    const int inside = min(4, a.w - x0);
    const uint8_t *src = (const uint8_t *)a.src + (size_t)y * a.src_pitch + (size_t)x0 * ITEM;
    uint16_t *dst = a.dst + (size_t)y * a.w + x0;
    float v[4];
    if (inside == 4 && ((uintptr_t)src & (4 * ITEM - 1)) == 0) {
        if constexpr (F == CVO_FE_DEPTH_F32) {
            const float4 f = *reinterpret_cast<const float4 *>(src);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
            const uint2 u = *reinterpret_cast<const uint2 *>(src);
            v[0] = df_half(u.x & 0xFFFFu); v[1] = df_half(u.x >> 16);
            v[2] = df_half(u.y & 0xFFFFu); v[3] = df_half(u.y >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.0f;   // (a pixel outside the row: not read, not stored)
            if (k < inside) {
                if constexpr (F == CVO_FE_DEPTH_F32) v[k] = reinterpret_cast<const float *>(src)[k];
                else v[k] = df_half(reinterpret_cast<const uint16_t *>(src)[k]);
            }
        }
    }
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = df_convert(v[k], a.unit, a.scale);
    if (inside == 4 && ((uintptr_t)dst & 7) == 0) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < inside) dst[k] = (uint16_t)o[k];
    }
}

template <int F> void df_launch(const FeDepthConvertArgs &a, hipStream_t s)
{
    const size_t threads = (size_t)((a.w + 3) / 4) * a.h;
    hipLaunchKernelGGL((k_fe_depth_convert<F>), dim3((unsigned)((threads + DF_BLOCK - 1) / DF_BLOCK)), dim3(DF_BLOCK), 0, s, a);
}

// the device memory and the stream of one cvo_fe_convert_depth call
struct ConvertCall {
    void *src = nullptr, *dst = nullptr;
    hipStream_t s = nullptr;
    ~ConvertCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (src) (void)hipFree(src);
        if (dst) (void)hipFree(dst);
    }
};

}   // namespace

size_t fe_depth_item(int format)
{
    return format == CVO_FE_DEPTH_U16 || format == CVO_FE_DEPTH_F16 ? 2 : format == CVO_FE_DEPTH_F32 ? 4 : 0;
}

bool fe_depth_format_ok(int format, float unit)
{
    if (fe_depth_item(format) == 0 || !std::isfinite(unit)) return false;
    if (format == CVO_FE_DEPTH_U16) return unit == 1.0f;
    return unit >= 0x1p-20f && unit <= 0x1p20f;
}

void fe_depth_convert_enqueue(const FeDepthConvertArgs &a, hipStream_t s)
{
    if (a.format == CVO_FE_DEPTH_F32) df_launch<CVO_FE_DEPTH_F32>(a, s);
    else df_launch<CVO_FE_DEPTH_F16>(a, s);   // (the caller has checked the format)
}

extern "C" int cvo_fe_check_depth_format(int format, float unit)
{
    return fe_depth_format_ok(format, unit) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

extern "C" int cvo_fe_convert_depth(int device, const void *src, size_t stride_bytes, int width, int height, int format,
                                    float unit, float scale, uint16_t *out)
{
    cvo_lock::Api api_guard;
    if (!src || !out || width < 1 || height < 1 || width > 8192 || height > 8192 || !fe_depth_format_ok(format, unit) ||
        !std::isfinite(scale) || !(scale > 0.0f))
        return CVO_HIP_ERR_INVALID;
    const size_t item = fe_depth_item(format), row = (size_t)width * item;
    size_t extent = 0;
    if (!input_stride_ok(stride_bytes, row, item) || !input_extent((size_t)height, stride_bytes, row, &extent))
        return CVO_HIP_ERR_INVALID;
    if (format == CVO_FE_DEPTH_U16) {   // (the output's own format: a copy)
        for (int y = 0; y < height; ++y)
            std::memcpy((uint8_t *)out + (size_t)y * row, (const uint8_t *)src + (size_t)y * stride_bytes, row);
        return CVO_HIP_OK;
    }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define DF_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    // the plane keeps the caller's pitch on the device, so that the kernel meets the addresses a frame's would have
    const size_t np = (size_t)width * height;
    ConvertCall c;
    if (hipMalloc(&c.src, extent) != hipSuccess || hipMalloc(&c.dst, np * 2) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    DF_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    DF_TRY(hipMemcpy2DAsync(c.src, stride_bytes, src, stride_bytes, row, (size_t)height, hipMemcpyHostToDevice, c.s));
    FeDepthConvertArgs a{};
    a.src = c.src; a.src_pitch = stride_bytes; a.dst = (uint16_t *)c.dst;
    a.w = width; a.h = height; a.format = format; a.unit = unit; a.scale = scale;
    fe_depth_convert_enqueue(a, c.s);
    DF_TRY(hipGetLastError());
    DF_TRY(hipMemcpyAsync(out, c.dst, np * 2, hipMemcpyDeviceToHost, c.s));
    DF_TRY(hipStreamSynchronize(c.s));
#undef DF_TRY
    return CVO_HIP_OK;
}
