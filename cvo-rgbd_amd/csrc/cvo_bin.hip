// cvo_bin.hip -- the input bin of the front end on MI355X (gfx950): the device side of the binning contract of
// include/cvo_frontend.h (at cvo_fe_binning).  The caller's images are f times the working size each way; the f x f
// box mean of the colour bytes and the lower median of the valid depths of each block make the working image.
// Everything here is integer arithmetic; the restatement tests/fe_binning_ref.py holds the planes to it by bytes.
//
// One kernel, k_fe_bin<F>, one launch per frame for all its planes: one thread per four consecutive working pixels of
// a row, blockIdx.y the plane (the left and the right image of a pair, or the colour image and the depth image).  The
// factor is a template argument: every loop over the block is unrolled, and the division by n = F * F is by a constant.
//   colour: a thread's input per input row is 12 F contiguous bytes, 12 F bytes into the row per group: whole dwords
//       where the input row starts on a dword and the group lies inside the row.  Every byte of them is picked by a
//       compile-time index into the 3 F dwords; the twelve sums become twelve bytes, stored as three dwords where the
//       output group is whole and aligned.  Input rows that do not start on a dword (an input width that is no multiple
//       of four) and the last w % 4 pixels of a row go byte by byte into the same dwords, so the arithmetic is one.
//   depth:  a thread's input per input row is 4 F values, 2 F dwords, with the same rule.  Per working pixel the n values
//       go through cvo_sortnet.h's network as 32-bit keys (value - 1: "none" is 0xFFFFFFFF and sorts last, 65535
//       included before it) and the lower median of the k valid ones is picked at (k - 1) >> 1 by a chain of selects:
//       nothing is indexed by a runtime value.  A block with k < depth_min has no depth.
// No LDS, no scratch (profiles/fe_binning_isa_resources.txt).  Neighbouring threads read neighbouring 12 F (8 F)
// bytes of each input row, so a wave's loads cover whole cache lines, each fetched once.
#include "cvo_bin.h"

#include "cvo_frontend.h"
#include "cvo_lock.h"
#include "cvo_sortnet.h"

namespace {

constexpr int BN_BLOCK = 256;

// byte I of the dwords a thread holds, I a compile-time number after unrolling
template <int N> __device__ __forceinline__ uint32_t bn_byte(const uint32_t (&d)[N], int i)
{
    return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// N dwords at p: as dwords where p is on one and all of them are `have` bytes long; else the first `have` bytes one
// by one, zeroes behind them (they belong to pixels that are not stored)
template <int N> __device__ __forceinline__ void bn_load(const uint8_t *p, int have, uint32_t (&d)[N])
{
    if (have == 4 * N && ((uintptr_t)p & 3u) == 0) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            uint32_t v = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < have) v |= (uint32_t)p[4 * i + b] << (8 * b);
            d[i] = v;
        }
    }
}

template <int F>
__global__ void __launch_bounds__(BN_BLOCK) k_fe_bin(const FeBinArgs a)
{
    constexpr int N = F * F;
    const int w = a.w, h = a.h;
    const int per_row = (w + 3) / 4;
    const size_t g = (size_t)blockIdx.x * BN_BLOCK + threadIdx.x;
    if (g >= (size_t)per_row * h) return;
    const int y = (int)(g / per_row), x0 = 4 * (int)(g % per_row);
    const int inside = min(4, w - x0);
    const size_t i0 = (size_t)y * w + x0;
    const int plane = (int)blockIdx.y;
    if (!a.is_depth[plane]) {
        const uint8_t *src = (const uint8_t *)a.src[plane];
        uint8_t *dst = (uint8_t *)a.dst[plane];
        const size_t in_row = (size_t)F * w * 3;
        uint32_t sum[4][3] = {};
#pragma unroll
        for (int j = 0; j < F; ++j) {
            uint32_t d[3 * F];
            bn_load<3 * F>(src + ((size_t)F * y + j) * in_row + (size_t)x0 * F * 3, inside * F * 3, d);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < F; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[k][c] += bn_byte(d, (k * F + i) * 3 + c);
        }
        uint32_t o[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * k + c] = (sum[k][c] + (uint32_t)(N >> 1)) / (uint32_t)N;
        if (inside == 4 && (i0 & 3) == 0) {
            uint32_t *q = reinterpret_cast<uint32_t *>(dst + 3 * i0);
#pragma unroll
            for (int t = 0; t < 3; ++t) q[t] = o[4 * t] | (o[4 * t + 1] << 8) | (o[4 * t + 2] << 16) | (o[4 * t + 3] << 24);
        } else {
#pragma unroll
            for (int t = 0; t < 12; ++t)
                if (t < 3 * inside) dst[3 * i0 + t] = (uint8_t)o[t];
        }
    } else {
        const uint8_t *src = (const uint8_t *)a.src[plane];
        uint16_t *dst = (uint16_t *)a.dst[plane];
        const size_t in_row = (size_t)F * w * 2;
        uint32_t cell[4][N];
#pragma unroll
        for (int j = 0; j < F; ++j) {
            uint32_t d[2 * F];
            bn_load<2 * F>(src + ((size_t)F * y + j) * in_row + (size_t)x0 * F * 2, inside * F * 2, d);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < F; ++i) {
                    const int e = k * F + i;   // the value's index in the row's 4 F
                    cell[k][j * F + i] = (e & 1) ? d[e >> 1] >> 16 : d[e >> 1] & 0xFFFFu;
                }
        }
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int n;
            const uint32_t med = md_lower_median<N>(cell[k], &n);
            o[k] = n >= a.depth_min ? med : 0u;
        }
        if (inside == 4 && (i0 & 3) == 0) {
            *reinterpret_cast<uint2 *>(dst + i0) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < inside) dst[i0 + k] = (uint16_t)o[k];
        }
    }
}

bool bn_factor_ok(int f) { return f >= 2 && f <= 4; }

}   // namespace

void fe_bin_enqueue(const FeBinArgs &a, hipStream_t s)
{
    const size_t work = ((size_t)((a.w + 3) / 4) * a.h + BN_BLOCK - 1) / BN_BLOCK;
    const dim3 grid((unsigned)work, (unsigned)a.planes);
    if (a.factor == 2) hipLaunchKernelGGL((k_fe_bin<2>), grid, dim3(BN_BLOCK), 0, s, a);
    else if (a.factor == 3) hipLaunchKernelGGL((k_fe_bin<3>), grid, dim3(BN_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((k_fe_bin<4>), grid, dim3(BN_BLOCK), 0, s, a);   // (2, 3 or 4: cvo_fe_check_binning)
}

extern "C" int cvo_fe_check_binning(const cvo_fe_binning *b, int width, int height)
{
    static_assert(sizeof(cvo_fe_binning) == 3 * sizeof(int32_t), "12 bytes, no padding");
    if (!b || !bn_factor_ok(b->factor) || b->pad_ != 0 || width < 1 || height < 1) return CVO_HIP_ERR_INVALID;
    if (b->depth_min < 1 || b->depth_min > b->factor * b->factor) return CVO_HIP_ERR_INVALID;
    return (long long)b->factor * width <= 8192 && (long long)b->factor * height <= 8192 ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

namespace {

// the device memory and the stream of one cvo_fe_bin_image / cvo_fe_bin_depth call
struct BinCall {
    void *in = nullptr, *out = nullptr;
    hipStream_t s = nullptr;
    ~BinCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (in) (void)hipFree(in);
        if (out) (void)hipFree(out);
    }
};

// one plane of `item` bytes per pixel (3: colour, 2: depth) through the frame's kernel
int bin_plane(int device, const void *src, size_t stride_bytes, int width, int height, const cvo_fe_binning &b, size_t item,
              void *out)
{
    const size_t in_row = (size_t)b.factor * width * item, in_rows = (size_t)b.factor * height;
    const size_t out_bytes = (size_t)width * height * item;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define BN_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    BinCall c;
    if (hipMalloc(&c.in, in_row * in_rows) != hipSuccess || hipMalloc(&c.out, out_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    BN_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    BN_TRY(hipMemcpy2DAsync(c.in, in_row, src, stride_bytes, in_row, in_rows, hipMemcpyHostToDevice, c.s));
    FeBinArgs a{};
    a.src[0] = c.in; a.dst[0] = c.out; a.is_depth[0] = item == 2 ? 1 : 0;
    a.w = width; a.h = height; a.factor = b.factor; a.depth_min = b.depth_min; a.planes = 1;
    fe_bin_enqueue(a, c.s);
    BN_TRY(hipGetLastError());
    BN_TRY(hipMemcpyAsync(out, c.out, out_bytes, hipMemcpyDeviceToHost, c.s));
    BN_TRY(hipStreamSynchronize(c.s));
#undef BN_TRY
    return CVO_HIP_OK;
}

}   // namespace

extern "C" int cvo_fe_bin_image(int device, const uint8_t *bgr, size_t stride_bytes, int width, int height, int factor,
                                uint8_t *out)
{
    cvo_lock::Api api_guard;
    const cvo_fe_binning b{factor, 1, 0};
    if (!bgr || !out || cvo_fe_check_binning(&b, width, height) != CVO_HIP_OK || stride_bytes < (size_t)factor * width * 3)
        return CVO_HIP_ERR_INVALID;
    return bin_plane(device, bgr, stride_bytes, width, height, b, 3, out);
}

extern "C" int cvo_fe_bin_depth(int device, const uint16_t *plane, size_t stride_bytes, int width, int height,
                                const cvo_fe_binning *b, uint16_t *out, int *valid)
{
    cvo_lock::Api api_guard;
    if (!plane || !out || !valid || cvo_fe_check_binning(b, width, height) != CVO_HIP_OK ||
        stride_bytes < (size_t)b->factor * width * 2)
        return CVO_HIP_ERR_INVALID;
    *valid = 0;
    const int rc = bin_plane(device, plane, stride_bytes, width, height, *b, 2, out);
    if (rc != CVO_HIP_OK) return rc;
    int n = 0;
    for (size_t i = 0; i < (size_t)width * height; ++i) n += out[i] != 0 ? 1 : 0;
    *valid = n;
    return CVO_HIP_OK;
}
