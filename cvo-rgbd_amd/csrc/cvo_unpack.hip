// cvo_unpack.hip -- the unpack stage of the front end on MI355X (gfx950): the device side of the unpack contract of
// include/cvo_frontend.h (at CVO_FE_PIXEL_*).  A colour image in the sensor's own pixel format -- RGB / BGRA / RGBA /
// grey bytes, YUY2 / UYVY / NV12, a Bayer mosaic -- becomes the dense B, G, R image every later stage reads.
// Everything here is integer arithmetic; the restatement tests/fe_unpack_ref.py holds the image to it by bytes.
//
// One kernel, k_fe_unpack<FORMAT>, one thread per four consecutive pixels of a row, blockIdx.y the image (a stereo
// pair is one launch).  The format is a template argument: the pixel loop holds no switch.
//   byte formats (RGB8 BGRA8 RGBA8 GREY8 YUY2 UYVY NV12): a thread whose four pixels lie inside the row, in a row that
//       starts on a dword of source and destination, loads whole dwords (4 B grey, 8 B YUY2 / UYVY, 4 + 4 B NV12, 12 B
//       RGB, 16 B BGRA) and stores 12 bytes as three dwords; every byte of them is picked by a compile-time index.  The
//       last w % 4 pixels of a row, and rows that do not start on a dword, go pixel by pixel.
//   Bayer: one workgroup per tile of 64 x 16 pixels.  Phase 1: the tile of the mosaic with its one-pixel halo goes to
//       LDS, byte cells in rows of 72 (4 + 64 + 4), as dword loads where the width is a multiple of four and the group
//       lies inside the row, cell by cell otherwise; a cell outside the image is the one MIRRORED about the border
//       pixel (-1 -> 1, w -> w - 2), which keeps the mosaic's phase.  Phase 2: a thread reads the 3 x 6 cells around
//       its four pixels as three dwords per row; the four kinds of site are told apart by the parity of (x, y) and the
//       format's phase through selects, no branch per pixel.
// LDS rows are 18 dwords apart: the sixteen threads of a row read consecutive dwords, the next row starts two banks on.
#include "cvo_unpack.h"

#include <cstring>

#include "cvo_frontend.h"
#include "cvo_lock.h"

namespace {

constexpr int UP_BLOCK = 256;
constexpr int UP_TW = FE_UNPACK_TW, UP_TH = FE_UNPACK_TH;
constexpr int UP_OFF = 4;                     // the LDS column of the tile's first pixel: one dword into the row
constexpr int UP_S = UP_OFF + UP_TW + 4;      // 72 cells per LDS row
constexpr int UP_ROWS = UP_TH + 2;
static_assert((UP_TW / 4) * UP_TH == UP_BLOCK, "one thread per four pixels of the tile");
static_assert(UP_S % 4 == 0 && UP_OFF % 4 == 0, "groups of four cells are dwords in LDS");

constexpr bool up_is_bayer(int f) { return f >= CVO_FE_PIXEL_BAYER_RGGB8 && f <= CVO_FE_PIXEL_BAYER_GBRG8; }
// bytes of one pixel in a row of the packed image (NV12: of its Y plane)
constexpr int up_bpp(int f)
{
    return f == CVO_FE_PIXEL_RGB8 ? 3 : (f == CVO_FE_PIXEL_BGRA8 || f == CVO_FE_PIXEL_RGBA8) ? 4
           : (f == CVO_FE_PIXEL_YUY2 || f == CVO_FE_PIXEL_UYVY) ? 2 : 1;
}
// the parities (x, y) of the mosaic's red pixel; its blue one has both the other way
constexpr int up_red_x(int f) { return (f == CVO_FE_PIXEL_BAYER_BGGR8 || f == CVO_FE_PIXEL_BAYER_GRBG8) ? 1 : 0; }
constexpr int up_red_y(int f) { return (f == CVO_FE_PIXEL_BAYER_BGGR8 || f == CVO_FE_PIXEL_BAYER_GBRG8) ? 1 : 0; }

struct UpBgr {
    uint32_t b, g, r;
};

__host__ __device__ __forceinline__ uint32_t up_sat8(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// the contract's BT.601, limited range: int32, an arithmetic shift, Y not clamped before the multiply
__host__ __device__ __forceinline__ UpBgr up_yuv(uint32_t Y, uint32_t U, uint32_t V)
{
    const int c = (int)Y - 16, d = (int)U - 128, e = (int)V - 128;
    UpBgr o;
    o.r = up_sat8((1220945 * c + 1673555 * e + 524288) >> 20);
    o.g = up_sat8((1220945 * c - 410793 * d - 852458 * e + 524288) >> 20);
    o.b = up_sat8((1220945 * c + 2115221 * d + 524288) >> 20);
    return o;
}

// byte I of the dwords a fast-path thread loaded, I a compile-time number after unrolling
template <int N> __device__ __forceinline__ uint32_t up_byte(const uint32_t (&d)[N], int i)
{
    return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

// pixel k of the four a thread makes, from the dwords of its group (NV12: d[0] four Y, d[1] two U V pairs)
template <int F, int N> __device__ __forceinline__ UpBgr up_from_dwords(const uint32_t (&d)[N], int k)
{
    UpBgr o;
    if constexpr (F == CVO_FE_PIXEL_RGB8) {
        o.r = up_byte(d, 3 * k); o.g = up_byte(d, 3 * k + 1); o.b = up_byte(d, 3 * k + 2);
    } else if constexpr (F == CVO_FE_PIXEL_BGRA8) {
        o.b = up_byte(d, 4 * k); o.g = up_byte(d, 4 * k + 1); o.r = up_byte(d, 4 * k + 2);
    } else if constexpr (F == CVO_FE_PIXEL_RGBA8) {
        o.r = up_byte(d, 4 * k); o.g = up_byte(d, 4 * k + 1); o.b = up_byte(d, 4 * k + 2);
    } else if constexpr (F == CVO_FE_PIXEL_GREY8) {
        o.b = o.g = o.r = up_byte(d, k);
    } else if constexpr (F == CVO_FE_PIXEL_YUY2) {
        const int p = 4 * (k >> 1);
        o = up_yuv(up_byte(d, p + 2 * (k & 1)), up_byte(d, p + 1), up_byte(d, p + 3));
    } else if constexpr (F == CVO_FE_PIXEL_UYVY) {
        const int p = 4 * (k >> 1);
        o = up_yuv(up_byte(d, p + 1 + 2 * (k & 1)), up_byte(d, p), up_byte(d, p + 2));
    } else {   // NV12
        o = up_yuv(up_byte(d, k), up_byte(d, 4 + 2 * (k >> 1)), up_byte(d, 5 + 2 * (k >> 1)));
    }
    return o;
}

// pixel (x, y) of a byte format by byte loads: the last w % 4 pixels of a row, and rows that do not start on a dword
template <int F> __device__ __forceinline__ UpBgr up_from_bytes(const uint8_t *src, int w, int h, int x, int y)
{
    UpBgr o;
    if constexpr (F == CVO_FE_PIXEL_NV12) {
        const uint8_t *uv = src + ((size_t)h + (size_t)(y >> 1)) * w + 2 * (x >> 1);
        o = up_yuv(src[(size_t)y * w + x], uv[0], uv[1]);
    } else if constexpr (F == CVO_FE_PIXEL_YUY2 || F == CVO_FE_PIXEL_UYVY) {
        const uint8_t *p = src + (size_t)y * w * 2 + 4 * (x >> 1);
        if constexpr (F == CVO_FE_PIXEL_YUY2) o = up_yuv(p[2 * (x & 1)], p[1], p[3]);
        else o = up_yuv(p[1 + 2 * (x & 1)], p[0], p[2]);
    } else {
        const uint8_t *p = src + ((size_t)y * w + x) * up_bpp(F);
        if constexpr (F == CVO_FE_PIXEL_GREY8) o.b = o.g = o.r = p[0];
        else if constexpr (F == CVO_FE_PIXEL_BGRA8) { o.b = p[0]; o.g = p[1]; o.r = p[2]; }
        else { o.r = p[0]; o.g = p[1]; o.b = p[2]; }   // RGB8, RGBA8
    }
    return o;
}

// the four pixels of a thread to dst at pixel index i0: three dwords where they are whole and aligned
__device__ __forceinline__ void up_store(uint8_t *dst, size_t i0, const UpBgr (&o)[4], int inside)
{
    if (inside == 4 && (i0 & 3) == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(dst + 3 * i0);
        q[0] = o[0].b | (o[0].g << 8) | (o[0].r << 16) | (o[1].b << 24);
        q[1] = o[1].g | (o[1].r << 8) | (o[2].b << 16) | (o[2].g << 24);
        q[2] = o[2].r | (o[3].b << 8) | (o[3].g << 16) | (o[3].r << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < inside) {
                dst[3 * (i0 + k)] = (uint8_t)o[k].b;
                dst[3 * (i0 + k) + 1] = (uint8_t)o[k].g;
                dst[3 * (i0 + k) + 2] = (uint8_t)o[k].r;
            }
    }
}

// a neighbour outside the image, mirrored about the border pixel (n >= 2); a cell further out than that is never
// looked at and only has to stay inside the image
__device__ __forceinline__ int up_mirror(int v, int n)
{
    const int m = v < 0 ? -v : v >= n ? 2 * (n - 1) - v : v;
    return m < 0 ? 0 : m > n - 1 ? n - 1 : m;
}

template <int F>
__global__ void __launch_bounds__(UP_BLOCK) k_fe_unpack(const FeUnpackArgs a)
{
    const int tid = (int)threadIdx.x;
    const uint8_t *src = a.src[blockIdx.y];
    uint8_t *dst = a.dst[blockIdx.y];
    const int w = a.w, h = a.h;
    if constexpr (up_is_bayer(F)) {
        __shared__ __align__(4) uint8_t s_m[UP_ROWS * UP_S];
        const int tiles_x = (w + UP_TW - 1) / UP_TW;
        const int tx0 = ((int)blockIdx.x % tiles_x) * UP_TW, ty0 = ((int)blockIdx.x / tiles_x) * UP_TH;
        // phase 1: LDS cell (r, UP_OFF + c) is pixel (tx0 + c, ty0 - 1 + r), mirrored.  The tile's own columns, four
        // cells a thread: x is a multiple of four, so with a width that is one the group is whole and on a dword
        const bool wide = (w & 3) == 0;
#pragma unroll
        for (int k = 0; k < (UP_ROWS * (UP_TW / 4) + UP_BLOCK - 1) / UP_BLOCK; ++k) {
            const int idx = k * UP_BLOCK + tid;
            if (idx < UP_ROWS * (UP_TW / 4)) {
                const int r = idx / (UP_TW / 4), c = 4 * (idx % (UP_TW / 4));
                const int x = tx0 + c, y = up_mirror(ty0 - 1 + r, h);
                const uint8_t *row = src + (size_t)y * w;
                uint32_t v;
                if (wide && x + 4 <= w) {
                    v = *reinterpret_cast<const uint32_t *>(row + x);
                } else {
                    v = 0u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v |= (uint32_t)row[up_mirror(x + q, w)] << (8 * q);
                }
                *reinterpret_cast<uint32_t *>(s_m + r * UP_S + UP_OFF + c) = v;
            }
        }
        // the halo's two columns
        if (tid < 2 * UP_ROWS) {
            const int r = tid >> 1, c = (tid & 1) ? UP_TW : -1;
            s_m[r * UP_S + UP_OFF + c] = src[(size_t)up_mirror(ty0 - 1 + r, h) * w + up_mirror(tx0 + c, w)];
        }
        __syncthreads();
        // phase 2
        const int ry = tid / (UP_TW / 4), cx = 4 * (tid % (UP_TW / 4));
        const int x0 = tx0 + cx, y = ty0 + ry;
        if (x0 >= w || y >= h) return;
        // cell [dy][j] is pixel (x0 - 1 + j, y - 1 + dy): bytes 3 .. 8 of the three dwords at LDS column cx
        uint32_t cell[3][6];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(s_m + (ry + dy) * UP_S + cx);
            const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int j = 0; j < 6; ++j) cell[dy][j] = up_byte(d, 3 + j);
        }
        const bool blue_row = ((y & 1) ^ up_red_y(F)) != 0;
        UpBgr o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t own = cell[1][k + 1];
            const uint32_t n = cell[0][k + 1], s = cell[2][k + 1], wst = cell[1][k], est = cell[1][k + 2];
            const uint32_t cross = (n + s + est + wst + 2u) >> 2;
            const uint32_t diag = (cell[0][k] + cell[0][k + 2] + cell[2][k] + cell[2][k + 2] + 2u) >> 2;
            const uint32_t horiz = (est + wst + 1u) >> 1, vert = (n + s + 1u) >> 1;
            // (x0 is a multiple of four: the column's parity is k's)
            const bool green = (((k & 1) ^ up_red_x(F)) != 0) != blue_row;
            const uint32_t of_row = green ? horiz : own, other = green ? vert : diag;
            o[k].g = green ? own : cross;
            o[k].r = blue_row ? other : of_row;
            o[k].b = blue_row ? of_row : other;
        }
        up_store(dst, (size_t)y * w + x0, o, min(4, w - x0));
    } else {
        const int per_row = (w + 3) / 4;
        const size_t g = (size_t)blockIdx.x * UP_BLOCK + tid;
        if (g >= (size_t)per_row * h) return;
        const int y = (int)(g / per_row), x0 = 4 * (int)(g % per_row);
        const int inside = min(4, w - x0);
        const size_t i0 = (size_t)y * w + x0;
        UpBgr o[4];
        // whole dwords: the group lies inside the row, and the row starts on a dword (NV12: its chroma row too)
        bool fast = inside == 4 && (i0 & 3) == 0;
        if constexpr (F == CVO_FE_PIXEL_NV12) fast = fast && ((((size_t)h + (size_t)(y >> 1)) * w) & 3) == 0;
        if (fast) {
            if constexpr (F == CVO_FE_PIXEL_NV12) {
                uint32_t d[2];
                d[0] = *reinterpret_cast<const uint32_t *>(src + i0);
                d[1] = *reinterpret_cast<const uint32_t *>(src + ((size_t)h + (size_t)(y >> 1)) * w + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = up_from_dwords<F>(d, k);
            } else {
                constexpr int N = up_bpp(F);   // dwords of four pixels
                uint32_t d[N];
                const uint32_t *p = reinterpret_cast<const uint32_t *>(src + i0 * up_bpp(F));
#pragma unroll
                for (int q = 0; q < N; ++q) d[q] = p[q];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = up_from_dwords<F>(d, k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < inside) o[k] = up_from_bytes<F>(src, w, h, x0 + k, y);
                else o[k] = UpBgr{0u, 0u, 0u};
        }
        up_store(dst, i0, o, inside);
    }
}

template <int F> void up_launch(const FeUnpackArgs &a, hipStream_t s)
{
    const size_t work = up_is_bayer(F) ? (size_t)((a.w + UP_TW - 1) / UP_TW) * ((a.h + UP_TH - 1) / UP_TH)
                                       : ((size_t)((a.w + 3) / 4) * a.h + UP_BLOCK - 1) / UP_BLOCK;
    hipLaunchKernelGGL((k_fe_unpack<F>), dim3((unsigned)work, (unsigned)a.images), dim3(UP_BLOCK), 0, s, a);
}

}   // namespace

bool fe_unpack_layout(int format, int w, int h, size_t *row_bytes, int *rows)
{
    if (format < CVO_FE_PIXEL_BGR8 || format > CVO_FE_PIXEL_BAYER_GBRG8 || w < 1 || h < 1) return false;
    if ((format == CVO_FE_PIXEL_YUY2 || format == CVO_FE_PIXEL_UYVY || format == CVO_FE_PIXEL_NV12) && (w & 1)) return false;
    if (format == CVO_FE_PIXEL_NV12 && (h & 1)) return false;
    if (up_is_bayer(format) && (w < 2 || h < 2)) return false;
    const int bpp = format == CVO_FE_PIXEL_BGR8 ? 3 : up_bpp(format);
    if (row_bytes) *row_bytes = (size_t)w * bpp;
    if (rows) *rows = format == CVO_FE_PIXEL_NV12 ? h + h / 2 : h;
    return true;
}

void fe_unpack_enqueue(const FeUnpackArgs &a, hipStream_t s)
{
    switch (a.format) {
    case CVO_FE_PIXEL_RGB8: up_launch<CVO_FE_PIXEL_RGB8>(a, s); break;
    case CVO_FE_PIXEL_BGRA8: up_launch<CVO_FE_PIXEL_BGRA8>(a, s); break;
    case CVO_FE_PIXEL_RGBA8: up_launch<CVO_FE_PIXEL_RGBA8>(a, s); break;
    case CVO_FE_PIXEL_GREY8: up_launch<CVO_FE_PIXEL_GREY8>(a, s); break;
    case CVO_FE_PIXEL_YUY2: up_launch<CVO_FE_PIXEL_YUY2>(a, s); break;
    case CVO_FE_PIXEL_UYVY: up_launch<CVO_FE_PIXEL_UYVY>(a, s); break;
    case CVO_FE_PIXEL_NV12: up_launch<CVO_FE_PIXEL_NV12>(a, s); break;
    case CVO_FE_PIXEL_BAYER_RGGB8: up_launch<CVO_FE_PIXEL_BAYER_RGGB8>(a, s); break;
    case CVO_FE_PIXEL_BAYER_BGGR8: up_launch<CVO_FE_PIXEL_BAYER_BGGR8>(a, s); break;
    case CVO_FE_PIXEL_BAYER_GRBG8: up_launch<CVO_FE_PIXEL_BAYER_GRBG8>(a, s); break;
    default: up_launch<CVO_FE_PIXEL_BAYER_GBRG8>(a, s); break;   // (the caller has checked the format)
    }
}

extern "C" int cvo_fe_check_pixel_format(int format, int width, int height)
{
    return fe_unpack_layout(format, width, height, nullptr, nullptr) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

extern "C" int cvo_fe_pixel_layout(int format, int width, int height, size_t *row_bytes, int *rows)
{
    if (!row_bytes || !rows) return CVO_HIP_ERR_INVALID;
    return fe_unpack_layout(format, width, height, row_bytes, rows) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

namespace {

// the device memory and the stream of one cvo_fe_unpack_image call
struct UnpackCall {
    void *packed = nullptr, *bgr = nullptr;
    hipStream_t s = nullptr;
    ~UnpackCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (packed) (void)hipFree(packed);
        if (bgr) (void)hipFree(bgr);
    }
};

}   // namespace

extern "C" int cvo_fe_unpack_image(int device, const uint8_t *src, size_t stride_bytes, int width, int height, int format,
                                   uint8_t *bgr)
{
    cvo_lock::Api api_guard;
    size_t row = 0;
    int rows = 0;
    if (!src || !bgr || width < 1 || height < 1 || width > 8192 || height > 8192 ||
        !fe_unpack_layout(format, width, height, &row, &rows) || stride_bytes < row)
        return CVO_HIP_ERR_INVALID;
    if (format == CVO_FE_PIXEL_BGR8) {   // (the output's own layout: a copy)
        for (int y = 0; y < rows; ++y) std::memcpy(bgr + (size_t)y * row, src + (size_t)y * stride_bytes, row);
        return CVO_HIP_OK;
    }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define UP_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const size_t np = (size_t)width * height;
    UnpackCall c;
    if (hipMalloc(&c.packed, row * (size_t)rows) != hipSuccess || hipMalloc(&c.bgr, np * 3) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    UP_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    UP_TRY(hipMemcpy2DAsync(c.packed, row, src, stride_bytes, row, (size_t)rows, hipMemcpyHostToDevice, c.s));
    FeUnpackArgs a{};
    a.src[0] = (const uint8_t *)c.packed; a.dst[0] = (uint8_t *)c.bgr;
    a.w = width; a.h = height; a.format = format; a.images = 1;
    fe_unpack_enqueue(a, c.s);
    UP_TRY(hipGetLastError());
    UP_TRY(hipMemcpyAsync(bgr, c.bgr, np * 3, hipMemcpyDeviceToHost, c.s));
    UP_TRY(hipStreamSynchronize(c.s));
#undef UP_TRY
    return CVO_HIP_OK;
}
