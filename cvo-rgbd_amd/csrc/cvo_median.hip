// cvo_median.hip -- the median stage of the front end on MI355X (gfx950): the device side of the median contract of
// include/cvo_frontend.h (at cvo_fe_depth_median).  The lower median of the valid values of a 3 x 3 or 5 x 5 window
// of a uint16 plane, in place of a valid pixel's value and, if asked for, in a hole with enough valid neighbours.
// Everything here is integer arithmetic; the restatement tests/fe_median_ref.py holds the plane, the flags and the two
// counts to it by bytes.
//
// One kernel, k_fe_median<R, FILL>, one workgroup per tile of 64 x 16 pixels, one thread per four pixels of a row:
//   phase 1: the tile of A with a halo of R pixels goes to LDS, 16-bit cells in rows of 72 (4 + 64 + 4): the tile's own
//            columns as 8-byte loads where the plane's width is a multiple of four (then every such group is aligned
//            and whole), cell by cell otherwise; the 2 R halo columns cell by cell.  A cell outside the image holds 0:
//            the contract's "absent" and its "none" are the same thing to a window, neither is a member of V.
//   phase 2: a thread reads, per window row, the twelve cells around its four pixels as three 8-byte LDS loads, and for
//            each pixel sorts the window's (2R+1)^2 keys by a fixed network, every index a compile-time constant:
//            nothing is indexed by a runtime value and nothing goes to scratch.
// The sort key is value - 1 in 32 bits: a pixel without a value becomes 0xFFFFFFFF and sorts behind every depth,
// 65535 (key 65534) included; no 16-bit sentinel.  With n valid cells the lower median is the sorted key of index
// (n - 1) >> 1, at most (2R+1)^2 / 2, picked by a chain of selects; for n == 0 that chain leaves key 0xFFFFFFFF, value 0.
// The network is Batcher's odd-even merge sort for any n, made at compile time; the comparators that only order the
// upper half never reach an output and the compiler drops them.  (The network and the pick are cvo_sortnet.h's: the
// input bin of cvo_bin.hip sorts its blocks by them as well.)
// FILL (fill_min > 0) is a template argument: without it a pixel without depth is done when its own cell is read, and
// the test against fill_min does not exist.
// LDS rows are 36 dwords apart: the sixteen threads of a row read consecutive 8-byte groups, the next row's start four
// banks to the side.
#include "cvo_median.h"

#include <utility>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_lock.h"
#include "cvo_sortnet.h"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_TW = FE_MEDIAN_TW, MD_TH = FE_MEDIAN_TH;
constexpr int MD_OFF = 4;                        // the LDS column of the tile's first pixel: 8 bytes into the row
constexpr int MD_S = MD_OFF + MD_TW + 4;         // 72 cells per LDS row
static_assert((MD_TW / 4) * MD_TH == MD_BLOCK, "one thread per four pixels of the tile");
static_assert(MD_TW % 4 == 0 && MD_S % 4 == 0 && MD_OFF % 4 == 0, "groups of four cells are 8-byte aligned in LDS");

template <int R, bool FILL>
__global__ void __launch_bounds__(MD_BLOCK) k_fe_median(const FeMedianArgs a)
{
    constexpr int ROWS = MD_TH + 2 * R, SIDE = 2 * R + 1, N = SIDE * SIDE;
    __shared__ __align__(8) uint16_t s_a[ROWS * MD_S];
    __shared__ uint32_t s_cnt[2];
    const int tid = (int)threadIdx.x;
    const int tx0 = blockIdx.x * MD_TW, ty0 = blockIdx.y * MD_TH;
    if (tid < 2) s_cnt[tid] = 0u;
    // phase 1: LDS cell (r, MD_OFF + c) is pixel (tx0 + c, ty0 - R + r).  The tile's own columns, four cells a thread:
    // x is a multiple of four, so with a width that is one the group lies inside the row and 8 bytes into the plane
    const bool wide = (a.w & 3) == 0;
#pragma unroll
    for (int k = 0; k < (ROWS * (MD_TW / 4) + MD_BLOCK - 1) / MD_BLOCK; ++k) {
        const int idx = k * MD_BLOCK + tid;
        if (idx < ROWS * (MD_TW / 4)) {
            const int r = idx / (MD_TW / 4), c = 4 * (idx % (MD_TW / 4));
            const int x = tx0 + c, y = ty0 - R + r;
            uint2 v = make_uint2(0u, 0u);
            if (y >= 0 && y < a.h && x < a.w) {
                const uint16_t *src = a.a + (size_t)y * a.w + x;
                if (wide) {
                    v = *reinterpret_cast<const uint2 *>(src);
                } else {
                    uint32_t e[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) e[q] = x + q < a.w ? (uint32_t)src[q] : 0u;
                    v = make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));
                }
            }
            *reinterpret_cast<uint2 *>(s_a + r * MD_S + MD_OFF + c) = v;
        }
    }
    // the halo's columns: R to the left of the tile, R to the right
    static_assert(ROWS * 2 * R <= MD_BLOCK, "one thread per cell of the halo's columns");
    if (tid < ROWS * 2 * R) {
        const int r = tid / (2 * R), j = tid % (2 * R);
        const int c = j < R ? j - R : MD_TW + j - R;
        const int x = tx0 + c, y = ty0 - R + r;
        uint16_t v = 0;
        if (x >= 0 && x < a.w && y >= 0 && y < a.h) v = a.a[(size_t)y * a.w + x];
        s_a[r * MD_S + MD_OFF + c] = v;
    }
    __syncthreads();
    // phase 2
    const int ry = tid / (MD_TW / 4), cx = 4 * (tid % (MD_TW / 4));
    const int x0 = tx0 + cx, y = ty0 + ry;
    uint32_t changed = 0u, filled = 0u;
    if (x0 < a.w && y < a.h) {
        // cell [dy][j] is pixel (x0 - 4 + j, y - R + dy): LDS columns cx .. cx + 11, of which the windows of the four
        // pixels reach j = 4 - R .. 7 + R (the others, at the row's two ends never written, are not looked at)
        uint32_t cell[SIDE][12];
#pragma unroll
        for (int dy = 0; dy < SIDE; ++dy) {
            const uint2 *row = reinterpret_cast<const uint2 *>(s_a + (ry + dy) * MD_S + cx);
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const uint2 p = row[g];
                cell[dy][4 * g] = p.x & 0xFFFFu; cell[dy][4 * g + 1] = p.x >> 16;
                cell[dy][4 * g + 2] = p.y & 0xFFFFu; cell[dy][4 * g + 3] = p.y >> 16;
            }
        }
        uint32_t out[4], fl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t own = cell[R][4 + k];
            uint32_t med = 0u;
            if (FILL || own != 0u) {
                uint32_t win[N];
#pragma unroll
                for (int dy = 0; dy < SIDE; ++dy)
#pragma unroll
                    for (int dx = 0; dx < SIDE; ++dx) win[dy * SIDE + dx] = cell[dy][4 + k - R + dx];
                int n;
                med = md_lower_median<N>(win, &n);
                if (FILL && own == 0u && n < a.fill_min) med = 0u;
            }
            out[k] = med;
            fl[k] = own != 0u ? (med != own ? (uint32_t)CVO_FE_MEDIAN_CHANGED : 0u) : (med != 0u ? (uint32_t)CVO_FE_MEDIAN_FILLED : 0u);
        }
        const size_t i0 = (size_t)y * a.w + x0;
        const int inside = min(4, a.w - x0);   // (a pixel of the four beyond the right border is neither stored nor counted)
        if (inside == 4 && (i0 & 3) == 0) {
            *reinterpret_cast<uint2 *>(a.b + i0) = make_uint2(out[0] | (out[1] << 16), out[2] | (out[3] << 16));
            *reinterpret_cast<uint32_t *>(a.flags + i0) = fl[0] | (fl[1] << 8) | (fl[2] << 16) | (fl[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < inside) {
                    a.b[i0 + k] = (uint16_t)out[k];
                    a.flags[i0 + k] = (uint8_t)fl[k];
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < inside) {
                changed += fl[k] == (uint32_t)CVO_FE_MEDIAN_CHANGED ? 1u : 0u;
                filled += fl[k] == (uint32_t)CVO_FE_MEDIAN_FILLED ? 1u : 0u;
            }
    }
    if (a.counts) {   // (the same in every thread of the launch)
        if (changed) atomicAdd(&s_cnt[0], changed);
        if (filled) atomicAdd(&s_cnt[1], filled);
        __syncthreads();
        if (tid < 2) a.counts[2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + tid] = s_cnt[tid];
    }
}

}   // namespace

void fe_median_enqueue(const FeMedianArgs &a, hipStream_t s)
{
    const dim3 tiles(fe_median_tiles_x(a.w), fe_median_tiles_y(a.h));
    const bool fill = a.fill_min > 0;
    if (a.radius == 1) {
        if (fill) hipLaunchKernelGGL((k_fe_median<1, true>), tiles, dim3(MD_BLOCK), 0, s, a);
        else hipLaunchKernelGGL((k_fe_median<1, false>), tiles, dim3(MD_BLOCK), 0, s, a);
    } else {   // (1 or 2: cvo_fe_check_depth_median)
        if (fill) hipLaunchKernelGGL((k_fe_median<2, true>), tiles, dim3(MD_BLOCK), 0, s, a);
        else hipLaunchKernelGGL((k_fe_median<2, false>), tiles, dim3(MD_BLOCK), 0, s, a);
    }
}

extern "C" int cvo_fe_check_depth_median(const cvo_fe_depth_median *m)
{
    static_assert(sizeof(cvo_fe_depth_median) == 3 * sizeof(int32_t), "12 bytes, no padding");
    if (!m || (m->radius != 1 && m->radius != 2) || m->pad_ != 0) return CVO_HIP_ERR_INVALID;
    const int side = 2 * m->radius + 1;
    return m->fill_min >= 0 && m->fill_min <= side * side - 1 ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

namespace {

// the device memory and the stream of one cvo_fe_median_plane call
struct MedianCall {
    void *planes = nullptr, *flags = nullptr, *counts = nullptr;
    hipStream_t s = nullptr;
    ~MedianCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (planes) (void)hipFree(planes);
        if (flags) (void)hipFree(flags);
        if (counts) (void)hipFree(counts);
    }
};

}   // namespace

extern "C" int cvo_fe_median_plane(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                                   const cvo_fe_depth_median *m, uint8_t *flags, int *changed, int *filled)
{
    cvo_lock::Api api_guard;
    if (!plane || !changed || !filled || width < 1 || height < 1 || width > 8192 || height > 8192 ||
        stride_bytes < (size_t)width * 2 || cvo_fe_check_depth_median(m) != CVO_HIP_OK)
        return CVO_HIP_ERR_INVALID;
    *changed = 0;
    *filled = 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define MD_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const size_t np = (size_t)width * height, row = (size_t)width * 2;
    const size_t plane_cells = (np + 3) & ~(size_t)3;   // (B behind A, 8 bytes into the allocation like A)
    const size_t ntiles = (size_t)fe_median_tiles_x(width) * fe_median_tiles_y(height);
    MedianCall c;
    if (hipMalloc(&c.planes, 2 * plane_cells * 2) != hipSuccess || hipMalloc(&c.flags, np) != hipSuccess ||
        hipMalloc(&c.counts, ntiles * 2 * 4) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    std::vector<uint32_t> counts(ntiles * 2);
    MD_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    MD_TRY(hipMemcpy2DAsync(c.planes, row, plane, stride_bytes, row, (size_t)height, hipMemcpyHostToDevice, c.s));
    FeMedianArgs a{};
    a.a = (const uint16_t *)c.planes; a.b = (uint16_t *)c.planes + plane_cells;
    a.flags = (uint8_t *)c.flags; a.counts = (uint32_t *)c.counts;
    a.w = width; a.h = height; a.radius = m->radius; a.fill_min = m->fill_min;
    fe_median_enqueue(a, c.s);
    MD_TRY(hipGetLastError());
    MD_TRY(hipMemcpy2DAsync(plane, stride_bytes, a.b, row, row, (size_t)height, hipMemcpyDeviceToHost, c.s));
    if (flags) MD_TRY(hipMemcpyAsync(flags, a.flags, np, hipMemcpyDeviceToHost, c.s));
    MD_TRY(hipMemcpyAsync(counts.data(), a.counts, ntiles * 2 * 4, hipMemcpyDeviceToHost, c.s));
    MD_TRY(hipStreamSynchronize(c.s));
#undef MD_TRY
    uint64_t nc = 0, nf = 0;
    for (size_t t = 0; t < ntiles; ++t) { nc += counts[2 * t]; nf += counts[2 * t + 1]; }
    *changed = (int)nc;
    *filled = (int)nf;
    return CVO_HIP_OK;
}
