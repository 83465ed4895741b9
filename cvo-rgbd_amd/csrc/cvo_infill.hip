// cvo_infill.hip -- the infill stage of the front end on MI355X (gfx950): the device side of the infill contract of
// include/cvo_frontend.h (at cvo_fe_depth_infill).  A run of pixels without depth that is bounded on both sides, in its
// row or its column, by depths of one surface takes the values linear in INVERSE depth between them.  The values are
// integer arithmetic and the one test is one float32 multiplication and one comparison (-ffp-contract=off: nothing is
// fused); the restatement tests/fe_infill_ref.py holds the plane, the flags and the two counts to it by bytes.
//
// One kernel, k_fe_infill, one workgroup per tile of 64 x 16 pixels, 256 threads, four pixels of the tile per thread:
//   phase 1: the tile of S with a halo of hx = gap_x + 1 columns and hy = gap_y + 1 rows (0 where the pass is off) goes
//            to LDS, the corners included: the halo's rows need a row pass of their own.  The tile sits at a fixed
//            place of the plane, (16, 32), whatever the halo.  A cell outside the image holds 0: "absent" and "none"
//            are the same thing to a search, neither is an end.
//   phase 2: the row pass into a second LDS plane H, for the tile's rows (the thread's own four pixels: what it found
//            stays in registers) and for the 2 hy rows of the halo.
//   phase 3: the column pass from H for the thread's four pixels; F and the flags go to planes other than S.
// A run of L <= g pixels has its two ends within g + 1 steps of each of its pixels, and da + db = L + 1: a search of
// g + 1 steps each way for the nearest cell with a depth finds both ends or proves that the run is no candidate.  The
// step count is the same in every thread of the launch; a pixel with a depth does not search.
// The division: the quotient is at most 65535, the divisor below 2^23 (exact in float32) and the dividend below 2^39,
// so the float32 quotient is off by less than 0.01 and its floor by at most one either way; one 64-bit product and one
// comparison put it right.  No 64-bit division, no scratch.
// LDS: S 80 rows of 96 cells, H 80 rows of 64 cells, 16 bits each: 25 600 bytes, and two counters.  A wave reads 64
// consecutive cells of one row of either plane: 32 consecutive dwords, two lanes to a dword.
#include "cvo_infill.h"

#include <cmath>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_lock.h"

namespace {

constexpr int IF_BLOCK = 256;
constexpr int IF_TW = FE_INFILL_TW, IF_TH = FE_INFILL_TH;
constexpr int IF_HX = FE_INFILL_GX_MAX + 1, IF_HY = FE_INFILL_GY_MAX + 1;   // the LDS column and row of the tile's first pixel
constexpr int IF_SS = IF_TW + 2 * IF_HX;    // 96 cells per LDS row of S
constexpr int IF_ROWS = IF_TH + 2 * IF_HY;  // 80 rows
static_assert(IF_TW * IF_TH == 4 * IF_BLOCK, "four pixels of the tile per thread");
static_assert(IF_TW == 64, "a pixel's row and column in the tile are idx >> 6 and idx & 63");

// floor((2 N + Dn) / (2 Dn)) with N = A B (da + db), Dn = A da + B db: the inverse-depth interpolation, rounded half up
__host__ __device__ __forceinline__ uint32_t if_value(uint32_t A, uint32_t B, uint32_t da, uint32_t db)
{
    const uint64_t n = (uint64_t)(A * B) * (uint64_t)(da + db);   // (A B < 2^32: 65535^2 = 4294836225)
    const uint32_t dn = A * da + B * db;                          // (at most 65535 * 32)
    const uint64_t num = 2u * n + dn;
    const uint32_t den = 2u * dn;
    uint32_t q = (uint32_t)((float)num / (float)den);
    const uint64_t p = (uint64_t)q * den;
    if (p > num) --q;
    else if (num - p >= den) ++q;
    return q;
}

// the pixel at p has no depth: the value its run takes along the line of cells `stride` apart, or 0; *refused where the
// run is a candidate and the jump test refuses it.  steps = g + 1, or 0 for a pass that is off.
__device__ __forceinline__ uint32_t if_line(const uint16_t *p, int stride, int steps, float jump_rel, bool *refused)
{
    uint32_t A = 0u, B = 0u, da = 0u, db = 0u;
    for (int j = 1; j <= steps; ++j) {
        const uint32_t va = p[-j * stride], vb = p[j * stride];
        if (da == 0u && va != 0u) { da = (uint32_t)j; A = va; }
        if (db == 0u && vb != 0u) { db = (uint32_t)j; B = vb; }
    }
    *refused = false;
    if (da == 0u || db == 0u || da + db > (uint32_t)steps) return 0u;   // (L = da + db - 1 <= g)
    const uint32_t lo = min(A, B), hi = max(A, B);
    if (jump_rel > 0.0f && (float)(hi - lo) > jump_rel * (float)lo) {
        *refused = true;
        return 0u;
    }
    return if_value(A, B, da, db);
}

__global__ void __launch_bounds__(IF_BLOCK) k_fe_infill(const FeInfillArgs a)
{
    __shared__ uint16_t s_s[IF_ROWS * IF_SS];   // S: the tile and its halo
    __shared__ uint16_t s_h[IF_ROWS * IF_TW];   // H, for the tile's columns
    __shared__ uint32_t s_cnt[2];
    const int tid = (int)threadIdx.x;
    const int tx0 = blockIdx.x * IF_TW, ty0 = blockIdx.y * IF_TH;
    const int hx = a.gap_x > 0 ? a.gap_x + 1 : 0, hy = a.gap_y > 0 ? a.gap_y + 1 : 0;   // (at most IF_HX, IF_HY: cvo_fe_check_depth_infill)
    if (tid < 2) s_cnt[tid] = 0u;
    // phase 1: LDS cell (r, c) is pixel (tx0 - IF_HX + c, ty0 - IF_HY + r); rows IF_HY - hy .. IF_HY + 15 + hy, whole
    // rows (the divisor is a constant), of which the columns IF_HX - hx .. IF_HX + 63 + hx are loaded and read
    const int first = IF_HY - hy, cells = (IF_TH + 2 * hy) * IF_SS;
    for (int idx = tid; idx < cells; idx += IF_BLOCK) {
        const int rr = idx / IF_SS, c = idx - rr * IF_SS, r = first + rr;
        const int x = tx0 - IF_HX + c, y = ty0 - IF_HY + r;
        const bool inside = c >= IF_HX - hx && c < IF_HX + IF_TW + hx && x >= 0 && x < a.w && y >= 0 && y < a.h;
        s_s[r * IF_SS + c] = inside ? a.s[(size_t)y * a.w + x] : (uint16_t)0;
    }
    __syncthreads();
    // phase 2: the row pass.  The thread's own four pixels first, then the halo's rows.
    uint32_t own[4], hv[4];
    bool row_refused[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = k * IF_BLOCK + tid;
        const int r = IF_HY + (idx >> 6), c = idx & 63;
        const uint16_t *p = s_s + r * IF_SS + IF_HX + c;
        own[k] = *p;
        row_refused[k] = false;
        hv[k] = own[k] != 0u ? own[k] : if_line(p, 1, hx, a.jump_rel, &row_refused[k]);
        s_h[r * IF_TW + c] = (uint16_t)hv[k];
    }
    for (int idx = tid; idx < 2 * hy * IF_TW; idx += IF_BLOCK) {
        const int rr = idx >> 6, c = idx & 63;
        const int r = rr < hy ? IF_HY - hy + rr : IF_HY + IF_TH + (rr - hy);
        const uint16_t *p = s_s + r * IF_SS + IF_HX + c;
        const uint32_t v = *p;
        bool refused;
        s_h[r * IF_TW + c] = (uint16_t)(v != 0u ? v : if_line(p, 1, hx, a.jump_rel, &refused));
    }
    __syncthreads();
    // phase 3: the column pass, and the output
    uint32_t nrow = 0u, ncol = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = k * IF_BLOCK + tid;
        const int r = idx >> 6, c = idx & 63;
        const int x = tx0 + c, y = ty0 + r;
        if (x >= a.w || y >= a.h) continue;
        uint32_t out = hv[k], fl = 0u;
        if (out != 0u) {
            fl = own[k] != 0u ? 0u : (uint32_t)CVO_FE_INFILL_ROW;
        } else {
            bool col_refused;
            out = if_line(s_h + (IF_HY + r) * IF_TW + c, IF_TW, hy, a.jump_rel, &col_refused);
            fl = out != 0u ? (uint32_t)CVO_FE_INFILL_COL : (row_refused[k] || col_refused) ? (uint32_t)CVO_FE_INFILL_JUMP : 0u;
        }
        const size_t i = (size_t)y * a.w + x;
        a.f[i] = (uint16_t)out;
        a.flags[i] = (uint8_t)fl;
        nrow += fl == (uint32_t)CVO_FE_INFILL_ROW ? 1u : 0u;
        ncol += fl == (uint32_t)CVO_FE_INFILL_COL ? 1u : 0u;
    }
    if (a.counts) {   // (the same in every thread of the launch)
        if (nrow) atomicAdd(&s_cnt[0], nrow);
        if (ncol) atomicAdd(&s_cnt[1], ncol);
        __syncthreads();
        if (tid < 2) a.counts[2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + tid] = s_cnt[tid];
    }
}

}   // namespace

void fe_infill_enqueue(const FeInfillArgs &a, hipStream_t s)
{
    const dim3 tiles(fe_infill_tiles_x(a.w), fe_infill_tiles_y(a.h));
    hipLaunchKernelGGL(k_fe_infill, tiles, dim3(IF_BLOCK), 0, s, a);
}

extern "C" int cvo_fe_check_depth_infill(const cvo_fe_depth_infill *f)
{
    static_assert(sizeof(cvo_fe_depth_infill) == 16, "16 bytes, no padding");
    if (!f || f->pad_ != 0) return CVO_HIP_ERR_INVALID;
    if (f->gap_x < 0 || f->gap_x > FE_INFILL_GX_MAX || f->gap_y < 0 || f->gap_y > FE_INFILL_GY_MAX) return CVO_HIP_ERR_INVALID;
    return std::isfinite(f->jump_rel) && f->jump_rel >= 0.0f ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

namespace {

// the device memory and the stream of one cvo_fe_infill_plane call
struct InfillCall {
    void *planes = nullptr, *flags = nullptr, *counts = nullptr;
    hipStream_t s = nullptr;
    ~InfillCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (planes) (void)hipFree(planes);
        if (flags) (void)hipFree(flags);
        if (counts) (void)hipFree(counts);
    }
};

}   // namespace

extern "C" int cvo_fe_infill_plane(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                                   const cvo_fe_depth_infill *f, uint8_t *flags, int *row_filled, int *col_filled)
{
    cvo_lock::Api api_guard;
    if (!plane || !row_filled || !col_filled || width < 1 || height < 1 || width > 8192 || height > 8192 ||
        stride_bytes < (size_t)width * 2 || cvo_fe_check_depth_infill(f) != CVO_HIP_OK)
        return CVO_HIP_ERR_INVALID;
    *row_filled = 0;
    *col_filled = 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define IF_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const size_t np = (size_t)width * height, row = (size_t)width * 2;
    const size_t ntiles = (size_t)fe_infill_tiles_x(width) * fe_infill_tiles_y(height);
    InfillCall c;
    if (hipMalloc(&c.planes, 2 * np * 2) != hipSuccess || hipMalloc(&c.flags, np) != hipSuccess ||
        hipMalloc(&c.counts, ntiles * 2 * 4) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    std::vector<uint32_t> counts(ntiles * 2);
    IF_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    IF_TRY(hipMemcpy2DAsync(c.planes, row, plane, stride_bytes, row, (size_t)height, hipMemcpyHostToDevice, c.s));
    FeInfillArgs a{};
    a.s = (const uint16_t *)c.planes; a.f = (uint16_t *)c.planes + np;   // (F behind S: the kernel is not in place)
    a.flags = (uint8_t *)c.flags; a.counts = (uint32_t *)c.counts;
    a.w = width; a.h = height; a.gap_x = f->gap_x; a.gap_y = f->gap_y; a.jump_rel = f->jump_rel;
    fe_infill_enqueue(a, c.s);
    IF_TRY(hipGetLastError());
    IF_TRY(hipMemcpy2DAsync(plane, stride_bytes, a.f, row, row, (size_t)height, hipMemcpyDeviceToHost, c.s));
    if (flags) IF_TRY(hipMemcpyAsync(flags, a.flags, np, hipMemcpyDeviceToHost, c.s));
    IF_TRY(hipMemcpyAsync(counts.data(), a.counts, ntiles * 2 * 4, hipMemcpyDeviceToHost, c.s));
    IF_TRY(hipStreamSynchronize(c.s));
#undef IF_TRY
    uint64_t nr = 0, nc = 0;
    for (size_t t = 0; t < ntiles; ++t) { nr += counts[2 * t]; nc += counts[2 * t + 1]; }
    *row_filled = (int)nr;
    *col_filled = (int)nc;
    return CVO_HIP_OK;
}
