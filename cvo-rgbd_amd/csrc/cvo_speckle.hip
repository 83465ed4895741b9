// cvo_speckle.hip -- the speckle filter of the front end on MI355X (gfx950): the device side of the speckle contract of
// include/cvo_frontend.h (at cvo_fe_speckle).  Connected components of a uint16 plane under "4-neighbours whose values
// differ by max_diff at the most", their pixel counts, and the removal of the small ones.  Everything here is integer
// arithmetic; the restatement tests/fe_speckle_ref.py holds the plane, SIZE and the count to it by bytes.
//
// A union-find by minimum: every valid pixel has a parent that is a valid pixel of its component with an index no
// larger than its own; a root is its own parent.  A parent only ever decreases (atomicMin), so the parents never
// form a cycle and every walk towards a root ends by its own progress.  No kernel waits for another lane, wave or
// block; there is no lock and no float atomic.
//   k_fe_speckle_tiles   a workgroup labels one tile of 64 x 16 pixels in LDS: a pixel starts at the first pixel of its
//                        run in the row (one ballot per row, no atomics), unions with the upper neighbour inside the
//                        tile, then every pixel's root; writes the parents (global indices: every pixel points at its
//                        tile's root), the tile's pixel count per root, zeroes the sums
//   k_fe_speckle_seams   one thread per pair of neighbours on either side of a tile border: unions in global memory
//   k_fe_speckle_count   every tile root finds its component's root and adds the tile's count to the sum there
//   k_fe_speckle_apply   every pixel finds its root, writes SIZE and, where SIZE <= max_size, goes
// What a block may read of a parent another block changes in the same launch (the seams): the value an atomicMin
// returns is the truth; a load (agent scope: past this CU's L1) may be old, and an old parent is still an ancestor of
// the same component further down the walk, which the retry of the union tolerates.  Between launches the stream's
// order makes every write visible.
#include "cvo_speckle.h"

#include "cvo_frontend.h"
#include "cvo_lock.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_TW = 64, SP_TH = 16;            // the tile
constexpr int SP_TILE = SP_TW * SP_TH;           // 1024 pixels, four per thread
constexpr int SP_PER = SP_TILE / SP_BLOCK;
constexpr uint32_t SP_NONE = 0xFFFFFFFFu;        // the parent of a pixel without a value
static_assert(SP_TILE % SP_BLOCK == 0, "every thread owns the same number of pixels of the tile");
static_assert(SP_TW == 64 && SP_BLOCK % 64 == 0, "a wave holds one row of the tile: lane = column");

// joined: both valid and |a - b| <= max_diff, the difference of signed integers
__device__ __forceinline__ bool sp_joined(int a, int b, int max_diff)
{
    return a != 0 && b != 0 && abs(a - b) <= max_diff;
}

// ---- the union-find of a tile, in LDS ---------------------------------------------------------------------------
// (LDS has no cache in front of it: a relaxed load at workgroup scope reads what the last atomic left)
__device__ __forceinline__ uint32_t sp_lds_find(uint32_t *l, uint32_t x)
{
    for (;;) {
        const uint32_t p = __hip_atomic_load(&l[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p >= x) return x;   // (a root: p == x; a parent is never larger)
        x = p;
    }
}

__device__ __forceinline__ void sp_lds_union(uint32_t *l, uint32_t a, uint32_t b)
{
    for (;;) {
        a = sp_lds_find(l, a);
        b = sp_lds_find(l, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        // a > b: a, a root when it was read, takes b as its parent -- unless it has taken another since.  Then the
        // atomic returns that parent (smaller than a) and the union goes on from there: every round a decreases.
        const uint32_t old = atomicMin(&l[a], b);
        if (old == a) return;
        a = old;
    }
}

// ---- the union-find of the plane, in global memory --------------------------------------------------------------
__device__ __forceinline__ uint32_t sp_find(uint32_t *labels, uint32_t x)
{
    for (;;) {
        const uint32_t p = __hip_atomic_load(&labels[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x) return x;   // (a root; the walk only ever moves to a smaller index: it stays inside the plane)
        x = p;
    }
}

__device__ __forceinline__ void sp_union(uint32_t *labels, uint32_t a, uint32_t b)
{
    for (;;) {
        a = sp_find(labels, a);
        b = sp_find(labels, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&labels[a], b);   // (device scope, returning: the authority)
        if (old == a) return;
        a = old;   // (old < a: a had a parent already; should b have replaced it, this round joins the two)
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_fe_speckle_tiles(const uint16_t *plane, int w, int h, int max_diff,
                                                               uint32_t *labels, uint32_t *sums, uint32_t *sizes,
                                                               uint32_t *removed)
{
    __shared__ uint16_t s_q[SP_TILE];
    __shared__ uint32_t s_l[SP_TILE], s_c[SP_TILE];
    const int tx0 = blockIdx.x * SP_TW, ty0 = blockIdx.y * SP_TH;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *removed = 0u;
    // A wave holds one row of the tile at a time (lane = column).  Inside a row nothing is united by atomics: a pixel
    // joined to its left neighbour belongs to that neighbour's run, and its first parent is the run's first pixel --
    // the highest lane at or below its own that is not joined to its left (lane 0 never is), read off one ballot.
    const int lane = threadIdx.x % SP_TW;
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int idx = threadIdx.x + k * SP_BLOCK, x = tx0 + lane, y = ty0 + (idx / SP_TW);
        const int q = (x < w && y < h) ? (int)plane[(size_t)y * w + x] : 0;
        const int left = __shfl_up(q, 1);   // (all 64 lanes are here; lane 0 gets its own value and does not use it)
        const unsigned long long runs_on = __ballot(lane > 0 && sp_joined(q, left, max_diff));
        const unsigned long long starts = ~runs_on & (~0ull >> (63 - lane));   // (the run starts at or below this lane)
        s_q[idx] = (uint16_t)q;
        s_l[idx] = q ? (uint32_t)(idx - lane + 63 - __clzll((long long)starts)) : SP_NONE;
        s_c[idx] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int idx = threadIdx.x + k * SP_BLOCK;
        if (idx >= SP_TW && sp_joined(s_q[idx], s_q[idx - SP_TW], max_diff))
            sp_lds_union(s_l, (uint32_t)idx, (uint32_t)(idx - SP_TW));
    }
    __syncthreads();
    uint32_t root[SP_PER];
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int idx = threadIdx.x + k * SP_BLOCK;
        root[k] = SP_NONE;
        if (s_q[idx]) {
            root[k] = sp_lds_find(s_l, (uint32_t)idx);
            atomicAdd(&s_c[root[k]], 1u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int idx = threadIdx.x + k * SP_BLOCK, x = tx0 + (idx % SP_TW), y = ty0 + (idx / SP_TW);
        if (x >= w || y >= h) continue;
        const size_t g = (size_t)y * w + x;
        const uint32_t r = root[k];
        // (a valid pixel's root is a valid pixel of the tile, hence inside the image)
        labels[g] = r == SP_NONE ? SP_NONE : (uint32_t)((ty0 + (int)(r / SP_TW)) * w + tx0 + (int)(r % SP_TW));
        sizes[g] = r == (uint32_t)idx ? s_c[idx] : 0u;   // the tile's count, at the tile's root
        sums[g] = 0u;
    }
}

// The pairs across the borders: first those above and below the (tiles_y - 1) horizontal borders, w each, then those
// left and right of the (tiles_x - 1) vertical ones, h each.
__global__ void __launch_bounds__(SP_BLOCK) k_fe_speckle_seams(const uint16_t *plane, int w, int h, int max_diff, int n_hor,
                                                               int n_all, uint32_t *labels)
{
    const int t = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (t >= n_all) return;
    int x, y, xn, yn;
    if (t < n_hor) {
        x = xn = t % w;
        y = (t / w + 1) * SP_TH;
        yn = y - 1;
    } else {
        const int u = t - n_hor;
        y = yn = u % h;
        x = (u / h + 1) * SP_TW;
        xn = x - 1;
    }
    const uint32_t a = (uint32_t)(y * w + x), b = (uint32_t)(yn * w + xn);
    if (sp_joined(plane[a], plane[b], max_diff)) sp_union(labels, a, b);
}

// A tile's root (the only pixels with a count) adds its tile's count to its component's root and takes that root as
// its parent, so that the last kernel reaches it in two steps.  Roots do not change in this launch.
__global__ void __launch_bounds__(SP_BLOCK) k_fe_speckle_count(int np, uint32_t *labels, const uint32_t *sizes, uint32_t *sums)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= np) return;
    const uint32_t c = sizes[i];
    if (c == 0u) return;
    const uint32_t r = sp_find(labels, (uint32_t)i);
    atomicAdd(&sums[r], c);
    if (r != (uint32_t)i) atomicMin(&labels[i], r);
}

__global__ void __launch_bounds__(SP_BLOCK) k_fe_speckle_apply(const FeSpeckleArgs a, int np)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= np) return;
    if (a.plane[i] == 0) {
        a.sizes[i] = 0u;
        return;
    }
    uint32_t x = (uint32_t)i;
    for (;;) {   // (nothing writes a parent in this launch: plain loads)
        const uint32_t p = a.labels[x];
        if (p >= x) break;
        x = p;
    }
    const uint32_t size = a.sums[x];
    a.sizes[i] = size;
    if (size <= (uint32_t)a.max_size) {
        a.plane[i] = 0;
        if (a.flags) a.flags[i] = (uint8_t)(a.flags[i] | CVO_FE_STEREO_SPECKLE);
        if (a.depth) a.depth[i] = 0;
        atomicAdd(a.removed, 1u);
    }
}

}   // namespace

void fe_speckle_enqueue(const FeSpeckleArgs &a, hipStream_t s)
{
    const int np = a.w * a.h, nb = (np + SP_BLOCK - 1) / SP_BLOCK;
    const int tiles_x = (a.w + SP_TW - 1) / SP_TW, tiles_y = (a.h + SP_TH - 1) / SP_TH;
    hipLaunchKernelGGL(k_fe_speckle_tiles, dim3(tiles_x, tiles_y), dim3(SP_BLOCK), 0, s, a.plane, a.w, a.h, a.max_diff, a.labels,
                       a.sums, a.sizes, a.removed);
    const int n_hor = (tiles_y - 1) * a.w, n_all = n_hor + (tiles_x - 1) * a.h;
    if (n_all > 0)
        hipLaunchKernelGGL(k_fe_speckle_seams, dim3((n_all + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, a.plane, a.w, a.h,
                           a.max_diff, n_hor, n_all, a.labels);
    hipLaunchKernelGGL(k_fe_speckle_count, dim3(nb), dim3(SP_BLOCK), 0, s, np, a.labels, a.sizes, a.sums);
    hipLaunchKernelGGL(k_fe_speckle_apply, dim3(nb), dim3(SP_BLOCK), 0, s, a, np);
}

extern "C" int cvo_fe_check_speckle(const cvo_fe_speckle *sp)
{
    static_assert(sizeof(cvo_fe_speckle) == 2 * sizeof(int32_t), "8 bytes, no padding");
    return sp && sp->max_size >= 1 && sp->max_size <= (1 << 26) && sp->max_diff >= 0 && sp->max_diff <= 65535 ? CVO_HIP_OK
                                                                                                                 : CVO_HIP_ERR_INVALID;
}

namespace {

// the device memory and the stream of one cvo_fe_filter_speckles call
struct SpeckleCall {
    void *plane = nullptr, *words = nullptr;
    hipStream_t s = nullptr;
    ~SpeckleCall()
    {
        if (s) (void)hipStreamDestroy(s);
        if (plane) (void)hipFree(plane);
        if (words) (void)hipFree(words);
    }
};

}   // namespace

extern "C" int cvo_fe_filter_speckles(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                                      const cvo_fe_speckle *sp, uint32_t *sizes, int *removed)
{
    cvo_lock::Api api_guard;
    if (!plane || !removed || width < 1 || height < 1 || width > 8192 || height > 8192 || stride_bytes < (size_t)width * 2 ||
        cvo_fe_check_speckle(sp) != CVO_HIP_OK)
        return CVO_HIP_ERR_INVALID;
    *removed = 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define SP_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const size_t np = (size_t)width * height, row = (size_t)width * 2;
    SpeckleCall c;
    // (labels, sums, sizes and, behind them, the count of removed pixels)
    if (hipMalloc(&c.plane, np * 2) != hipSuccess || hipMalloc(&c.words, (3 * np + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    SP_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    SP_TRY(hipMemcpy2DAsync(c.plane, row, plane, stride_bytes, row, (size_t)height, hipMemcpyHostToDevice, c.s));
    FeSpeckleArgs a{};
    a.plane = (uint16_t *)c.plane;
    a.labels = (uint32_t *)c.words; a.sums = a.labels + np; a.sizes = a.sums + np; a.removed = a.sizes + np;
    a.w = width; a.h = height; a.max_size = sp->max_size; a.max_diff = sp->max_diff;
    fe_speckle_enqueue(a, c.s);
    SP_TRY(hipGetLastError());
    uint32_t gone = 0;
    SP_TRY(hipMemcpy2DAsync(plane, stride_bytes, c.plane, row, row, (size_t)height, hipMemcpyDeviceToHost, c.s));
    if (sizes) SP_TRY(hipMemcpyAsync(sizes, a.sizes, np * 4, hipMemcpyDeviceToHost, c.s));
    SP_TRY(hipMemcpyAsync(&gone, a.removed, 4, hipMemcpyDeviceToHost, c.s));
    SP_TRY(hipStreamSynchronize(c.s));
#undef SP_TRY
    *removed = (int)gone;
    return CVO_HIP_OK;
}
