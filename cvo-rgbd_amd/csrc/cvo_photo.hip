// cvo_photo.hip -- the photometric stage of the front end on MI355X (gfx950): the device side of the photometric
// contract of include/cvo_frontend.h (at cvo_fe_photometric).  A response table per channel, a vignette gain per pixel
// and a gain per channel and frame correct the B G R bytes in place, at the input size, in front of the bin and of
// everything else.  Everything here is unsigned integer arithmetic; the restatement tests/fe_photometric_ref.py holds
// the image to it by bytes and the frame's record by value.
//
// k_fe_photo_apply<FLAGS> (FLAGS: CVO_FE_PHOTO_RESPONSE | CVO_FE_PHOTO_VIGNETTE, what the instance reads): one launch
//     for both images of a pair (blockIdx.y), one thread per four consecutive pixels of the dense image: three whole
//     dwords in and out, the vignette's four gains as one 8-byte load.  The response table sits in LDS (1 536 bytes,
//     filled once per block, 384 dwords).  The three gains are read from memory -- the frame's header, or under AUTO
//     what k_fe_photo_gain left -- so a captured launch holds no gain.  The last np % 4 pixels are assembled byte by
//     byte into the same dwords, so the arithmetic exists once (ph_values).
// k_fe_photo_stat<FLAGS> (AUTO): the same loads on the left image, at most 2048 blocks whose threads loop; k and M_c
//     summed per thread in 32 bits (2^27 at most), per wave by shuffles and per block through LDS in 64 bits, then one
//     64-bit atomicAdd per block and word, the blocks dealt over 32 slots of accumulators a cache line apart.  Integer
//     sums are exact in any order.
// k_fe_photo_gain (AUTO): one wave that sums the slots, then one thread; a launch of its own between the two (no ticket among the blocks of the stat: a
//     launch boundary is the only ordering the three kernels need, and it costs the stage one more node).  It forms the
//     gains and the lock, writes the record, and leaves the accumulators zero for the next replay.
// No scratch (profiles/fe_photometric_isa_resources.txt).
#include "cvo_photo.h"

#include <cmath>

#include "cvo_lock.h"

namespace {

constexpr int PH_BLOCK = 256;
constexpr unsigned PH_STAT_BLOCKS = 2048;   // of k_fe_photo_stat at the most: eight per CU, each thread then loops
constexpr int PH_TABLES = CVO_FE_PHOTO_RESPONSE | CVO_FE_PHOTO_VIGNETTE;

// the response table into LDS: 384 dwords, every thread of the block arrives
template <int FLAGS> __device__ __forceinline__ void ph_fill(uint32_t *lut, const uint16_t *response)
{
    if (FLAGS & CVO_FE_PHOTO_RESPONSE) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(response);
        for (int i = (int)threadIdx.x; i < 384; i += PH_BLOCK) lut[i] = q[i];
        __syncthreads();
    }
}

// A = L * V of the twelve bytes of group g (pixels 4 g .. 4 g + inside - 1); d: the bytes as they lie, zero behind them
template <int FLAGS>
__device__ __forceinline__ void ph_values(const uint8_t *img, const uint16_t *vig, const uint32_t *lut, size_t g, int inside,
                                          uint32_t (&d)[3], uint32_t (&A)[12])
{
    const uint8_t *p = img + 12 * g;
    uint32_t v[4];
    if (inside == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            uint32_t x = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < 3 * inside) x |= (uint32_t)p[4 * i + b] << (8 * b);
            d[i] = x;
        }
    }
    if (FLAGS & CVO_FE_PHOTO_VIGNETTE) {
        if (inside == 4) {
            const uint2 t = *reinterpret_cast<const uint2 *>(vig + 4 * g);
            v[0] = t.x & 0xFFFFu; v[1] = t.x >> 16; v[2] = t.y & 0xFFFFu; v[3] = t.y >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < inside ? (uint32_t)vig[4 * g + k] : 0u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 4096u;
    }
    const uint16_t *lut16 = reinterpret_cast<const uint16_t *>(lut);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint32_t b = (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const uint32_t L = (FLAGS & CVO_FE_PHOTO_RESPONSE) ? (uint32_t)lut16[(i % 3) * 256 + b] : b << 8;
        A[i] = L * v[i / 3];
    }
}

template <int FLAGS>
__global__ void __launch_bounds__(PH_BLOCK) k_fe_photo_apply(const FePhotoArgs a, const uint32_t *gains)
{
    __shared__ uint32_t lut[384];
    ph_fill<FLAGS>(lut, a.response);
    const size_t np = (size_t)a.w * a.h, groups = (np + 3) / 4;
    const size_t g = (size_t)blockIdx.x * PH_BLOCK + threadIdx.x;
    if (g >= groups) return;   // (behind the block's only barrier)
    const int inside = np - 4 * g < 4 ? (int)(np - 4 * g) : 4;
    uint8_t *img = a.img[blockIdx.y];
    const uint32_t G[3] = {gains[0], gains[1], gains[2]};
    uint32_t d[3], A[12], o[12];
    ph_values<FLAGS>(img, a.vignette, lut, g, inside, d, A);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint64_t q = ((uint64_t)A[i] * G[i % 3] + 0x80000000ull) >> 32;
        o[i] = q > 255u ? 255u : (uint32_t)q;
    }
    uint8_t *p = img + 12 * g;
    if (inside == 4) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
        for (int t = 0; t < 3; ++t) q[t] = o[4 * t] | (o[4 * t + 1] << 8) | (o[4 * t + 2] << 16) | (o[4 * t + 3] << 24);
    } else {
#pragma unroll
        for (int t = 0; t < 12; ++t)
            if (t < 3 * inside) p[t] = (uint8_t)o[t];
    }
}

template <int FLAGS>
__global__ void __launch_bounds__(PH_BLOCK) k_fe_photo_stat(const FePhotoArgs a)
{
    __shared__ uint32_t lut[384];
    __shared__ unsigned long long part[PH_BLOCK / 64][4];
    ph_fill<FLAGS>(lut, a.response);
    const size_t np = (size_t)a.w * a.h, groups = (np + 3) / 4;
    const uint32_t lo = (uint32_t)a.set.lo, hi = (uint32_t)a.set.hi;
    // k, M_0, M_1, M_2 of this thread's pixels: at most 2^24 groups over at least PH_STAT_BLOCKS * 256 = 2^19 threads
    // where the grid is capped, 32 groups of 4 * 2^20 a thread, 2^27
    uint32_t sum[4] = {0u, 0u, 0u, 0u};
    for (size_t g = (size_t)blockIdx.x * PH_BLOCK + threadIdx.x; g < groups; g += (size_t)gridDim.x * PH_BLOCK) {
        const int inside = np - 4 * g < 4 ? (int)(np - 4 * g) : 4;
        uint32_t d[3], A[12];
        ph_values<FLAGS>(a.img[0], a.vignette, lut, g, inside, d, A);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool in = k < inside;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * k + c;
                const uint32_t b = (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                in = in && b >= lo && b <= hi;
            }
            if (in) {
                sum[0] += 1u;
#pragma unroll
                for (int c = 0; c < 3; ++c) sum[1 + c] += A[3 * k + c] >> 12;
            }
        }
    }
    // (a wave's sum may pass 32 bits: 64 bits from here on)
    unsigned long long wide[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        wide[t] = sum[t];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wide[t] += __shfl_down(wide[t], off, 64);
    }
    const int wave = (int)threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) part[wave][t] = wide[t];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0ull;
#pragma unroll
        for (int v = 0; v < PH_BLOCK / 64; ++v) s += part[v][threadIdx.x];
        // (the blocks are dealt over the slots, each on a cache line of its own: adds to one address queue up behind
        // one another, some eight thousand blocks of a 3840 x 2160 image on four words took 103 us)
        if (s) atomicAdd(&a.state->acc[blockIdx.x % FE_PHOTO_SLOTS][threadIdx.x], s);
    }
}

__device__ __forceinline__ uint32_t ph_gain(uint64_t T, uint64_t k, uint64_t M, const cvo_fe_photometric &set)
{
    const uint64_t q = (T * k * 4096ull + (M >> 1)) / M;
    const uint64_t lo = (uint64_t)set.gain_min, hi = (uint64_t)set.gain_max;
    return (uint32_t)(q < lo ? lo : q > hi ? hi : q);
}

__global__ void k_fe_photo_gain(FePhotoState *st, const FePhotoHeader *hdr, const cvo_fe_photometric set)
{
    // one wave: lane l takes slot l's four words and leaves them zero (the next frame, or the next replay, starts from
    // zero); lane 0 has their sums and does the rest alone
    unsigned long long word[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        word[t] = threadIdx.x < FE_PHOTO_SLOTS ? st->acc[threadIdx.x][t] : 0ull;
        if (threadIdx.x < FE_PHOTO_SLOTS) st->acc[threadIdx.x][t] = 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) word[t] += __shfl_down(word[t], off, 64);
    }
    if (threadIdx.x != 0) return;
    const uint64_t k = word[0], M[3] = {word[1], word[2], word[3]};
    const bool use_lock = (set.target[0] | set.target[1] | set.target[2]) == 0u;
    uint32_t locked = hdr->rearm ? 0u : st->locked;
    uint32_t T[3], G[3] = {4096u, 4096u, 4096u}, flags = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) T[c] = use_lock ? (locked ? st->T[c] : 0u) : set.target[c];
    if (k < (uint64_t)set.min_count) flags = CVO_FE_PHOTO_FALLBACK;
    else if (use_lock && !locked) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[c] = (uint32_t)((M[c] + (k >> 1)) / k);
        locked = 1u;
        flags = CVO_FE_PHOTO_LOCKED;
    } else if (set.per_channel) {
        if (M[0] == 0ull || M[1] == 0ull || M[2] == 0ull) flags = CVO_FE_PHOTO_FALLBACK;
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) G[c] = ph_gain(T[c], k, M[c], set);
        }
    } else {
        const uint64_t Ms = M[0] + M[1] + M[2], Ts = (uint64_t)T[0] + T[1] + T[2];
        if (Ms == 0ull) flags = CVO_FE_PHOTO_FALLBACK;
        else G[0] = G[1] = G[2] = ph_gain(Ts, k, Ms, set);
    }
    cvo_fe_photometric_frame r;
    for (int c = 0; c < 3; ++c) {
        st->G[c] = G[c];
        st->T[c] = use_lock && locked ? T[c] : 0u;
        r.gain[c] = G[c];
        r.sum[c] = M[c];
        r.target[c] = use_lock && !locked ? 0u : T[c];
    }
    st->locked = locked;
    r.flags = flags;
    r.count = k;
    r.pad_ = 0u;
    st->rec = r;
}

template <int FLAGS> void ph_launch(const FePhotoArgs &a, hipStream_t s)
{
    const size_t np = (size_t)a.w * a.h;
    const unsigned blocks = (unsigned)(((np + 3) / 4 + PH_BLOCK - 1) / PH_BLOCK);
    const bool automatic = (a.set.flags & CVO_FE_PHOTO_AUTO) != 0;
    if (automatic) {
        hipLaunchKernelGGL((k_fe_photo_stat<FLAGS>), dim3(blocks < PH_STAT_BLOCKS ? blocks : PH_STAT_BLOCKS), dim3(PH_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_fe_photo_gain, dim3(1), dim3(64), 0, s, a.state, a.hdr, a.set);
    }
    hipLaunchKernelGGL((k_fe_photo_apply<FLAGS>), dim3(blocks, (unsigned)a.images), dim3(PH_BLOCK), 0, s, a,
                       automatic ? (const uint32_t *)a.state->G : (const uint32_t *)a.hdr->gain);
}

}   // namespace

void fe_photo_enqueue(const FePhotoArgs &a, hipStream_t s)
{
    switch (a.set.flags & PH_TABLES) {
    case 0: ph_launch<0>(a, s); break;
    case CVO_FE_PHOTO_RESPONSE: ph_launch<CVO_FE_PHOTO_RESPONSE>(a, s); break;
    case CVO_FE_PHOTO_VIGNETTE: ph_launch<CVO_FE_PHOTO_VIGNETTE>(a, s); break;
    default: ph_launch<PH_TABLES>(a, s); break;
    }
}

void fe_photo_header(const cvo_fe_photometric &set, const uint32_t gains_q12[3], bool rearm, FePhotoHeader *out)
{
    for (int c = 0; c < 3; ++c) {
        uint32_t g = 4096u;
        if ((set.flags & CVO_FE_PHOTO_GAIN) && gains_q12) {
            g = gains_q12[c];
            if (g < (uint32_t)set.gain_min) g = (uint32_t)set.gain_min;
            if (g > (uint32_t)set.gain_max) g = (uint32_t)set.gain_max;
        }
        out->gain[c] = g;
    }
    out->rearm = rearm ? 1u : 0u;
}

void fe_photo_plain_record(const FePhotoHeader &hdr, cvo_fe_photometric_frame *out)
{
    *out = cvo_fe_photometric_frame{};
    for (int c = 0; c < 3; ++c) out->gain[c] = hdr.gain[c];
}

extern "C" int cvo_fe_check_photometric(const cvo_fe_photometric *p, int have_response, int have_vignette)
{
    static_assert(sizeof(cvo_fe_photometric) == 11 * sizeof(int32_t), "44 bytes, no padding");
    static_assert(sizeof(cvo_fe_photometric_frame) == 64, "64 bytes, no padding");
    if (!p || p->flags == 0u || p->flags > 15u || p->pad_ != 0) return CVO_HIP_ERR_INVALID;
    if ((p->flags & CVO_FE_PHOTO_GAIN) && (p->flags & CVO_FE_PHOTO_AUTO)) return CVO_HIP_ERR_INVALID;
    if (p->lo < 0 || p->lo > p->hi || p->hi > 255 || p->min_count < 1) return CVO_HIP_ERR_INVALID;
    if (p->per_channel != 0 && p->per_channel != 1) return CVO_HIP_ERR_INVALID;
    for (uint32_t t : p->target)
        if (t > 65535u) return CVO_HIP_ERR_INVALID;
    if (p->gain_min < 1 || p->gain_min > p->gain_max || p->gain_max > 65535) return CVO_HIP_ERR_INVALID;
    if ((have_response != 0) != ((p->flags & CVO_FE_PHOTO_RESPONSE) != 0)) return CVO_HIP_ERR_INVALID;
    if ((have_vignette != 0) != ((p->flags & CVO_FE_PHOTO_VIGNETTE) != 0)) return CVO_HIP_ERR_INVALID;
    return CVO_HIP_OK;
}

extern "C" int cvo_fe_response_table(const float inv[256], uint16_t out[256])
{
    if (!inv || !out) return CVO_HIP_ERR_INVALID;
    for (int i = 0; i < 256; ++i)
        if (!std::isfinite(inv[i]) || inv[i] < 0.0f || inv[i] > 255.0f) return CVO_HIP_ERR_INVALID;
    for (int i = 0; i < 256; ++i) {
        const float scaled = inv[i] * 256.0f;
        const uint32_t v = (uint32_t)(scaled + 0.5f);
        out[i] = (uint16_t)(v > 65535u ? 65535u : v);
    }
    return CVO_HIP_OK;
}

extern "C" int cvo_fe_vignette_gains(const uint16_t *atten, size_t n, uint16_t *out)
{
    if (n > 0 && (!atten || !out)) return CVO_HIP_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t a = atten[i];
        const uint32_t g = a ? (4096u * 65535u + a / 2u) / a : 65535u;
        out[i] = (uint16_t)(g > 65535u ? 65535u : g);
    }
    return CVO_HIP_OK;
}

namespace {

// the device memory and the stream of one cvo_fe_photometric_image call
struct PhotoCall {
    void *img = nullptr, *resp = nullptr, *vig = nullptr, *hdr = nullptr, *state = nullptr;
    hipStream_t s = nullptr;
    ~PhotoCall()
    {
        if (s) (void)hipStreamDestroy(s);
        for (void *p : {img, resp, vig, hdr, state})
            if (p) (void)hipFree(p);
    }
};

}   // namespace

extern "C" int cvo_fe_photometric_image(int device, const uint8_t *bgr, int width, int height, size_t stride,
                                        const cvo_fe_photometric *settings, const uint16_t *response, const uint16_t *vignette,
                                        size_t vignette_stride, const uint32_t gains_q12[3], uint8_t *out,
                                        cvo_fe_photometric_frame *frame_out)
{
    cvo_lock::Api api_guard;
    if (!bgr || !out || width < 1 || width > 8192 || height < 1 || height > 8192 || stride < (size_t)width * 3)
        return CVO_HIP_ERR_INVALID;
    if (cvo_fe_check_photometric(settings, response != nullptr, vignette != nullptr) != CVO_HIP_OK) return CVO_HIP_ERR_INVALID;
    if (vignette && (vignette_stride < (size_t)width * 2 || vignette_stride % 2 != 0)) return CVO_HIP_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_NODEVICE; }
#define PH_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return CVO_HIP_ERR_HIP; } } while (0)
    const size_t np = (size_t)width * height, row = (size_t)width * 3;
    PhotoCall c;
    if (hipMalloc(&c.img, np * 3) != hipSuccess || hipMalloc(&c.hdr, sizeof(FePhotoHeader)) != hipSuccess ||
        hipMalloc(&c.state, sizeof(FePhotoState)) != hipSuccess || (response && hipMalloc(&c.resp, 768 * 2) != hipSuccess) ||
        (vignette && hipMalloc(&c.vig, np * 2) != hipSuccess)) {
        (void)hipGetLastError();
        return CVO_HIP_ERR_NOMEM;
    }
    FePhotoHeader hdr;
    fe_photo_header(*settings, gains_q12, false, &hdr);
    PH_TRY(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
    // (dense rows go in one copy: a pitched copy of 8192 rows of one pixel takes milliseconds)
    if (stride == row) PH_TRY(hipMemcpyAsync(c.img, bgr, np * 3, hipMemcpyHostToDevice, c.s));
    else PH_TRY(hipMemcpy2DAsync(c.img, row, bgr, stride, row, (size_t)height, hipMemcpyHostToDevice, c.s));
    if (response) PH_TRY(hipMemcpyAsync(c.resp, response, 768 * 2, hipMemcpyHostToDevice, c.s));
    if (vignette && vignette_stride == (size_t)width * 2) PH_TRY(hipMemcpyAsync(c.vig, vignette, np * 2, hipMemcpyHostToDevice, c.s));
    else if (vignette)
        PH_TRY(hipMemcpy2DAsync(c.vig, (size_t)width * 2, vignette, vignette_stride, (size_t)width * 2, (size_t)height,
                                hipMemcpyHostToDevice, c.s));
    PH_TRY(hipMemcpyAsync(c.hdr, &hdr, sizeof(hdr), hipMemcpyHostToDevice, c.s));
    PH_TRY(hipMemsetAsync(c.state, 0, sizeof(FePhotoState), c.s));   // (a first frame: the lock open, the sums zero)
    FePhotoArgs a{};
    a.img[0] = (uint8_t *)c.img; a.images = 1; a.w = width; a.h = height;
    a.response = (const uint16_t *)c.resp; a.vignette = (const uint16_t *)c.vig;
    a.hdr = (const FePhotoHeader *)c.hdr; a.state = (FePhotoState *)c.state; a.set = *settings;
    fe_photo_enqueue(a, c.s);
    PH_TRY(hipGetLastError());
    PH_TRY(hipMemcpyAsync(out, c.img, np * 3, hipMemcpyDeviceToHost, c.s));
    cvo_fe_photometric_frame rec;
    fe_photo_plain_record(hdr, &rec);
    if (settings->flags & CVO_FE_PHOTO_AUTO)
        PH_TRY(hipMemcpyAsync(&rec, &((FePhotoState *)c.state)->rec, sizeof(rec), hipMemcpyDeviceToHost, c.s));
    PH_TRY(hipStreamSynchronize(c.s));
#undef PH_TRY
    if (frame_out) *frame_out = rec;
    return CVO_HIP_OK;
}
