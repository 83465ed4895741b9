// cvo_score.hip -- gfx950 (MI355X, CDNA4) kernels of cvo_hip_pose_score (include/cvo_hip.h).
//
//   k_pose_score        : one pass over the kept list of a PROC_FLOW pass (the members of A and their float32 weights at
//                         the pose): sum a d2 per block, and a "matched" byte per fixed and per moving row of a member
//   k_pose_score_reduce : one block adds the block partials in a fixed order and counts the matched bytes
//
// d2 is recomputed from the rows exactly as the member test computed it (eval_pair: e = x - y, fma(e2, e2, fma(e1, e1,
// e0 e0)), y through apply_tf with the state's [Rt|t]), so a d2 is the bits the flow pass tested.  Every term a d2 is
// float32 (-ffp-contract=off), accumulated per lane in float64 and reduced through the same wave reduce-scatter as the
// list passes'.  The matched bytes are plain stores of 1 -- two members of one row racing store the same value -- on
// arrays the host zeroes on the stream; they are counted with integer sums.  No atomics anywhere: repeated calls give
// the same bits.
#include "cvo_device.h"

namespace cvo_dev {

// Block b, wave w streams slice 4 b + w of the kept list (kept_slice).
__global__ void __launch_bounds__(BLOCK) k_pose_score(const ScoreArgs a)
{
    __shared__ double red[4];
    if ((int)blockIdx.x >= a.kept.nblk) return;
    const int tid = threadIdx.x, lane = tid & 63;
    float Rt[9], tt[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) Rt[q] = a.kept.st->Rt[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) tt[q] = a.kept.st->t[q];
    size_t base;
    unsigned n;
    const CVO_GLOBAL char *kept_w = kept_slice(a.kept, __builtin_amdgcn_readfirstlane(tid >> 6), base, n);
    const CVO_GLOBAL char *pos_a = (const CVO_GLOBAL char *)(unsigned long long)a.pos_a;
    const CVO_GLOBAL char *pos_b = (const CVO_GLOBAL char *)(unsigned long long)a.pos_b;
    double acc[1] = {0.0};
    for (unsigned off = (unsigned)lane; off < n; off += 64u) {
        unsigned i, j;
        float w;
        kept_entry(a.kept, kept_w, base, off, i, j, w);
        if (i >= (unsigned)a.na || j >= (unsigned)a.nb) continue;   // (never: a member's rows are rows of the clouds)
        const float4 x = load_pos<false>(pos_a, i * 16u);
        const float4 y = apply_tf(Rt, tt, load_pos<false>(pos_b, j * 16u));
        const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z;
        const float d2 = __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0));
        acc[0] += (double)(w * d2);
        a.flag_a[i] = 1;
        a.flag_b[j] = 1;
    }
    const double sum = block_sums<1>(acc, red);
    if (tid == 0) a.partials[blockIdx.x] = sum;
}

// the matched bytes of words tid, tid + BLOCK, ... of a flag array (every byte is 0 or 1: the byte sum of a word is
// the top byte of its product with 0x01010101)
__device__ __forceinline__ unsigned count_flags(const uint8_t *flags, int nbytes, int tid)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(flags);
    unsigned c = 0;
    for (int q = tid; q < nbytes / 4; q += BLOCK) c += (w[q] * 0x01010101u) >> 24;
    return c;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}

__global__ void __launch_bounds__(BLOCK) k_pose_score_reduce(const ScoreArgs a)
{
    __shared__ double red[4];
    __shared__ unsigned cnt[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned ca = wave_sum_u32(count_flags(a.flag_a, a.na, tid));
    const unsigned cb = wave_sum_u32(count_flags(a.flag_b, a.nb, tid));
    if (lane == 0) {
        cnt[0][wid] = ca;
        cnt[1][wid] = cb;
    }
    const double sum = block_partials_sum<1>(a.partials, a.kept.nblk, red);   // (its barrier: the counts are in place)
    if (tid == 0) {
        a.out[0] = sum;
        a.out[1] = (double)(cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3]);
        a.out[2] = (double)(cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3]);
    }
}

void launch_pose_score(const ScoreArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_score, dim3((unsigned)a.kept.nblk), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_pose_score_reduce, dim3(1), dim3(BLOCK), 0, s, a);
}

}   // namespace cvo_dev
