// cvo_scan.hip -- gfx950 (MI355X, CDNA4) kernels of cvo_hip_pose_scan (include/cvo_hip.h): the CVO inner product of ONE
// pair of clouds at MANY candidate poses, without tile lists, kept lists or the host between the poses.
//
//   k_pose_scan        : grid (blocks of four fixed segments) x (poses).  A wave owns one segment of SEG = 64 fixed rows,
//                        lane = row, the row's position and features in registers.  It walks the moving cloud's segments
//                        in device order; a segment whose bounding sphere, moved with the pose, is out of reach of the
//                        wave's own is skipped, the others are transformed once per BLOCK into LDS and tested row by
//                        row.  Per lane: sum a, sum a d2 (float64), members.
//   k_pose_scan_reduce : a thread per pose adds the pose's block sums in block order.
//
// The member rule and the weights are the flow pass's, bit for bit: y = apply_tf(Rt, t, z), e = x - y,
// d2 = fma(e2, e2, fma(e1, e1, e0 e0)), member iff d2 < kc.tau and pair_weight<WEIGHT>(...) > 0 (cvo_pair.h; the same
// build flags).  A term is the float32 a, resp. the float32 product a d2 as k_pose_score forms it.
//
// Order of the sums.  A lane adds its row's members in ascending device row of the moving cloud; the 64 lanes are joined
// by wave_sums, the four waves of a block in wave order, the blocks of a pose in block order.  Culling removes only pairs
// that are not members, and a pair that is not a member adds nothing, so the sums of a pose are a function of the two
// device clouds, the constants and the pose alone -- not of the other poses of the launch, their number or their order.
// No atomics.
#include "cvo_device.h"
#include "cvo_pair.h"

namespace cvo_dev {

// Culling.  A wave skips moving segment s iff
//     |c_x - c_y'| - r_x - scale r_y > reach          (all float32, c_y' = apply_tf(Rt, t, c_y))
// with (c_x, r_x), (c_y, r_y) the segments' spheres (cvo_cloud.hip k_cloud_seg: every real row of the segment lies within
// r of c, r already rounded up), scale >= |Rt|_2 and reach = sqrt(tau) + slack, both made per pose by the host
// (cvo_pose.cpp scan_pose_consts, where the slack is derived).  A member (i, j) has a computed d2 < tau, hence
// |x_i - y^_j| < sqrt(tau) (1 + 4 u) for the computed row y^_j, and
//     |c_x - c_y*| <= |c_x - x_i| + |x_i - y^_j| + |y^_j - y_j*| + |y_j* - c_y*| <= r_x + sqrt(tau)(1 + 4 u) + err + |Rt|_2 r_y
// (* = in exact arithmetic); the slack covers err, the rounding of c_y' and of the left-hand side.  So a skipped
// segment holds no member of any row of the wave.
__device__ __forceinline__ bool scan_near(const float4 sx, const float4 cy, const float ry, const float scale, const float reach)
{
    const float dx = sx.x - cy.x, dy = sx.y - cy.y, dz = sx.z - cy.z;
    const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
    return !((dist - sx.w) - scale * ry > reach);   // (a NaN keeps the segment: the exact test decides)
}

template <int WEIGHT>
__global__ void __launch_bounds__(BLOCK) k_pose_scan(const ScanArgs a)
{
    __shared__ float4 s_pos[2][SEG];      // the staged segment's transformed rows (x, y, z, f4), double-buffered
    __shared__ float4 s_feat[2][SEG];     // ... and their features f0..f3
    __shared__ double s_etab_all[4][64];  // exp_neg's table, a copy per wave
    __shared__ unsigned long long s_mask[4];
    __shared__ double s_red[4][3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.y;
    const int sa = (int)blockIdx.x * 4 + wid;
    const bool have = sa < a.nseg_a;      // (the last block of a pose may own fewer than four segments)
    s_etab_all[wid][lane] = c_exp2_64[lane];
    const double *etab = s_etab_all[wid];
    const float *tf = a.tf + (size_t)k * SCAN_TF;
    float Rt[9], tt[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) Rt[q] = tf[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) tt[q] = tf[9 + q];
    const float scale = tf[12], reach = tf[13];
    const KernConsts &kc = a.kc;
    const int row = (have ? sa : 0) * SEG + lane;
    const float4 x = a.pos_a[row];
    const float4 fa0 = *reinterpret_cast<const float4 *>(a.feat_a + (size_t)row * FEAT_STRIDE);
    const float fa4 = x.w;   // the 5th feature travels in pos.w
    const float4 sx = a.seg_a[have ? sa : 0];
    double sum_a = 0.0, sum_ad2 = 0.0;
    unsigned members = 0;
    for (int base = 0; base < a.nseg_b; base += 64) {
        // lane l judges moving segment base + l for this wave
        bool near = false;
        if (have && base + lane < a.nseg_b) {
            const float4 sy = a.seg_b[base + lane];
            near = scan_near(sx, apply_tf(Rt, tt, sy), sy.w, scale, reach);
        }
        const unsigned long long mine = __ballot(near);
        if (lane == 0) s_mask[wid] = mine;
        __syncthreads();
        unsigned long long todo = (s_mask[0] | s_mask[1]) | (s_mask[2] | s_mask[3]);   // segments some wave of the block needs
        int buf = 0;
        while (todo) {
            const int s = __builtin_ctzll(todo);
            todo &= todo - 1;
            // staged once per block: the first wave moves the rows, the second copies the features.  (Buffer `buf` was read
            // last before the barrier of the previous segment: every wave is past that.)
            const int jrow = (base + s) * SEG + lane;
            if (wid == 0) s_pos[buf][lane] = apply_tf(Rt, tt, a.pos_b[jrow]);
            else if (wid == 1) s_feat[buf][lane] = *reinterpret_cast<const float4 *>(a.feat_b + (size_t)jrow * FEAT_STRIDE);
            __syncthreads();
            if ((mine >> s) & 1ull) {
                const float4 *sp = s_pos[buf];
                // which of the 64 rows pass d2 < tau (broadcast reads, no divergence) ...
                unsigned long long hit = 0;
#pragma unroll 8
                for (int j = 0; j < SEG; ++j) {
                    const float4 y = sp[j];
                    const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z;
                    const float d2 = __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0));
                    hit |= (d2 < kc.tau) ? (1ull << j) : 0ull;
                }
                // ... then their weights, every lane its own rows in ascending order: the wave makes as many trips as its
                // busiest lane has rows, not one per row that any lane passed
                while (hit) {
                    const int j = __builtin_ctzll(hit);
                    hit &= hit - 1;
                    const float4 y = sp[j];
                    const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z;
                    const float d2 = __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0));
                    const float w = pair_weight<WEIGHT>(kc, d2, fa0, fa4, s_feat[buf][j], y.w, etab);
                    if (w > 0.0f) {   // (a NaN -- a padding row's features -- is no member)
                        sum_a += (double)w;
                        sum_ad2 += (double)(w * d2);
                        ++members;
                    }
                }
            }
            buf ^= 1;
        }
        __syncthreads();   // (s_mask and both buffers are free again)
    }
    double acc[3] = {sum_a, sum_ad2, (double)members};
    wave_sums<3>(acc, lane, s_red[wid]);
    __syncthreads();
    if (tid < 3) {
        const size_t at = ((size_t)tid * a.nblk + blockIdx.x) * (size_t)a.count + (size_t)k;
        a.partials[at] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

__global__ void __launch_bounds__(BLOCK) k_pose_scan_reduce(const ScanArgs a)
{
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= a.count) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double *p = a.partials + (size_t)q * a.nblk * (size_t)a.count + (size_t)k;
        double s = 0.0;
        for (int b = 0; b < a.nblk; ++b) s += p[(size_t)b * a.count];
        a.out[(size_t)k * 3 + q] = s;
    }
}

void launch_pose_scan(const ScanArgs &a, int weight, hipStream_t s)
{
    const dim3 grid((unsigned)a.nblk, (unsigned)a.count);
    if (weight == 1) hipLaunchKernelGGL(k_pose_scan<1>, grid, dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL(k_pose_scan<0>, grid, dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_pose_scan_reduce, dim3((unsigned)((a.count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, a);
}

}   // namespace cvo_dev
