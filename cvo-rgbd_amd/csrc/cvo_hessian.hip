// cvo_hessian.hip -- gfx950 (MI355X, CDNA4) kernels of cvo_hip_pose_hessian (include/cvo_hip.h).
//
//   k_pose_hessian        : one pass over the kept list of a PROC_FLOW pass (the members of A and their float32
//                           weights at the pose), the gradient and the Hessian terms of every member
//   k_pose_hessian_reduce : one block adds the block partials in a fixed order
//
// Per member (definition in include/cvo_hip.h): r = y - x, J = [[y]x, -I], u = J^T r = (y x x, x - y),
//   dF    = -(a / l^2) u
//   d2F   = (a / l^4) u u^T - (a / l^2) (J^T J + S)
// where J^T J + S, with S the Hessian of r . 1/2 (w x (w x y) + w x v), simplifies to
//   [[ (x.y) I - 1/2 (x y^T + y x^T),  [m]x ],
//    [ -[m]x,                           I   ]],   m = (x + y) / 2.
// Every per-member term is float32 (-ffp-contract=off: the FMAs below are the explicit ones), accumulated per lane in
// float64; the sums go through the same wave reduce-scatter as the list passes'.  No atomics anywhere: repeated calls
// give the same bits.
#include "cvo_device.h"

namespace cvo_dev {

// the 27 sums of one member: acc[0..5] dF, acc[6..26] the upper triangle of d2F row by row
__device__ __forceinline__ void member_hessian_terms(const float4 x, const float4 y, const float w, const float inv_l2,
                                                     const float inv_l, double *acc)
{
    // u = (y x x, x - y) = (r x x, -r): r = y - x first (y is near x: the difference is exact or nearly), then the cross
    // product of the small vector -- no cancellation between the products of y x x
    const float r0 = y.x - x.x, r1 = y.y - x.y, r2 = y.z - x.z;
    float u[6];
    u[0] = r1 * x.z - r2 * x.y;
    u[1] = r2 * x.x - r0 * x.z;
    u[2] = r0 * x.y - r1 * x.x;
    u[3] = -r0;
    u[4] = -r1;
    u[5] = -r2;
    const float p = w * inv_l2;     // a / l^2
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += (double)(p * -u[k]);
    float s[6];                     // u / l: (a / l^4) u_k u_l = p s_k s_l
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = u[k] * inv_l;
    // -(J^T J + S), upper triangle
    // (x.y) I - 1/2 (x y^T + y x^T) has the diagonal x_b y_b + x_c y_c ({b, c} the other two axes)
    const float m0 = 0.5f * (x.x + y.x), m1 = 0.5f * (x.y + y.y), m2 = 0.5f * (x.z + y.z);
    float nm[21];
    nm[0] = -__builtin_fmaf(x.z, y.z, x.y * y.y);            // (0,0)
    nm[1] = 0.5f * __builtin_fmaf(x.x, y.y, x.y * y.x);      // (0,1)
    nm[2] = 0.5f * __builtin_fmaf(x.x, y.z, x.z * y.x);      // (0,2)
    nm[3] = 0.0f;                                            // (0,3)
    nm[4] = m2;                                              // (0,4)
    nm[5] = -m1;                                             // (0,5)
    nm[6] = -__builtin_fmaf(x.z, y.z, x.x * y.x);            // (1,1)
    nm[7] = 0.5f * __builtin_fmaf(x.y, y.z, x.z * y.y);      // (1,2)
    nm[8] = -m2;                                             // (1,3)
    nm[9] = 0.0f;                                            // (1,4)
    nm[10] = m0;                                             // (1,5)
    nm[11] = -__builtin_fmaf(x.y, y.y, x.x * y.x);           // (2,2)
    nm[12] = m1;                                             // (2,3)
    nm[13] = -m0;                                            // (2,4)
    nm[14] = 0.0f;                                           // (2,5)
    nm[15] = -1.0f;                                          // (3,3)
    nm[16] = 0.0f;                                           // (3,4)
    nm[17] = 0.0f;                                           // (3,5)
    nm[18] = -1.0f;                                          // (4,4)
    nm[19] = 0.0f;                                           // (4,5)
    nm[20] = -1.0f;                                          // (5,5)
    int q = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int l = k; l < 6; ++l, ++q) acc[6 + q] += (double)(p * __builtin_fmaf(s[k], s[l], nm[q]));
    }
}

// Block b, wave w streams slice 4 b + w of the kept list (kept_slice).  y is the moving row through apply_tf with the
// state's [Rt|t]: the bits the flow pass tested.
__global__ void __launch_bounds__(BLOCK) k_pose_hessian(const HessArgs a)
{
    __shared__ double red[4 * NACC_HESS];
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
    double acc[NACC_HESS];
#pragma unroll
    for (int k = 0; k < NACC_HESS; ++k) acc[k] = 0.0;
    for (unsigned off = (unsigned)lane; off < n; off += 64u) {
        unsigned i, j;
        float w;
        kept_entry(a.kept, kept_w, base, off, i, j, w);
        const float4 x = load_pos<false>(pos_a, i * 16u);
        const float4 y = apply_tf(Rt, tt, load_pos<false>(pos_b, j * 16u));
        member_hessian_terms(x, y, w, a.inv_l2, a.inv_l, acc);
    }
    const double sum = block_sums<NACC_HESS>(acc, red);
    if (tid < NACC_HESS) a.partials[(size_t)tid * a.kept.nblk + blockIdx.x] = sum;   // [value][block]: coalesced for the reader
}

__global__ void __launch_bounds__(BLOCK) k_pose_hessian_reduce(const HessArgs a)
{
    __shared__ double red[4 * NACC_HESS];
    const double sum = block_partials_sum<NACC_HESS>(a.partials, a.kept.nblk, red);
    if (threadIdx.x < NACC_HESS) a.out[threadIdx.x] = sum;
}

void launch_pose_hessian(const HessArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_hessian, dim3((unsigned)a.kept.nblk), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_pose_hessian_reduce, dim3(1), dim3(BLOCK), 0, s, a);
}

}   // namespace cvo_dev
