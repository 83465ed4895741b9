// cvo_pair.h -- the arithmetic of one pair (x_i, y_j), shared by the list kernels (cvo_kernels.hip) and the pose scan
// (cvo_scan.hip): the feature distance, exp for the kernel weights and its table, the pair weight.  One copy: the
// member rule and every float32 weight are the same bits in both translation units.
#pragma once

#include "cvo_device.h"

namespace cvo_dev {

__device__ __forceinline__ float d2_feat(const float4 fa0, const float fa4, const float4 fb0,
                                         const float fb4)
{
    const float e0 = fa0.x - fb0.x, e1 = fa0.y - fb0.y, e2 = fa0.z - fb0.z, e3 = fa0.w - fb0.w,
                e4 = fa4 - fb4;
    float r = e0 * e0;
    r = __builtin_fmaf(e1, e1, r);
    r = __builtin_fmaf(e2, e2, r);
    r = __builtin_fmaf(e3, e3, r);
    r = __builtin_fmaf(e4, e4, r);
    return r;
}

// ---------------------------------------------------------------------------
// exp(x) for the kernel weights, x <= 0 (ref cvo.cpp:149-150 calls the double
// overload of exp).  2^(k/64) table + degree-5 polynomial on |r| <= ln2/128, the
// scheme of every libm: at most one ulp from glibc's exp (differs from it in the
// last bit for 25 % of the arguments) and -- what the arithmetic contract needs --
// the float32 values of sigma^2 exp(x) and c_sigma^2 exp(x) are libm's, which the
// suite holds pair by pair: tests/test_gpu_pair_weight.py compares every kept weight
// of the stars of tests/pair_weight_cases.py with the oracle's (libm's exp) by bits,
// at exponents down to -83 on the spatial and -64 on the colour side, results down
// to float32 subnormals, and both with the float64 reference (whose own exp
// tests/test_pair_weight_cpu.py holds to 60-digit arithmetic).  With the low part of
// ln2/64 below set to zero that test fails at the far exponents.
// 14 float64 operations instead of ~30 in the device libm;
// the two exp are the largest single item of the per-pair work.
__device__ const double c_exp2_64[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0,
};

__device__ __forceinline__ double exp_neg(double x, const double *tab /* LDS copy of c_exp2_64 */)
{
    const double kd = __builtin_rint(x * 0x1.71547652b82fep+6);          // x * 64/ln2
    const int k = (int)kd;
    double r = __builtin_fma(-kd, 0x1.62e42fee00000p-7, x);              // ln2/64, high part (exact product)
    r = __builtin_fma(-kd, 0x1.a39ef35793c76p-39, r);                    // low part
    double p = 1.0 / 120.0;
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = p * r;
    const double s = tab[k & 63];
    return __builtin_ldexp(__builtin_fma(s, p, s), k >> 6);
}

// pair weight for a pair that passed d2 < tau; 0 if dropped.
// WEIGHT 0: the C++ objects' (ref cvo.cpp:143-153).  WEIGHT 1: the MATLAB object's (SURVEY 8
// a9, ref rkhs_se3_registration.m:40-73,125-127): linear colour inner product, threshold on
// K alone -- a separate instantiation (k_process<PROC_FLOW, 1>), so that the kernels of the
// main path carry nothing of it (a run-time branch here cost them 6 %).
template <int WEIGHT>
__device__ __forceinline__ float pair_weight(const KernConsts &kc, float d2, const float4 fa0,
                                             const float fa4, const float4 fb0, const float fb4,
                                             const double *etab)
{
    if (WEIGHT == 1) {
        const float km = (float)(kc.s2_d * exp_neg((double)d2 * kc.ninv_2l2, etab));
        if (!(km >= kc.sp)) return 0.0f;
        const float ci = kc.cscale * ((fa0.x * fb0.x + fa0.y * fb0.y) + fa0.z * fb0.z);
        return ci * km;
    }
    const float d2c = d2_feat(fa0, fa4, fb0, fb4);
    if (!(d2c < kc.tau_c)) return 0.0f;
    const float k = (float)(kc.s2_d * exp_neg((double)d2 * kc.ninv_2l2, etab));
    const float ck = (float)(kc.cs2_d * exp_neg((double)d2c * kc.ninv_2cl2, etab));
    const float a = ck * k;
    return a > kc.sp ? a : 0.0f;
}

}   // namespace cvo_dev
