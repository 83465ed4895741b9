// cvo_matches.hip -- gfx950 (MI355X, CDNA4) kernels of cvo_hip_pose_matches (include/cvo_hip.h).
//
//   k_pose_matches        : one pass over the kept list of a PROC_FLOW pass (the members of A and their float32 weights
//                           at the pose): per row of either cloud the number of members, the sum of their weights and
//                           the member with the largest weight
//   k_pose_matches_finish : turns a row's accumulators into support / count / best / best_w at the row's index in the
//                           caller's cloud (word FEAT_INDEX_SLOT of the row of Cloud::feat) and counts the matched rows
//
// Every accumulation is an integer atomic, so the order in which the members arrive does not show: repeated calls give
// the same bytes.
//   count : 32-bit atomicAdd of 1.
//   best  : 64-bit atomicMax of (bits of the weight << 32) | (0xFFFFFFFF - caller's index of the other point).  A
//           member's weight is positive (k_process keeps a pair only if w > 0), so the bit patterns order as the
//           values do; among equal weights the larger low word -- the smaller caller's index -- wins.  0: no member.
//   sum   : 64-bit atomicAdd of the weight in fixed point with the unit 2^(E - 61), E = floor(log2(inner)), inner the
//           float64 sum of ALL weights of the pass (DevState::red[RED_FLOW + 6], on the device before this kernel
//           starts).  Headroom: a row's sum is at most the sum of all weights <= inner (1 + 2^-20) < 2^(E + 1) (1 + 2^-20)
//           (inner is a float64 sum of fewer than 2^32 positive terms: its rounding error is below 2^32 2^-53 relative),
//           that is below 2^62 (1 + 2^-20) units < 2^63, however many members a row has -- MATCH_UNIT_BITS below.  A
//           float32 weight m 2^(e - 150) (m its 24-bit significand, e its exponent field) is m << (e - 89 - E) units;
//           that is exact while e - 89 - E >= 0, i.e. for every weight from inner 2^-38 up (the fr1/desk pair: inner
//           ~2^15, weights 2^-7: 16 binades to spare).  Below that the shift goes right and drops bits (less than one
//           unit, inner 2^-61, per member); a dropped non-zero bit is counted in MatchCounters::inexact, which the
//           caller gets as `exact` = 0.  Integer addition commutes: with exact terms the sum is THE sum of the weights.
//
// The hazard is the fixed side: consecutive entries of a wave's slice tend to share their fixed row (the flow pass
// expands a tile row by row; fr1/desk: 1 200 members per row), so the 64 lanes of a trip would send their three atomics
// to one address.  COMBINE = true joins the lanes of a run of equal fixed rows first -- a segmented inclusive scan over
// the wave (6 levels of shuffles; the segments are the maximal runs of adjacent lanes with equal row, so that any
// order of the entries is handled) -- and only the last lane of a run sends atomics.  The moving side scatters (a
// column of a tile per lane) and keeps plain atomics.  Both forms give the same bytes; which one a context launches is
// the test switch "matches_combine" (measured: profiles/pose_matches.json).
#include "cvo_device.h"

namespace cvo_dev {

constexpr int MATCH_UNIT_BITS = 62;   // inner < 2^(E + 1) is 2^MATCH_UNIT_BITS units
static_assert(MATCH_UNIT_BITS + 1 <= 63, "a row's sum (<= inner (1 + 2^-20) < 2^(MATCH_UNIT_BITS + 1) units) must fit 64 bits");

// floor(log2(v)) of a positive normal float64
__device__ __forceinline__ int f64_exponent(double v) { return (int)((__double2hiint(v) >> 20) & 0x7ff) - 1023; }

// the weight in units of 2^(E - 61); *dropped: a non-zero bit fell off
__device__ __forceinline__ unsigned long long weight_units(float w, int E, bool *dropped)
{
    const unsigned b = __float_as_uint(w);
    unsigned e = (b >> 23) & 0xffu;
    unsigned long long m = b & 0x7fffffu;
    if (e) m |= 0x800000u; else e = 1;   // (a denormal: no hidden bit, the exponent of field 1)
    const int sh = (int)e - (150 - (MATCH_UNIT_BITS - 1)) - E;
    *dropped = false;
    if (sh >= 0) return m << (sh < 39 ? sh : 39);   // (sh <= 39 always: w <= inner (1 + 2^-20) < 2^(E + 2))
    if (sh <= -24) { *dropped = m != 0; return 0; }
    *dropped = (m & ((1ull << -sh) - 1ull)) != 0;
    return m >> -sh;
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d)
{
    const int lo = __shfl_up((int)(unsigned)v, d, 64), hi = __shfl_up((int)(unsigned)(v >> 32), d, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ void row_atomics(MatchAcc *acc, unsigned row, unsigned long long best, unsigned long long units,
                                            unsigned count)
{
    MatchAcc *r = acc + row;
    atomicMax(&r->best, best);
    atomicAdd(&r->units, units);
    atomicAdd(&r->count, count);
}

// Block b, wave w streams slice 4 b + w of the kept list (kept_slice).
template <bool COMBINE>
__global__ void __launch_bounds__(BLOCK) k_pose_matches(const MatchArgs a)
{
    if ((int)blockIdx.x >= a.kept.nblk) return;
    const int tid = threadIdx.x, lane = tid & 63;
    size_t base;
    unsigned n;
    const CVO_GLOBAL char *kept_w = kept_slice(a.kept, __builtin_amdgcn_readfirstlane(tid >> 6), base, n);
    if (n == 0) return;
    const int E = f64_exponent(a.kept.st->red[RED_FLOW + 6]);   // (n > 0: the pass has members, inner > 0)
    unsigned inexact = 0;
    for (unsigned off0 = 0; off0 < n; off0 += 64u) {   // (wave-uniform trips: the scan below needs every lane)
        const unsigned off = off0 + (unsigned)lane;
        bool live = off < n;
        unsigned i = 0, j = 0;
        float w = 0.0f;
        if (live) {
            kept_entry(a.kept, kept_w, base, off, i, j, w);
            live = i < (unsigned)a.na && j < (unsigned)a.nb;   // (always: a member's rows are rows of the clouds)
        }
        unsigned ci = 0, cj = 0;
        if (live) {
            ci = (unsigned)__float_as_int(a.feat_a[(size_t)i * FEAT_STRIDE + FEAT_INDEX_SLOT]);
            cj = (unsigned)__float_as_int(a.feat_b[(size_t)j * FEAT_STRIDE + FEAT_INDEX_SLOT]);
        }
        bool dropped = false;
        const unsigned long long units = live ? weight_units(w, E, &dropped) : 0ull;
        inexact += dropped ? 1u : 0u;
        const unsigned long long wb = (unsigned long long)__float_as_uint(w) << 32;
        if (live) row_atomics(a.acc_b, j, wb | (0xffffffffu - ci), units, 1u);
        if (!COMBINE) {
            if (live) row_atomics(a.acc_a, i, wb | (0xffffffffu - cj), units, 1u);
        } else {
            // segments: maximal runs of adjacent live lanes with equal i (a dead lane is a segment of its own)
            const unsigned key = live ? i : 0xffffffffu - (unsigned)lane;
            const unsigned key_dn = (unsigned)__shfl_up((int)key, 1, 64), key_up = (unsigned)__shfl_down((int)key, 1, 64);
            int head = (lane == 0 || key_dn != key) ? 1 : 0;
            const bool tail = lane == 63 || key_up != key;
            unsigned long long best = live ? (wb | (0xffffffffu - cj)) : 0ull, sum = units;
            unsigned cnt = live ? 1u : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long best_o = shfl_up_u64(best, d), sum_o = shfl_up_u64(sum, d);
                const unsigned cnt_o = (unsigned)__shfl_up((int)cnt, d, 64);
                const int head_o = __shfl_up(head, d, 64);
                if (lane >= d) {
                    if (!head) {
                        best = best_o > best ? best_o : best;
                        sum += sum_o;
                        cnt += cnt_o;
                    }
                    head |= head_o;
                }
            }
            if (live && tail) row_atomics(a.acc_a, i, best, sum, cnt);
        }
    }
    if (inexact) atomicAdd(&a.counters->inexact, inexact);
}

// One thread per device row of either cloud: blocks [0, blocks_a) the fixed cloud's, the rest the moving cloud's.
__global__ void __launch_bounds__(BLOCK) k_pose_matches_finish(const MatchArgs a)
{
    const int side = (int)blockIdx.x >= a.blocks_a ? 1 : 0;
    const int r = ((int)blockIdx.x - (side ? a.blocks_a : 0)) * BLOCK + (int)threadIdx.x;
    const int nrows = side ? a.nb : a.na, npts = side ? a.n_moving : a.n_fixed;
    const MatchAcc *acc = side ? a.acc_b : a.acc_a;
    const float *feat = side ? a.feat_b : a.feat_a;
    const MatchOut o = a.out[side];
    bool matched = false;
    if (r < nrows) {
        const int c = __float_as_int(feat[(size_t)r * FEAT_STRIDE + FEAT_INDEX_SLOT]);   // (-1: a padding row)
        if (c >= 0 && c < npts) {
            const MatchAcc v = acc[r];
            matched = v.count != 0;
            const int E = matched ? f64_exponent(a.kept.st->red[RED_FLOW + 6]) : 0;
            // (unsigned 64-bit to float64 rounds to nearest: the float64 nearest the sum; the scaling is exact)
            o.support[c] = matched ? __builtin_ldexp((double)v.units, E - (MATCH_UNIT_BITS - 1)) : 0.0;
            o.count[c] = (int32_t)v.count;
            o.best[c] = matched ? (int32_t)(0xffffffffu - (unsigned)(v.best & 0xffffffffull)) : -1;
            o.best_w[c] = matched ? __uint_as_float((unsigned)(v.best >> 32)) : 0.0f;
        }
    }
    const unsigned long long m = __ballot(matched);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(side ? &a.counters->matched_b : &a.counters->matched_a, (unsigned)__popcll(m));
}

void launch_pose_matches(const MatchArgs &a, bool combine, hipStream_t s)
{
    if (combine)
        hipLaunchKernelGGL(k_pose_matches<true>, dim3((unsigned)a.kept.nblk), dim3(BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(k_pose_matches<false>, dim3((unsigned)a.kept.nblk), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_pose_matches_finish, dim3((unsigned)(a.blocks_a + a.blocks_b)), dim3(BLOCK), 0, s, a);
}

}   // namespace cvo_dev
