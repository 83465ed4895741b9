// cvo_stereo.hip -- the semi-global matcher of the front end on MI355X (gfx950): the device side of the
// stereo contract of include/cvo_frontend.h (at cvo_fe_stereo).  Everything here is integer arithmetic; the
// numpy restatement tests/fe_stereo_ref.py holds every plane to it by bytes.
//
// Five kernels, four launches and one per chosen path per frame (eight under the default mask of four paths,
// twelve under all eight):
//   k_fe_stereo_grey    both colour images -> grey (contract 1)
//   k_fe_census         both grey images -> 62-bit census words (contract 2)
//   k_fe_sgm_path x n   one launch per set bit of the path mask: the recurrence of contract 4 along every line of
//                       that direction (rows, columns, or wrapped diagonals), the cost of contract 3 recomputed
//                       from the census rows (no cost volume is stored); the first launch stores S, the others
//                       add to it
//   k_fe_sgm_winner     contracts 5, 6, 8 and the right map of 7, per pixel, into one packed word
//   k_fe_stereo_final   contracts 7, 8 (MIN), 9, 10: the tests, the lookup, the three planes; under a stereo rig
//                       (the rig contract, at cvo_fe_stereo_rig) the instance that ORs OUTSIDE in behind them
// S lies as [y][x][d]: a step of either path direction and the winner read one contiguous vector over d.
#include "cvo_stereo.h"

#include "cvo_frontend.h"

namespace {

constexpr int ST_BLOCK = 256;
constexpr int ST_INF = 0x3FFF;            // above every L_r (<= 64 + 255) with room for + p2
constexpr int CEN_TW = 64, CEN_TH = 4;    // the census tile; CEN_TW * CEN_TH == ST_BLOCK
constexpr int CEN_RX = 4, CEN_RY = 3;     // the window's reach: 9 wide, 7 high
constexpr int CEN_LW = CEN_TW + 2 * CEN_RX, CEN_LH = CEN_TH + 2 * CEN_RY;   // 72 x 10 cells of LDS
static_assert(CEN_TW * CEN_TH == ST_BLOCK, "one thread per pixel of the tile");

// ---- cross-lane steps of one wave (64 lanes, all of them active at every call) --------------------------
// v_mov_b32 with a DPP control: a lane whose source lies outside the row (row_shr), outside the wave
// (wave_shr / wave_shl) or in a row the mask switches off keeps `old`.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int st_dpp(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

// the minimum over the wave, the same in every lane: a prefix minimum inside each row of 16, row 0's total into
// row 1 and row 2's into row 3, lane 31's into rows 2 and 3; lane 63 then holds the minimum of all 64.  `big` is
// a value no smaller than any v.
__device__ __forceinline__ int st_wave_min(int v, int big)
{
    v = min(v, st_dpp<DPP_ROW_SHR1, 0xF>(big, v));
    v = min(v, st_dpp<DPP_ROW_SHR2, 0xF>(big, v));
    v = min(v, st_dpp<DPP_ROW_SHR4, 0xF>(big, v));
    v = min(v, st_dpp<DPP_ROW_SHR8, 0xF>(big, v));
    v = min(v, st_dpp<DPP_ROW_BCAST15, 0xA>(big, v));
    v = min(v, st_dpp<DPP_ROW_BCAST31, 0xC>(big, v));
    return __builtin_amdgcn_readlane(v, 63);
}

// lane i takes lane i - 1's value, lane 0 takes `in`; lane i takes lane i + 1's, lane 63 takes `in`
__device__ __forceinline__ int st_from_below(int v, int in) { return st_dpp<DPP_WAVE_SHR1, 0xF>(in, v); }
__device__ __forceinline__ int st_from_above(int v, int in) { return st_dpp<DPP_WAVE_SHL1, 0xF>(in, v); }

// ---- contract 1 -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ST_BLOCK) k_fe_stereo_grey(const uint8_t *left, const uint8_t *right, int np,
                                                             uint8_t *gray_l, uint8_t *gray_r)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i >= np) return;
    const uint8_t *l = left + 3 * (size_t)i, *r = right + 3 * (size_t)i;
    gray_l[i] = (uint8_t)fe_grey(l[0], l[1], l[2]);
    gray_r[i] = (uint8_t)fe_grey(r[0], r[1], r[2]);
}

// ---- contract 2 -----------------------------------------------------------------------------------------
// A workgroup owns 64 x 4 pixels of one image (blockIdx.z: left, right); the tile and the window's reach go
// to LDS with the coordinates clamped to the image, so that the 62 comparisons of a pixel read LDS bytes only.
__global__ void __launch_bounds__(ST_BLOCK) k_fe_census(const uint8_t *gray_l, const uint8_t *gray_r, int w, int h,
                                                        uint64_t *census_l, uint64_t *census_r)
{
    __shared__ uint8_t s_g[CEN_LH * CEN_LW];
    const uint8_t *gray = blockIdx.z ? gray_r : gray_l;
    uint64_t *census = blockIdx.z ? census_r : census_l;
    const int tx0 = blockIdx.x * CEN_TW, ty0 = blockIdx.y * CEN_TH;
    for (int idx = threadIdx.x; idx < CEN_LH * CEN_LW; idx += ST_BLOCK) {
        const int r = idx / CEN_LW, c = idx - r * CEN_LW;
        const int x = min(max(tx0 - CEN_RX + c, 0), w - 1), y = min(max(ty0 - CEN_RY + r, 0), h - 1);
        s_g[idx] = gray[(size_t)y * w + x];
    }
    __syncthreads();
    const int lx = threadIdx.x % CEN_TW, ly = threadIdx.x / CEN_TW;
    const int x = tx0 + lx, y = ty0 + ly;
    if (x >= w || y >= h) return;
    const int centre = s_g[(ly + CEN_RY) * CEN_LW + lx + CEN_RX];
    uint64_t c = 0;
#pragma unroll
    for (int dy = -CEN_RY; dy <= CEN_RY; ++dy)
#pragma unroll
        for (int dx = -CEN_RX; dx <= CEN_RX; ++dx) {
            if (dy == 0 && dx == 0) continue;
            // (the cell of a neighbour outside the image holds the pixel its clamped coordinates name: filled so above)
            const int n = s_g[(ly + CEN_RY + dy) * CEN_LW + lx + CEN_RX + dx];
            c = (c << 1) | (uint64_t)(n < centre ? 1 : 0);
        }
    census[(size_t)y * w + x] = c;
}

// ---- contracts 3 and 4 ------------------------------------------------------------------------------------
// One wave per line of the direction, lanes over d, NV = 1 for D <= 64 and 2 for D <= 128 (lane l holds d = l and
// d = l + 64).  A lane whose d >= D holds ST_INF throughout: its neighbour sees a term that never wins, which is the
// contract's "left out", and so does lane 0's missing d - 1.  The recurrence is a chain of dependent steps, each a
// wave minimum (six DPP moves) and two neighbour moves; what does not depend on it -- the census words, hence the
// costs, and the sums to add to -- is loaded CH steps ahead of the chain.
//
// Which pixel a line visits at step t, and whether its path begins there, is the Walk's; the chain does not know
// the direction.  AxisWalk: bits 0 to 3 of the path mask (0: left to right, 1: right to left -- a line is a row of
// w steps; 2: top to bottom, 3: bottom to top -- a line is a column of h steps); a path begins at step 0 only.
// DiagWalk: bits 4 to 7, a WRAPPED line: h steps, one row each (downwards for ry = +1, upwards for ry = -1), the
// column moving by rx per step and wrapping round the image: x = (line + rx * t) mod w.  The pixel before, p - r,
// lies outside the image at step 0 (the row) and at the step after a wrap (the column: x == 0 for rx = +1,
// x == w - 1 for rx = -1), and there the path begins anew with L = C.  Between two restarts a wrapped line is one
// true diagonal from the border where it enters to the border where it leaves, and the w lines of a launch visit
// every pixel once.  Every line has h steps, as a vertical one, and the restart is the same in every lane.
struct StStep {
    int x, y;
    bool first;   // p - r lies outside the image: L = C
};

struct AxisWalk {
    static constexpr bool RESTARTS = false;   // a path begins at step 0 and nowhere else
    int w, h, dir;
    __device__ int steps() const { return dir < 2 ? w : h; }
    __device__ StStep at(int line, int t) const
    {
        const int tt = (dir & 1) ? steps() - 1 - t : t;
        return dir < 2 ? StStep{tt, line, t == 0} : StStep{line, tt, t == 0};
    }
};

struct DiagWalk {
    static constexpr bool RESTARTS = true;
    int w, h, rx, ry;
    __device__ int steps() const { return h; }
    __device__ StStep at(int line, int t) const
    {
        int x = (line + rx * t) % w;   // (|rx * t| < h: no overflow; % truncates towards zero, so x > -w)
        if (x < 0) x += w;
        return StStep{x, ry > 0 ? t : h - 1 - t, t == 0 || x == (rx > 0 ? 0 : w - 1)};
    }
};

template <int NV, bool FIRST, class Walk>
__global__ void __launch_bounds__(64) k_fe_sgm_path(const uint64_t *census_l, const uint64_t *census_r, int w, int D,
                                                    int p1, int p2, const Walk walk, uint16_t *sum)
{
    constexpr int CH = 8;
    const int line = blockIdx.x, lane = threadIdx.x;
    const int nsteps = walk.steps();
    int L[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) L[k] = ST_INF;
    for (int t0 = 0; t0 < nsteps; t0 += CH) {
        int cost[CH][NV], old[CH][NV];
        size_t at[CH];
        bool first[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            // (a step past the end repeats the last one and is not run below)
            const StStep p = walk.at(line, min(t0 + j, nsteps - 1));
            const int x = p.x;
            const size_t row = (size_t)p.y * w;
            const uint64_t cl = census_l[row + x];
            at[j] = (row + x) * (size_t)D;
            first[j] = p.first;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int d = lane + 64 * k;
                int c = 64;
                if (d < D && x - d >= 0) c = __popcll(cl ^ census_r[row + x - d]);
                cost[j][k] = c;
                old[j][k] = (!FIRST && d < D) ? (int)sum[at[j] + d] : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if (t0 + j >= nsteps) break;   // (the same in every lane)
            // A path that begins has no pixel before it: L = C.  A walk that begins at step 0 only (AxisWalk) says so at
            // compile time and takes the branch below once per line.  A walk that restarts forgets L instead -- a select on
            // a flag every lane shares -- and runs the step: from L = ST_INF in every lane m is ST_INF and so is every
            // term of the minimum, and cost + ST_INF - ST_INF is the cost.  Either way the eight steps of a chunk stay one
            // straight run of code; with a branch on first[j] per step a launch measured up to 20 % slower.
            if (!Walk::RESTARTS && t0 + j == 0) {
#pragma unroll
                for (int k = 0; k < NV; ++k) L[k] = (lane + 64 * k < D) ? cost[j][k] : ST_INF;
            } else {
                if (Walk::RESTARTS) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) L[k] = first[j] ? ST_INF : L[k];
                }
                int lo = L[0];
                if (NV == 2) lo = min(lo, L[1]);
                const int m = st_wave_min(lo, ST_INF);
                int below[NV], above[NV];
                below[0] = st_from_below(L[0], ST_INF);
                if (NV == 2) {
                    below[1] = st_from_below(L[1], __builtin_amdgcn_readlane(L[0], 63));
                    above[0] = st_from_above(L[0], __builtin_amdgcn_readfirstlane(L[1]));
                    above[1] = st_from_above(L[1], ST_INF);
                } else above[0] = st_from_above(L[0], ST_INF);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int best = min(min(L[k], m + p2), min(below[k], above[k]) + p1);
                    L[k] = (lane + 64 * k < D) ? cost[j][k] + best - m : ST_INF;
                }
            }
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (lane + 64 * k < D) sum[at[j] + lane + 64 * k] = (uint16_t)(old[j][k] + L[k]);
        }
    }
}

// ---- contracts 5, 6, 8 and the right map of 7 -----------------------------------------------------------
// One wave per pixel, lanes over d as above, PW pixels after one another per wave.  The minima are wave minima
// of keys (value << 8 | d: the smallest value, the smallest d on ties); S(d* - 1) and S(d* + 1) come from the
// lanes that hold them.  The right map reads the diagonal S(x + d, y, d): one gathered uint16 per lane.
// With all eight paths S <= 8 * (64 + 255) = 2552 < 2^12: a key S << 8 | d stays below 2^20, and S2 * (100 -
// uniqueness) and S1 * 100 below 255 200 < 2^18, so neither the keys nor the uniqueness test change with the mask.
template <int NV>
__global__ void __launch_bounds__(ST_BLOCK) k_fe_sgm_winner(const uint16_t *sum, int w, int np, int D, int uniqueness,
                                                            uint32_t *win)
{
    constexpr int PW = 4;
    constexpr int KEY_INF = 0x7FFFFFFF;
    const int lane = threadIdx.x & 63;
    const int first = (blockIdx.x * (ST_BLOCK / 64) + (int)(threadIdx.x >> 6)) * PW;
    for (int q = 0; q < PW; ++q) {
        const int i = first + q;
        if (i >= np) return;   // (the same in every lane)
        const int x = i % w;
        int S[NV], key = KEY_INF, keyR = KEY_INF;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int d = lane + 64 * k;
            S[k] = d < D ? (int)sum[(size_t)i * D + d] : 0xFFFF;
            if (d < D) key = min(key, (S[k] << 8) | d);
            if (d < D && x + d < w) keyR = min(keyR, ((int)sum[((size_t)i + d) * D + d] << 8) | d);
        }
        key = st_wave_min(key, KEY_INF);
        keyR = st_wave_min(keyR, KEY_INF);
        const int ds = key & 255, S1 = key >> 8, dR = keyR & 255;
        int s2 = KEY_INF;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int d = lane + 64 * k;
            if (d < D && (d > ds + 1 || d < ds - 1)) s2 = min(s2, S[k]);
        }
        const int S2 = st_wave_min(s2, KEY_INF);
        const bool unique = S2 != KEY_INF && S2 * (100 - uniqueness) < S1 * 100;
        int off = 0;
        if (ds > 0 && ds < D - 1) {   // (the same in every lane)
            const int dm = ds - 1, dp = ds + 1;
            const int Sm = __builtin_amdgcn_readlane(NV == 2 && dm >= 64 ? S[NV - 1] : S[0], dm & 63);
            const int Sp = __builtin_amdgcn_readlane(NV == 2 && dp >= 64 ? S[NV - 1] : S[0], dp & 63);
            const int den = Sm + Sp - 2 * S1;
            if (den > 0) {
                const int num = (Sm - Sp) * 16 + den, dd = 2 * den;
                off = num / dd;
                if (num % dd != 0 && num < 0) --off;   // floor
            }
        }
        if (lane == 0)
            win[i] = (uint32_t)(16 * ds + off) | ((uint32_t)ds << 16) | ((uint32_t)dR << 23) | (unique ? 1u << 30 : 0u);
    }
}

// ---- contracts 7 to 10 ----------------------------------------------------------------------------------
// RIG: the frame came through k_fe_stereo_rectify and `valid` is its plane (bit 0 V_L, bit 1 V_R).  OUTSIDE is ORed in
// behind the other flags, DEPTH's "no other flag" included; the instance without a rig never reads `valid`.
template <bool RIG>
__global__ void __launch_bounds__(ST_BLOCK) k_fe_stereo_final(const uint32_t *win, const uint16_t *table, const uint8_t *valid,
                                                              int w, int np, int min_disp, int lr_max, uint16_t *disparity,
                                                              uint8_t *flags, uint16_t *depth)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i >= np) return;
    const uint32_t v = win[i];
    const int q = (int)(v & 0xFFFFu), ds = (int)((v >> 16) & 127u);
    const int x = i % w;
    uint32_t f = (v >> 30) & 1u ? (uint32_t)CVO_FE_STEREO_UNIQUE : 0u;
    if (lr_max >= 0) {
        bool lr = x - ds < 0;
        if (!lr) {
            const int dR = (int)((win[i - ds] >> 23) & 127u);
            lr = abs(dR - ds) > lr_max;
        }
        if (lr) f |= (uint32_t)CVO_FE_STEREO_LR;
    }
    if (q < 16 * min_disp) f |= (uint32_t)CVO_FE_STEREO_MIN;
    const uint16_t u = table[q];   // (q < 16 * D: the table's length)
    if (f == 0 && u == 0) f = (uint32_t)CVO_FE_STEREO_DEPTH;
    if (RIG) {
        bool outside = (valid[i] & 1u) == 0;
        if (x - ds >= 0) outside = outside || (valid[i - ds] & 2u) == 0;   // (i - ds: the same row, inside the plane)
        if (outside) f |= (uint32_t)CVO_FE_STEREO_OUTSIDE;
    }
    disparity[i] = f ? (uint16_t)0 : (uint16_t)q;
    flags[i] = (uint8_t)f;
    depth[i] = f ? (uint16_t)0 : u;
}

// One launch per set bit of the path mask, in bit order; the first one stores S, the others add to it (no memset).
// Two launches never run in one: they read-modify-write the same S.
template <int NV, bool FIRST> void launch_path(const FeStereoArgs &a, int bit, hipStream_t s)
{
    if (bit < 4) {
        const AxisWalk walk{a.w, a.h, bit};
        hipLaunchKernelGGL((k_fe_sgm_path<NV, FIRST, AxisWalk>), dim3(bit < 2 ? a.h : a.w), dim3(64), 0, s, a.census_l,
                           a.census_r, a.w, a.D, a.p1, a.p2, walk, a.sum);
    } else {
        // bit 4: (+1, +1), 5: (-1, -1), 6: (-1, +1), 7: (+1, -1)
        const DiagWalk walk{a.w, a.h, (bit == 4 || bit == 7) ? 1 : -1, (bit == 4 || bit == 6) ? 1 : -1};
        hipLaunchKernelGGL((k_fe_sgm_path<NV, FIRST, DiagWalk>), dim3(a.w), dim3(64), 0, s, a.census_l, a.census_r, a.w, a.D,
                           a.p1, a.p2, walk, a.sum);
    }
}

template <int NV> void launch_paths(const FeStereoArgs &a, hipStream_t s)
{
    bool first = true;
    for (int bit = 0; bit < 8; ++bit) {
        if (!(a.paths >> bit & 1u)) continue;
        if (first) launch_path<NV, true>(a, bit, s);
        else launch_path<NV, false>(a, bit, s);
        first = false;
    }
    const int np = a.w * a.h, per_block = (ST_BLOCK / 64) * 4;   // (PW of k_fe_sgm_winner)
    hipLaunchKernelGGL(k_fe_sgm_winner<NV>, dim3((np + per_block - 1) / per_block), dim3(ST_BLOCK), 0, s, a.sum, a.w, np, a.D,
                       a.uniqueness, a.win);
}

}   // namespace

void fe_stereo_enqueue(const FeStereoArgs &a, hipStream_t s)
{
    const int np = a.w * a.h, nb = (np + ST_BLOCK - 1) / ST_BLOCK;
    hipLaunchKernelGGL(k_fe_stereo_grey, dim3(nb), dim3(ST_BLOCK), 0, s, a.left, a.right, np, a.gray_l, a.gray_r);
    hipLaunchKernelGGL(k_fe_census, dim3((a.w + CEN_TW - 1) / CEN_TW, (a.h + CEN_TH - 1) / CEN_TH, 2), dim3(ST_BLOCK), 0, s,
                       a.gray_l, a.gray_r, a.w, a.h, a.census_l, a.census_r);
    if (a.D <= 64) launch_paths<1>(a, s);
    else launch_paths<2>(a, s);
    if (a.valid)
        hipLaunchKernelGGL(k_fe_stereo_final<true>, dim3(nb), dim3(ST_BLOCK), 0, s, a.win, a.table, a.valid, a.w, np, a.min_disp,
                           a.lr_max, a.disparity, a.flags, a.depth);
    else
        hipLaunchKernelGGL(k_fe_stereo_final<false>, dim3(nb), dim3(ST_BLOCK), 0, s, a.win, a.table, a.valid, a.w, np, a.min_disp,
                           a.lr_max, a.disparity, a.flags, a.depth);
}
