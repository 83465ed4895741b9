// Host-only check of the bounding-sphere cull of k_filter (csrc/cvo_device.h: spheres_near, cull_slack, apply_tf,
// compute_filter_bounds; se3_math.hpp: inverse_tf) on the extremal stream of tests/test_gpu_hostile.py: two collinear runs
// of 64 points whose nearest end points lie a hair inside or outside sqrt(tau), far from the origin, under a small rotation.
// Per trial the two runs get the spheres k_cloud_seg gives them and the filter geometry fill_filter_geometry gives the pair
// (both restated here: they are host / wave code around a context), the moving run's sphere is moved as filter_body moves
// it, and the cull is asked.  A trial is LOST when the cull drops the pair of runs although a pair of points passes the
// exact test of the list passes (y = apply_tf(Rt, t, y0), e = x - y, d2 = fma(e2, e2, fma(e1, e1, e0 e0)) < tau).
//   cull_host TRIALS SLACK     TRIALS per (offset, largest angle); SLACK 1: reach = sqrt(tauf) + cull_slack, the library's;
//                              SLACK 0: reach = sqrt(tauf), the bound before cull_slack existed
// prints one line per (offset, angle) and "lost L of M" at the end; exit status 1 when a trial was lost.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cvo_device.h"

using namespace cvo_dev;

namespace {
unsigned long long rng_state = 88172645463325252ull;
double rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
double uni(double lo, double hi) { return lo + (hi - lo) * rnd(); }
double gauss()
{
    const double a = std::sqrt(-2.0 * std::log(1.0 - rnd())), b = 6.283185307179586 * rnd();
    return a * std::cos(b);
}
void unit(double d[3])
{
    double n;
    do {
        for (int q = 0; q < 3; ++q) d[q] = gauss();
        n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    } while (n < 1e-3);
    for (int q = 0; q < 3; ++q) d[q] /= n;
}

constexpr int N = 64;

// k_cloud_seg: centre of the run's bounding box, radius = farthest point, inflated
float4 run_sphere(const float (*p)[3], float lo[3], float hi[3])
{
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int i = 0; i < N; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = p[i][a] < lo[a] ? p[i][a] : lo[a];
            hi[a] = p[i][a] > hi[a] ? p[i][a] : hi[a];
        }
    float c[3];
    for (int a = 0; a < 3; ++a) c[a] = (float)(0.5 * ((double)lo[a] + hi[a]));
    double d2 = 0.0;
    for (int i = 0; i < N; ++i) {
        const double dx = (double)p[i][0] - (double)c[0], dy = (double)p[i][1] - (double)c[1], dz = (double)p[i][2] - (double)c[2];
        const double o = (dx * dx + dy * dy) + dz * dz;
        d2 = o > d2 ? o : d2;
    }
    return make_float4(c[0], c[1], c[2], (float)(std::sqrt(d2) * 1.00001 + 1e-6));
}

// fill_filter_geometry's radius of a cloud's box about the centre
float box_radius(const float lo[3], const float hi[3], const float center[3])
{
    double r2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double d = std::fmax(std::fabs((double)lo[a] - center[a]), std::fabs((double)hi[a] - center[a]));
        r2 += d * d;
    }
    return (float)(std::sqrt(r2) * 1.0001 + 1e-6);
}

struct Class { double off[3], gl, gh; };
}   // namespace

int main(int argc, char **argv)
{
    const int trials = argc > 1 ? std::atoi(argv[1]) : 7000;
    const int slack = argc > 2 ? std::atoi(argv[2]) : 1;
    const Class classes[] = {{{0, 0, 1.5}, -3e-3, 1e-4},
                             {{80, -120, 60}, -1e-4, 3e-5},
                             {{300, -500, 200}, -4e-4, 1e-4},
                             {{800, -1200, 600}, -1e-3, 3e-4},
                             {{2000, -3000, 1500}, -3e-3, 1e-3}};
    const double thmax[] = {3e-4, 1e-3, 3e-3};

    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.mode = CVO_HIP_MODE_CVO;
    p.sp = 8e-3f;
    p.log_sp_s2 = (float)std::log((double)(8e-3f / (0.1f * 0.1f)));   // (cvo's defaults: to_dev_params)
    p.c = p.d = 7.0f; p.c_ell = 200.0f;
    p.s2_d = (double)(0.1f * 0.1f); p.cs2_d = 1.0;
    const KernConsts kc = make_kconsts(p, 0.1f);
    const double rt = std::sqrt((double)kc.tau);

    long lost_all = 0, member_all = 0;
    for (const Class &c : classes)
        for (const double tm : thmax) {
            long with_member = 0, lost = 0, culled = 0;
            for (int trial = 0; trial < trials; ++trial) {
                double d[3], ax[3];
                unit(d);
                unit(ax);
                double O[3];
                for (int q = 0; q < 3; ++q) O[q] = c.off[q] + uni(-1.0, 1.0);
                const double g = rt * (1.0 + uni(c.gl, c.gh));
                const double th = tm * std::pow(10.0, uni(-1.0, 0.0));
                const double cs = std::cos(th), sn = std::sin(th), v = 1.0 - cs;
                const double R[9] = {cs + ax[0] * ax[0] * v, ax[0] * ax[1] * v - ax[2] * sn, ax[0] * ax[2] * v + ax[1] * sn,
                                     ax[1] * ax[0] * v + ax[2] * sn, cs + ax[1] * ax[1] * v, ax[1] * ax[2] * v - ax[0] * sn,
                                     ax[2] * ax[0] * v - ax[1] * sn, ax[2] * ax[1] * v + ax[0] * sn, cs + ax[2] * ax[2] * v};
                double T[3];
                for (int q = 0; q < 3; ++q) T[q] = 0.02 * gauss();
                float x[N][3], y0[N][3];
                for (int i = 0; i < N; ++i) {
                    const double s = -0.1 + 0.2 * i / (N - 1);
                    double Y[3];
                    for (int q = 0; q < 3; ++q) {
                        x[i][q] = (float)(O[q] + s * d[q]);
                        Y[q] = O[q] + (0.1 + g + 0.1 + s) * d[q];
                    }
                    for (int r = 0; r < 3; ++r) y0[i][r] = (float)(R[3 * r] * Y[0] + R[3 * r + 1] * Y[1] + R[3 * r + 2] * Y[2] + T[r]);
                }
                DevHead s;
                std::memset(&s, 0, sizeof(s));
                for (int q = 0; q < 9; ++q) s.R[q] = (float)R[q];
                for (int q = 0; q < 3; ++q) s.T[q] = (float)T[q];
                cvo_math::inverse_tf(s.R, s.T, s.Rt, s.t);
                float xlo[3], xhi[3], ylo[3], yhi[3];
                const float4 sa = run_sphere(x, xlo, xhi);
                float4 sb = run_sphere(y0, ylo, yhi);
                for (int a = 0; a < 3; ++a) s.center[a] = 0.5f * (xlo[a] + xhi[a]);
                s.xmax = box_radius(xlo, xhi, s.center);
                s.y0max = box_radius(ylo, yhi, s.center);
                s.kc = kc;
                compute_filter_bounds(&s, false);
                // filter_body: the moving run's sphere under [Rt | t], the radius kept
                const float rb = sb.w;
                sb = apply_tf(s.Rt, s.t, sb);
                sb.w = rb;
                const float reach = std::sqrt(s.tauf[LIST_XY]) + (slack ? cull_slack(s.t, s.center[0], s.center[1], s.center[2], s.xmax, s.y0max) : 0.0f);
                const bool near = spheres_near(sa, sb, reach);
                bool member = false;
                for (int j = 0; j < N && !member; ++j) {
                    const float4 y = apply_tf(s.Rt, s.t, make_float4(y0[j][0], y0[j][1], y0[j][2], 0.0f));
                    for (int i = 0; i < N; ++i) {
                        const float e0 = x[i][0] - y.x, e1 = x[i][1] - y.y, e2 = x[i][2] - y.z;
                        const float d2 = __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0));
                        if (d2 < kc.tau) { member = true; break; }
                    }
                }
                with_member += member;
                culled += !near;
                lost += member && !near;
            }
            std::printf("offset (%g, %g, %g) theta_max %g: %d trials, %ld with a member, %ld culled, %ld lost\n", c.off[0], c.off[1], c.off[2], tm,
                        trials, with_member, culled, lost);
            lost_all += lost;
            member_all += with_member;
        }
    std::printf("lost %ld of %ld\n", lost_all, member_all);
    return lost_all ? 1 : 0;
}
