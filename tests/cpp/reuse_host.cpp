// Host-only check of the re-use bounds of the list plans (csrc/cvo_device.h: prepare_iteration -> plan_lists, plan_xy_async,
// plan_self_async_one; pose_travel, xy_travel, compute_filter_bounds, apply_tf; se3_math.hpp: inverse_tf) far from the origin,
// on an extremal stream: one pair of points per trial, a build at one pose, then a change of pose (or a growth of the length
// scale) that uses up all but 0 - 0.2 % of what the plan still allows -- found by bisection ON THE PLAN ITSELF, nothing of it is
// restated here -- and that brings the pair to sqrt(tau) +- a few ulp of the coordinates.
//   The list of a build is the smallest the filter may give: the pairs whose float32 d2 (apply_tf at the build's pose, e = x - y,
//   d2 = fma(e2, e2, fma(e1, e1, e0 e0)), as eval_pair) is below the build's own tauf (tauf[l] after the plan, tauf_build,
//   sf_tauf_build); after a narrowing or an expansion of a bounded record the record keeps d2 < rec_r rec_r at that pose
//   (stream_candidates, process_body).  A trial is LOST when the plan names re-use or a narrowing and the pair is a member at the
//   current pose by the float32 test d2 < tau, yet absent from the tile list or the record.
// Plans (one class = one plan at one offset): `sync` plan_lists on the xy list, record_narrow off; `narrow` the same with
// record_narrow on, a drop of the length scale that narrows the record or a change of launch geometry that expands the bounded
// record, then re-use against the record's own radius and pose; `async` plan_xy_async over both buffers; `yy` plan_lists with
// LIST_YY and `yy-async` plan_self_async_one<1>, where BOTH points are moved by apply_tf at the current pose while the plan
// treats the list as rigid and the length scale grows until r0 reaches the list's radius.  The xx list is never transformed:
// its d2 must be the same bits at both poses.
//   Pose changes: a rotation of 1e-5 .. 1e-2 rad about the image of the cloud's centre, the pair one extent away and moving
// straight towards its partner (the rotational part of the bound is tight; 1.5 km and more from the origin dt and dRt c are
// metres and cancel), or -- every fourth trial -- about an axis through the pair; then a translation towards the partner.
// For the yy plans every second trial also shifts the moving cloud by 1 mm .. 100 m between the build and the current pose: the list is
// rigid, nothing ties the build's t to the current one, and one offset class has an axis-aligned centre, (3000, 0, 0), where sums of
// |coordinates| leave a bound made of the current t alone no room.
//   The plan steps are those of the classic launches (plan_builds_none, then plan_builds_classic: the build named by one step is
// judged by the next).  Head mode (plan_builds_head: a build in flight blocks a new one and is judged two slots later) hands the
// same plan_xy_async / plan_self_async_one the same state with other values of fresh / inflight; the bounds under test, `need <= radius`
// with need and radius made as here, are the same expressions on that path.  It is not driven here.
//   Also asserted: pose_travel / xy_travel bound the float64 displacement of every point within y0max of the centre,
// displacement <= travel 1.0001 + the library's slack.
//   reuse_host [TRIALS]        TRIALS per class (default 6000); one line per (offset, plan, length scale), exit status 1 when a
//                              trial was lost, a travel bound failed or a class misses its floors (>= 90 % of the trials re-use;
//                              1.5 km and beyond: >= 200 trials with a member under a re-used list)
//   -DREUSE_HOST_OLD_SLACK     for a header without reuse_slack: the travel assertion then takes 1e-4 (1 + xmax + y0max)
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
void cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
void perp_unit(const double e[3], double n[3])   // a random unit vector perpendicular to e
{
    double r[3], len;
    do {
        unit(r);
        cross(e, r, n);
        len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    } while (len < 0.1);
    for (int q = 0; q < 3; ++q) n[q] /= len;
}
void rotation(const double ax[3], double th, double R[9])
{
    const double cs = std::cos(th), sn = std::sin(th), v = 1.0 - cs;
    const double M[9] = {cs + ax[0] * ax[0] * v, ax[0] * ax[1] * v - ax[2] * sn, ax[0] * ax[2] * v + ax[1] * sn,
                         ax[1] * ax[0] * v + ax[2] * sn, cs + ax[1] * ax[1] * v, ax[1] * ax[2] * v - ax[0] * sn,
                         ax[2] * ax[0] * v - ax[1] * sn, ax[2] * ax[1] * v + ax[0] * sn, cs + ax[2] * ax[2] * v};
    std::memcpy(R, M, sizeof(M));
}

// a rigid map y' = A y0 + b of the moving cloud into the fixed cloud's frame, float64
struct Map { double A[9], b[3]; };
void map_apply(const Map &m, const double p[3], double o[3])
{
    for (int r = 0; r < 3; ++r) o[r] = m.A[3 * r] * p[0] + m.A[3 * r + 1] * p[1] + m.A[3 * r + 2] * p[2] + m.b[r];
}
void map_inverse_apply(const Map &m, const double p[3], double o[3])
{
    const double d[3] = {p[0] - m.b[0], p[1] - m.b[1], p[2] - m.b[2]};
    for (int r = 0; r < 3; ++r) o[r] = m.A[r] * d[0] + m.A[3 + r] * d[1] + m.A[6 + r] * d[2];
}
// G o m: G = the rotation by th about the axis `ax` through `pivot`, then the shift tau e
Map moved(const Map &m, const double ax[3], double th, const double pivot[3], const double e[3], double tau)
{
    double Rg[9];
    rotation(ax, th, Rg);
    Map o;
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) o.A[3 * r + q] = Rg[3 * r] * m.A[q] + Rg[3 * r + 1] * m.A[3 + q] + Rg[3 * r + 2] * m.A[6 + q];
    const double d[3] = {m.b[0] - pivot[0], m.b[1] - pivot[1], m.b[2] - pivot[2]};
    for (int r = 0; r < 3; ++r) o.b[r] = Rg[3 * r] * d[0] + Rg[3 * r + 1] * d[1] + Rg[3 * r + 2] * d[2] + pivot[r] + tau * e[r];
    return o;
}
// the state's pose (R, T) is the inverse of the map, rounded to float32 once; [Rt | t] is the library's own inverse of that
void set_pose(DevHead *s, const Map &m)
{
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) s->R[3 * r + q] = (float)m.A[3 * q + r];
        s->T[r] = (float)(-(m.A[r] * m.b[0] + m.A[3 + r] * m.b[1] + m.A[6 + r] * m.b[2]));
    }
}
struct Pose { float Rt[9], t[3]; };
Pose pose_of(const DevHead &s)
{
    Pose p;
    std::memcpy(p.Rt, s.Rt, sizeof(p.Rt));
    std::memcpy(p.t, s.t, sizeof(p.t));
    return p;
}
// the exact image of a float32 point under the float32 pose, float64
void image(const Pose &p, const float y0[3], double o[3])
{
    for (int r = 0; r < 3; ++r)
        o[r] = ((double)p.Rt[3 * r] * y0[0] + (double)p.Rt[3 * r + 1] * y0[1]) + (double)p.Rt[3 * r + 2] * y0[2] + (double)p.t[r];
}
// eval_pair's squared distance: either point moved by apply_tf where its cloud is
float pair_d2(const Pose &p, const int tf_a, const int tf_b, const float a[3], const float b[3])
{
    float4 xi = make_float4(a[0], a[1], a[2], 0.0f), yj = make_float4(b[0], b[1], b[2], 0.0f);
    if (tf_a) xi = apply_tf(p.Rt, p.t, xi);
    if (tf_b) yj = apply_tf(p.Rt, p.t, yj);
    const float e0 = xi.x - yj.x, e1 = xi.y - yj.y, e2 = xi.z - yj.z;
    return __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, e0 * e0));
}
double dist3(const double a[3], const double b[3])
{
    return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}
float lib_slack(const DevHead &s)
{
#ifdef REUSE_HOST_OLD_SLACK
    return 1.0e-4f * (1.0f + s.xmax + s.y0max);
#else
    return reuse_slack(s.t, s.center, s.xmax, s.y0max, 1.0f);
#endif
}

DevParams params(bool acvo)
{
    DevParams p;
    std::memset(&p, 0, sizeof(p));
    const float sp = acvo ? 8.315e-3f : 8e-3f;   // (the defaults of cvo_hip_default_params through make_dev_params)
    p.mode = acvo ? CVO_HIP_MODE_ACVO : CVO_HIP_MODE_CVO;
    p.sp = p.c_sp = sp;
    p.c = p.d = 7.0f;
    p.c_ell = acvo ? 0.5f : 200.0f;
    p.log_sp_s2 = (float)std::log((double)(sp / (0.1f * 0.1f)));
    p.tau_c = (float)(-2.0 * p.c_ell * p.c_ell * (double)(float)std::log((double)(sp / 1.0f / 1.0f)));
    p.s2_d = (double)(0.1f * 0.1f); p.cs2_d = 1.0;
    p.ell_min = acvo ? 0.0391f : 0.0f; p.ell_max_init = 0.15f;
    p.build_at = 0.7f;
    p.list_stale_max = 3.0f;
    return p;
}

// one plan step at the state's (R, T, ell) the way the post kernels take it (classic launches)
void plan(DevHead *s, const DevParams &p, const Map &m, float ell, bool first)
{
    set_pose(s, m);
    s->ell = ell;
    if (p.async_self && !p.async_xy) s->stall = 0;   // (plan_xy_async is what clears it otherwise)
    const PlanBuilds b = first ? plan_builds_none() : plan_builds_classic(s, false, false, false);
    prepare_iteration(s, s, true, p, b);
}
template <class F> double bisect(F ok, double lo, double hi)   // the largest v in [lo, hi] with ok(v); ok(lo) holds
{
    if (ok(hi)) return hi;
    for (int it = 0; it < 26; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (ok(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

enum Plan { SYNC = 0, NARROW, ASYNC, YY, YY_ASYNC, NPLAN };
const char *plan_name[NPLAN] = {"sync", "narrow", "async", "yy", "yy-async"};
struct Offset { double off[3]; bool far; };
struct Tally { long trials, reuse, member, lost; };

long travel_checks = 0, travel_failures = 0;
void check_travel(const char *what, const DevHead &s, const float travel, const Pose &from, const Pose &now, const float y0[3])
{
    double a[3], b[3];
    image(from, y0, a);
    image(now, y0, b);
    const double moved = dist3(a, b), bound = (double)travel * 1.0001 + (double)lib_slack(s);
    ++travel_checks;
    if (!(moved <= bound)) {
        if (++travel_failures <= 20)
            std::printf("  TRAVEL %s: a point moved %.9g, the bound is %.9g (travel %.9g) about centre (%g, %g, %g)\n", what, moved, bound, (double)travel,
                        (double)s.center[0], (double)s.center[1], (double)s.center[2]);
    }
}
// the pair's own moving point and three more within y0max of the centre
void check_travel_points(const char *what, const DevHead &s, const float travel, const Pose &from, const Pose &now, const float y0[3])
{
    check_travel(what, s, travel, from, now, y0);
    for (int k = 0; k < 3; ++k) {
        double d[3];
        unit(d);
        const double rho = (double)s.y0max * (k == 0 ? 0.9999 : rnd());
        const float p[3] = {(float)((double)s.center[0] + rho * d[0]), (float)((double)s.center[1] + rho * d[1]), (float)((double)s.center[2] + rho * d[2])};
        const double back[3] = {(double)p[0] - s.center[0], (double)p[1] - s.center[1], (double)p[2] - s.center[2]};
        if (std::sqrt(back[0] * back[0] + back[1] * back[1] + back[2] * back[2]) <= (double)s.y0max) check_travel(what, s, travel, from, now, p);
    }
}

const float ELLS[4] = {0.15f, 0.10f, 0.06f, 0.03f};
long loss_lines = 0;

// one trial of an xy plan; returns the length-scale bucket, fills reuse / member / lost
int trial_xy(const int plan_id, const Offset &oc, const double band, const long trial, bool &reuse, bool &member, bool &lost, const bool no_chain = false)
{
    DevParams p = params(false);
    p.list_margin = (trial / 4) % 2 ? 0.15f : 0.25f;
    const double extent = ((trial / 8) % 3 == 0) ? 0.2 : ((trial / 8) % 3 == 1) ? 1.0 : 3.0;
    const bool chain_narrow = plan_id == NARROW && (trial / 24) % 2 == 0 && !no_chain;   // else: an expansion of the bounded record
    int bucket = chain_narrow ? (int)(trial % 3) : (int)(trial % 4);        // (a narrowing needs a length scale to drop to)
    const float ell_a = ELLS[bucket], ell_b = chain_narrow ? ELLS[bucket + 1] : ell_a;
    if (chain_narrow) bucket += 1;   // (reported by the length scale the member is judged at)
    p.record_narrow = plan_id == NARROW;
    p.async_xy = plan_id == ASYNC;

    DevHead s;
    std::memset(&s, 0, sizeof(s));
    for (int q = 0; q < 3; ++q) s.center[q] = (float)(oc.off[q] + uni(-1.0, 1.0));
    const double c[3] = {s.center[0], s.center[1], s.center[2]};
    s.y0max = (float)extent;
    s.xmax = (float)(extent + 0.3);   // (the partner lies up to a list radius beside a point one extent out)

    // the build's pose: a small rotation about the centre and a small shift
    Map m0;
    double ax0[3], sh[3];
    unit(ax0);
    for (int q = 0; q < 3; ++q) sh[q] = 0.01 * gauss();
    {
        Map id = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
        m0 = moved(id, ax0, uni(0.0, 0.02), c, sh, 1.0);
    }
    plan(&s, p, m0, ell_a, true);
    Pose built[2];
    float tauf_built[2] = {0.0f, 0.0f};
    if (plan_id == ASYNC) {
        if (!(s.stall == 1 && s.xy_target == 0)) { std::printf("  the first asynchronous plan did not name a build of buffer 0\n"); lost = true; return bucket; }
        tauf_built[0] = s.tauf_build;
    } else {
        if (s.reuse[LIST_XY] != 0) { std::printf("  the first plan did not name a build\n"); lost = true; return bucket; }
        tauf_built[0] = s.tauf[LIST_XY];
    }
    built[0] = pose_of(s);
    int nblk = 64;
    s.ck_nblk[LIST_XY] = nblk;   // (head_plan: the pass after the build has recorded the list)

    // the motion: direction e towards the partner, the pair's moving point y' (at the build) and the pivot
    double e[3], n[3], ax[3], q0[3], yb[3];
    unit(e);
    perp_unit(e, n);
    map_apply(m0, c, q0);   // the image of the centre
    const bool through_pair = (trial / 48) % 4 == 3;
    const double rho = extent * uni(0.9, 0.999);
    double pivot[3];
    for (int q = 0; q < 3; ++q) yb[q] = q0[q] + rho * n[q];
    if (through_pair) { for (int q = 0; q < 3; ++q) { pivot[q] = yb[q]; ax[q] = e[q]; } }
    else { cross(n, e, ax); for (int q = 0; q < 3; ++q) pivot[q] = q0[q]; }
    double th = std::pow(10.0, uni(-5.0, -2.0));

    const auto good = [&](const DevHead &t) { return plan_id == ASYNC ? t.stall == 0 : t.reuse[LIST_XY] == 1; };
    // ---- step 1 (narrow, async): a first change of pose, committed
    Map m1 = m0;
    Pose pose1 = built[0];
    bool filtered1 = false;
    float rec_lim1 = 0.0f;
    if (plan_id == NARROW || plan_id == ASYNC) {
        double th1 = th;
        const auto ok1 = [&](double tau) { DevHead t = s; plan(&t, p, moved(m0, ax, th1, pivot, e, tau), ell_b, false); return good(t); };
        while (!ok1(0.0) && th1 > 1e-5) th1 = std::fmax(th1 * 0.1, 1e-5);
        // (a drop the plan answers with a build whatever the pose -- far out the slack leaves the record no room to narrow into --
        // has nothing to lose: the trial is drawn again as an expansion)
        if (!ok1(0.0) && chain_narrow) return trial_xy(plan_id, oc, band, trial, reuse, member, lost, true);
        if (!ok1(0.0)) { reuse = false; return bucket; }
        const double room = bisect(ok1, 0.0, 1.0);
        const double tau1 = chain_narrow ? room * (1.0 - 2e-3 * rnd()) : room * rnd();
        m1 = moved(m0, ax, th1, pivot, e, tau1);
        if (plan_id == NARROW && !chain_narrow) nblk = 32;   // the launch geometry changes: the flow pass expands the tile list again
        plan(&s, p, m1, ell_b, false);
        if (!good(s)) { reuse = false; return bucket; }
        pose1 = pose_of(s);
        if (plan_id == ASYNC) {
            if (s.xy_target == 1) { built[1] = pose1; tauf_built[1] = s.tauf_build; }
        } else {
            const bool bounded = (s.narrow & REC_BOUNDED) != 0, expand = s.ck_nblk[LIST_XY] != nblk;
            if (expand) {   // process_body keeps d2 < rec_r^2 of a bounded record; head_plan moves the record's pose
                filtered1 = bounded;
                if (bounded) { std::memcpy(s.rec_Rt, s.Rt, sizeof(s.Rt)); std::memcpy(s.rec_t, s.t, sizeof(s.t)); }
            } else if (s.narrow & REC_NARROW) filtered1 = true;   // stream_candidates
            rec_lim1 = s.rec_r * s.rec_r;
            s.ck_nblk[LIST_XY] = nblk;
        }
        for (int q = 0; q < 3; ++q) {   // the pivot and the point go with the cloud
            yb[q] += ((through_pair ? 0.0 : th1 * rho) + tau1) * e[q];
            pivot[q] = through_pair ? yb[q] : pivot[q] + tau1 * e[q];
        }
    }
    // ---- the last step: all but 0 - 0.2 % of what the plan still allows
    const auto ok2 = [&](double tau) { DevHead t = s; plan(&t, p, moved(m1, ax, th, pivot, e, tau), ell_b, false); return good(t); };
    while (!ok2(0.0) && th > 1e-5) th = std::fmax(th * 0.1, 1e-5);
    if (!ok2(0.0)) { reuse = false; return bucket; }
    const double room = bisect(ok2, 0.0, 1.0);
    const Map m2 = moved(m1, ax, th, pivot, e, room * (1.0 - 2e-3 * rnd()));
    DevHead s2 = s;
    plan(&s2, p, m2, ell_b, false);
    reuse = good(s2);
    const Pose pose2 = pose_of(s2);

    // the pair: y0 the moving point as stored, x = its exact image at the last pose + (sqrt(tau) +- band) e
    double y0d[3], Y2[3];
    {
        double at_build[3];
        for (int q = 0; q < 3; ++q) at_build[q] = q0[q] + rho * n[q];
        map_inverse_apply(m0, at_build, y0d);
    }
    const float y0[3] = {(float)y0d[0], (float)y0d[1], (float)y0d[2]};
    image(pose2, y0, Y2);
    const double r_now = std::sqrt((double)s2.kc.tau), gap = r_now + uni(-band, band);
    const float x[3] = {(float)(Y2[0] + gap * e[0]), (float)(Y2[1] + gap * e[1]), (float)(Y2[2] + gap * e[2])};
    const double xd[3] = {x[0], x[1], x[2]};

    member = pair_d2(pose2, 0, 1, x, y0) < s2.kc.tau;
    bool in_tile, in_record;
    int act = 0;
    if (plan_id == ASYNC) {
        act = s2.xy_active ? 1 : 0;
        in_tile = in_record = pair_d2(built[act], 0, 1, x, y0) < tauf_built[act];
    } else {
        in_tile = pair_d2(built[0], 0, 1, x, y0) < tauf_built[0];
        in_record = in_tile && (!filtered1 || pair_d2(pose1, 0, 1, x, y0) < rec_lim1);
    }
    lost = reuse && member && !(in_tile && in_record);
    if (lost && ++loss_lines <= 40) {
        double Yb[3], Y1[3];
        image(built[act], y0, Yb);
        image(pose1, y0, Y1);
        std::printf("  LOST %s offset (%g, %g, %g) ell %.2f margin %.2f extent %g theta %.2g: float64 distance %.9g at the build, %.9g at the record's pose, "
                    "%.9g now; sqrt(tau) %.9g list radius %.9g; in the tile list %d in the record %d\n", plan_name[plan_id], oc.off[0], oc.off[1], oc.off[2],
                    (double)ell_b, (double)p.list_margin, extent, th, dist3(xd, Yb), dist3(xd, Y1), dist3(xd, Y2), r_now,
                    (double)(plan_id == ASYNC ? s2.xy_r[act] : s2.list_r[LIST_XY]), (int)in_tile, (int)in_record);
    }
    // ---- the travel bounds as bounds
    if (plan_id == ASYNC) {
        if (s2.xy_ok[0]) check_travel_points("xy_travel<0>", s2, xy_travel<0>(&s2, &s2), built[0], pose2, y0);
        if (s2.xy_ok[1]) check_travel_points("xy_travel<1>", s2, xy_travel<1>(&s2, &s2), built[1], pose2, y0);
    } else {
        check_travel_points("pose_travel (list)", s2, pose_travel(&s2, s.list_Rt, s.list_t, s2.y0max), built[0], pose2, y0);
        Pose rec;
        std::memcpy(rec.Rt, s.rec_Rt, sizeof(rec.Rt));
        std::memcpy(rec.t, s.rec_t, sizeof(rec.t));
        check_travel_points("pose_travel (record)", s2, pose_travel(&s2, s.rec_Rt, s.rec_t, s2.y0max), rec, pose2, y0);
    }
    return bucket;
}

// one trial of a yy plan: both points are the moving cloud's, the length scale grows
void trial_yy(const int plan_id, const Offset &oc, const double band, const long trial, bool &reuse, bool &member, bool &lost)
{
    DevParams p = params(true);
    p.list_margin = (trial / 4) % 2 ? 0.15f : 0.25f;
    const double extent = ((trial / 8) % 3 == 0) ? 0.2 : ((trial / 8) % 3 == 1) ? 1.0 : 3.0;
    p.async_self = plan_id == YY_ASYNC;
    DevHead s;
    std::memset(&s, 0, sizeof(s));
    for (int q = 0; q < 3; ++q) s.center[q] = (float)(oc.off[q] + uni(-1.0, 1.0));
    const double c[3] = {s.center[0], s.center[1], s.center[2]};
    s.y0max = (float)(extent + 0.3);
    s.xmax = (float)extent;
    const float ell0 = (float)uni(0.0391, 0.12);

    Map m0;
    double ax0[3], sh[3];
    unit(ax0);
    for (int q = 0; q < 3; ++q) sh[q] = 0.01 * gauss();
    {
        Map id = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
        m0 = moved(id, ax0, uni(0.0, 0.02), c, sh, 1.0);
    }
    plan(&s, p, m0, ell0, true);
    Pose built[2];
    float tauf_built[2] = {0.0f, 0.0f};
    built[0] = pose_of(s);
    if (plan_id == YY_ASYNC) {
        if (s.sf_target[1] != 0) { std::printf("  the first asynchronous plan did not name a build of yy buffer 0\n"); lost = true; return; }
        tauf_built[0] = s.sf_tauf_build[1];
    } else {
        if (s.reuse[LIST_YY] != 0) { std::printf("  the first plan did not name a build of the yy list\n"); lost = true; return; }
        tauf_built[0] = s.tauf[LIST_YY];
    }
    const auto good = [&](const DevHead &t) { return plan_id == YY_ASYNC ? t.stall == 0 : t.reuse[LIST_YY] == 1; };
    double q0[3];
    map_apply(m0, c, q0);
    // a pose change per step: any rotation about the image of the centre and a small shift (the list is rigid: no budget to keep)
    const auto change = [&](const Map &m) {
        double ax[3], e[3];
        unit(ax);
        unit(e);
        return moved(m, ax, std::pow(10.0, uni(-5.0, -2.0)), q0, e, trial % 2 ? std::pow(10.0, uni(-3.0, 2.0)) : 0.005 * rnd());
    };
    float ell1 = ell0;
    Map m1 = m0;
    if (plan_id == YY_ASYNC) {   // a first step, committed: part of the room, and perhaps a build of the other buffer ahead
        m1 = change(m0);
        const auto ok1 = [&](double ell) { DevHead t = s; plan(&t, p, m1, (float)ell, false); return good(t); };
        if (!ok1(ell0)) { reuse = false; return; }
        const double top = bisect(ok1, ell0, 1.6 * ell0);
        ell1 = (float)(ell0 + rnd() * (top - ell0));
        plan(&s, p, m1, ell1, false);
        if (!good(s)) { reuse = false; return; }
        if (s.sf_target[1] >= 0) { built[s.sf_target[1]] = pose_of(s); tauf_built[s.sf_target[1]] = s.sf_tauf_build[1]; }
    }
    const Map m2 = change(m1);
    const auto ok2 = [&](double ell) { DevHead t = s; plan(&t, p, m2, (float)ell, false); return good(t); };
    if (!ok2(ell1)) { reuse = false; return; }
    const double top = bisect(ok2, ell1, 1.6 * ell1);
    const float ell2 = (float)(top - 2e-3 * rnd() * (top - ell1));
    DevHead s2 = s;
    plan(&s2, p, m2, ell2, false);
    reuse = good(s2);
    const Pose pose2 = pose_of(s2);
    const int act = plan_id == YY_ASYNC ? (s2.sf_active[1] ? 1 : 0) : 0;

    // the pair, as stored: a within the extent of the centre, b = a + (sqrt(tau) +- band) e
    double d[3], e[3];
    unit(d);
    unit(e);
    const double rho = extent * rnd(), r_now = std::sqrt((double)s2.kc.tau), gap = r_now + uni(-band, band);
    const float a[3] = {(float)(c[0] + rho * d[0]), (float)(c[1] + rho * d[1]), (float)(c[2] + rho * d[2])};
    const float b[3] = {(float)((double)a[0] + gap * e[0]), (float)((double)a[1] + gap * e[1]), (float)((double)a[2] + gap * e[2])};
    member = pair_d2(pose2, 1, 1, a, b) < s2.kc.tau;
    const bool in_list = pair_d2(built[act], 1, 1, a, b) < tauf_built[act];
    lost = reuse && member && !in_list;
    if (lost && ++loss_lines <= 40) {
        double A0[3], B0[3], A2[3], B2[3];
        image(built[act], a, A0); image(built[act], b, B0);
        image(pose2, a, A2); image(pose2, b, B2);
        std::printf("  LOST %s offset (%g, %g, %g) ell %.4f -> %.4f margin %.2f extent %g: float64 distance %.9g at the build, %.9g now; sqrt(tau) %.9g "
                    "list radius %.9g\n", plan_name[plan_id], oc.off[0], oc.off[1], oc.off[2], (double)ell0, (double)ell2, (double)p.list_margin, extent,
                    dist3(A0, B0), dist3(A2, B2), r_now, (double)(plan_id == YY_ASYNC ? s2.sf_r[1][act] : s2.list_r[LIST_YY]));
    }
    // the xx list: neither point is moved, the pose cannot reach its d2
    const float xa[3] = {a[0], a[1], a[2]}, xb[3] = {b[0], b[1], b[2]};
    const float d2_build = pair_d2(built[0], 0, 0, xa, xb), d2_now = pair_d2(pose2, 0, 0, xa, xb);
    if (std::memcmp(&d2_build, &d2_now, sizeof(float)) != 0) { std::printf("  the xx list's d2 changed with the pose\n"); lost = true; }
}
}   // namespace

int main(int argc, char **argv)
{
    const long trials = argc > 1 ? std::atol(argv[1]) : 6000;
    // the five offset classes of cull_host.cpp, two whose coordinates straddle a binade edge (the centre is drawn within 1 m) and one
    // on an axis
    const Offset offsets[] = {{{0, 0, 1.5}, false}, {{80, -120, 60}, false}, {{300, -500, 200}, false}, {{800, -1200, 600}, true},
                              {{2000, -3000, 1500}, true}, {{1024, -2048, 512}, true}, {{2048, -4096, 1024}, true}, {{3000, 0, 0}, true}};
    long lost_all = 0, member_all = 0, floor_failures = 0;
    for (const Offset &oc : offsets) {
        double big = 0.0;
        for (int q = 0; q < 3; ++q) big = std::fmax(big, std::fabs(oc.off[q]) + 1.0);
        const double band = 4.0 * std::ldexp(1.0, (int)std::floor(std::log2(big)) - 23);   // four ulp of the largest coordinate
        for (int pl = 0; pl < NPLAN; ++pl) {
            Tally by_ell[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, all = {0, 0, 0, 0};
            for (long trial = 0; trial < trials; ++trial) {
                bool reuse = false, member = false, lost = false;
                int bucket = 0;
                if (pl == YY || pl == YY_ASYNC) trial_yy(pl, oc, band, trial, reuse, member, lost);
                else bucket = trial_xy(pl, oc, band, trial, reuse, member, lost);
                Tally *t[2] = {&by_ell[bucket], &all};
                for (Tally *y : t) { y->trials += 1; y->reuse += reuse; y->member += reuse && member; y->lost += lost; }
            }
            for (int k = 0; k < 4; ++k) {
                if (!by_ell[k].trials) continue;
                char ell[32];
                if (pl == YY || pl == YY_ASYNC) std::snprintf(ell, sizeof(ell), "0.039-0.19");
                else std::snprintf(ell, sizeof(ell), "%.2f", (double)ELLS[k]);
                std::printf("offset (%g, %g, %g) plan %s ell %s: %ld trials, %ld re-use, %ld with a member under re-use, %ld lost\n", oc.off[0], oc.off[1],
                            oc.off[2], plan_name[pl], ell, by_ell[k].trials, by_ell[k].reuse, by_ell[k].member, by_ell[k].lost);
            }
            if (10 * all.reuse < 9 * all.trials) {
                std::printf("  FLOOR offset (%g, %g, %g) plan %s: only %ld of %ld trials re-use\n", oc.off[0], oc.off[1], oc.off[2], plan_name[pl], all.reuse, all.trials);
                ++floor_failures;
            }
            if (oc.far && all.member < 200) {
                std::printf("  FLOOR offset (%g, %g, %g) plan %s: only %ld trials with a member under a re-used list\n", oc.off[0], oc.off[1], oc.off[2],
                            plan_name[pl], all.member);
                ++floor_failures;
            }
            lost_all += all.lost;
            member_all += all.member;
        }
    }
    std::printf("travel bounds: %ld failed of %ld\n", travel_failures, travel_checks);
    std::printf("floors missed: %ld\n", floor_failures);
    std::printf("lost %ld of %ld\n", lost_all, member_all);
    return (lost_all || travel_failures || floor_failures) ? 1 : 0;
}
