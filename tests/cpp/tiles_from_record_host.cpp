// Host-only check of the tile list rebuilt from its candidate record (csrc/cvo_device.h record_covers_its_radius, plan_lists with
// DevParams::list_stale_engine; csrc/cvo_kernels.hip kt_tiles_from_record): the model of tests/cpp/plan_lists_host.cpp -- the plan of
// the synchronous xy list stepped through cvo's length-scale schedule with a synthetic motion, a tile list and a candidate record kept
// as pair sets on two small clouds in float64 -- with what an engine does when its launch geometry changes: the plan of the
// iteration that begins has been made (a narrowing may be named and the record's radius and pose already be the new ones while the
// record in memory is still the old one), and where the record covers its radius the tile list BECOMES the record's pair set and takes
// the record's radius and pose.  The flow pass then expands that list.  In every iteration the record and the tile list must hold
// every pair with d < sqrt(tau) at the current pose, and the slots of an engine must narrow at every drop of the length scale.
//   tiles_from_record_host     prints one line per case, exit status 0 = all assertions held
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "cvo_device.h"

using namespace cvo_dev;

namespace {
struct P3 { double x, y, z; };
typedef std::set<std::pair<int, int>> PairSet;

unsigned long long rng_state = 88172645463325252ull;
double rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

// inverse transform [Rt | t] of a rotation by `ang` about a fixed axis and a translation
void make_pose(double ang, const double tr[3], float Rt[9], float t[3])
{
    const double ax[3] = {0.26726124, 0.53452248, 0.80178373};
    const double c = std::cos(ang), s = std::sin(ang), v = 1.0 - c;
    double R[9] = {c + ax[0] * ax[0] * v, ax[0] * ax[1] * v - ax[2] * s, ax[0] * ax[2] * v + ax[1] * s,
                   ax[1] * ax[0] * v + ax[2] * s, c + ax[1] * ax[1] * v, ax[1] * ax[2] * v - ax[0] * s,
                   ax[2] * ax[0] * v - ax[1] * s, ax[2] * ax[1] * v + ax[0] * s, c + ax[2] * ax[2] * v};
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) Rt[3 * r + q] = (float)R[3 * q + r];
    for (int r = 0; r < 3; ++r) t[r] = (float)(-(R[0 + r] * tr[0] + R[3 + r] * tr[1] + R[6 + r] * tr[2]));
}

double dist(const P3 &x, const P3 &y0, const float Rt[9], const float t[3])
{
    const double yx = (double)Rt[0] * y0.x + (double)Rt[1] * y0.y + (double)Rt[2] * y0.z + (double)t[0];
    const double yy = (double)Rt[3] * y0.x + (double)Rt[4] * y0.y + (double)Rt[5] * y0.z + (double)t[1];
    const double yz = (double)Rt[6] * y0.x + (double)Rt[7] * y0.y + (double)Rt[8] * y0.z + (double)t[2];
    return std::sqrt((x.x - yx) * (x.x - yx) + (x.y - yy) * (x.y - yy) + (x.z - yz) * (x.z - yz));
}

struct Result { int builds, narrowings, reexpansions, rebuilds, refused, failures; };

// far: the moving cloud starts far from its final pose (large early travel); regeom_every: the launch geometry changes every so many iterations
Result run_case(float margin, bool far, int regeom_every, bool rebuild, int iters)
{
    const int N = 260;
    std::vector<P3> X(N), Y(N);
    rng_state = 88172645463325252ull;
    double cx[3] = {0.3, -0.2, 1.5};
    float xmax = 0.0f, ymax = 0.0f;
    for (int i = 0; i < N; ++i) {   // two noisy copies of a patch of surface about 1.2 m across
        const double u = rnd() * 1.2 - 0.6, v = rnd() * 1.2 - 0.6, w = 0.05 * std::sin(5.0 * u) + 0.02 * rnd();
        X[i] = {cx[0] + u, cx[1] + v, cx[2] + w};
        Y[i] = {cx[0] + u + 0.01 * (rnd() - 0.5), cx[1] + v + 0.01 * (rnd() - 0.5), cx[2] + w + 0.01 * (rnd() - 0.5)};
        const double dx = std::sqrt(u * u + v * v + w * w) + 0.02;
        if ((float)dx > xmax) xmax = (float)dx;
    }
    ymax = xmax;

    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.mode = CVO_HIP_MODE_CVO;
    p.max_iter = iters;
    p.sp = 8.0e-3f;
    p.log_sp_s2 = (float)std::log(8.0e-3 / 0.01);
    p.c = p.d = 7.0f; p.c_ell = 200.0f;
    p.list_margin = margin;
    p.record_narrow = 1;
    p.list_stale_max = 3.0f;
    p.list_stale_engine = rebuild ? 1.0e6f : 0.0f;   // (what loop_params gives the slots of an engine)
    p.s2_d = 0.01; p.cs2_d = 1.0;

    DevHead s;
    std::memset(&s, 0, sizeof(s));
    for (int q = 0; q < 3; ++q) s.center[q] = (float)cx[q];
    s.xmax = xmax; s.y0max = ymax;

    PairSet tiles, record;
    const int NBLK_A = 64, NBLK_B = 32;
    int nblk = NBLK_A;
    Result res = {0, 0, 0, 0, 0, 0};
    float ell = 0.15f;
    for (int k = 0; k < iters; ++k) {
        // the pose of iteration k: a decaying offset from the final pose (a registration converging)
        const double a0 = far ? 0.12 : 0.02, t0 = far ? 0.25 : 0.03;
        const double decay = std::exp(-0.18 * k);
        const double tr[3] = {t0 * decay, -0.6 * t0 * decay, 0.3 * t0 * decay};
        make_pose(a0 * decay, tr, s.Rt, s.t);
        const KernConsts kc = make_kconsts(p, ell);
        s.kc.tau = kc.tau;
        for (int l = 0; l < 3; ++l) s.tauf[l] = kc.tau;
        const float r_now = std::sqrt(kc.tau);
        const int stat_before[3] = {s.list_stat[0], s.list_stat[1], s.list_stat[2]};
        const float rec_r_before = s.rec_r;
        plan_lists(&s, &s, true, p, r_now);
        const bool built = s.reuse[LIST_XY] == 0;
        const bool narrowing = (s.narrow & REC_NARROW) != 0;
        if (built != (s.list_stat[0] == stat_before[0] + 1)) { std::printf("  k=%d: build not counted\n", k); ++res.failures; }
        if (narrowing != (s.list_stat[1] == stat_before[1] + 1)) { std::printf("  k=%d: narrowing not counted\n", k); ++res.failures; }
        if (built && narrowing) { std::printf("  k=%d: build and narrowing named together\n", k); ++res.failures; }
        if (narrowing && !(s.rec_r < rec_r_before)) { std::printf("  k=%d: a narrowing that does not narrow\n", k); ++res.failures; }
        // ---- the engine's geometry changed behind the last iteration: in front of this iteration's launches the list is rebuilt from the
        // record as it stands in memory (kt_tiles_from_record; a slot whose plan builds has no record: ck_nblk = 0)
        if (rebuild && s.ck_nblk[LIST_XY] != 0 && s.ck_nblk[LIST_XY] != nblk && s.list_ok[LIST_XY]) {
            if (record_covers_its_radius(&s)) {
                tiles = record;
                s.list_r[LIST_XY] = s.rec_r;
                for (int q = 0; q < 9; ++q) s.list_Rt[q] = s.rec_Rt[q];
                for (int q = 0; q < 3; ++q) s.list_t[q] = s.rec_t[q];
                ++res.rebuilds;
            } else {
                ++res.refused;
            }
        }
        // ---- what the kernels do with the plan
        if (built) {   // k_filter: every pair within list_r at this pose (it is conservative: a superset would do as well)
            tiles.clear();
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j)
                    if (dist(X[i], Y[j], s.Rt, s.t) < (double)s.list_r[LIST_XY]) tiles.insert({i, j});
        }
        const bool bounded = (s.narrow & REC_BOUNDED) != 0;
        const bool expand = s.ck_nblk[LIST_XY] != nblk;   // process_body: no record of this geometry
        if (expand) {
            record.clear();
            for (const auto &pr : tiles)
                if (!bounded || dist(X[pr.first], Y[pr.second], s.Rt, s.t) < (double)s.rec_r) record.insert(pr);
        } else if (narrowing) {
            PairSet kept;
            for (const auto &pr : record)
                if (dist(X[pr.first], Y[pr.second], s.Rt, s.t) < (double)s.rec_r) kept.insert(pr);
            record.swap(kept);
        }
        // ---- the check: every member of A is a candidate of the pass, and of an expansion that may come
        int missing_rec = 0, missing_tile = 0;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                if (dist(X[i], Y[j], s.Rt, s.t) < (double)r_now) {
                    if (!record.count({i, j})) ++missing_rec;
                    if (!tiles.count({i, j})) ++missing_tile;
                }
        if (missing_rec || missing_tile) {
            std::printf("  k=%d ell=%.2f: %d members missing from the record, %d from the tile list (reuse %d narrow %d rec_r %.5f list_r %.5f)\n", k,
                        ell, missing_rec, missing_tile, s.reuse[LIST_XY], s.narrow, s.rec_r, s.list_r[LIST_XY]);
            ++res.failures;
        }
        // ---- the post kernel (head_plan): the record now matches this geometry; an expansion of a bounded record moves its pose
        if (expand) {
            if (s.reuse[LIST_XY]) s.list_stat[2] += 1;
            if (bounded) {
                for (int q = 0; q < 9; ++q) s.rec_Rt[q] = s.Rt[q];
                for (int q = 0; q < 3; ++q) s.rec_t[q] = s.t[q];
            }
        }
        s.ck_nblk[LIST_XY] = nblk;
        if (regeom_every > 0 && k % regeom_every == regeom_every - 1) nblk = nblk == NBLK_A ? NBLK_B : NBLK_A;
        // cvo's schedule (ref src/cvo.cpp:408-410)
        ell = (k > 2) ? 0.10f : ell;
        ell = (k > 9) ? 0.06f : ell;
        ell = (k > 19) ? 0.03f : ell;
    }
    res.builds = s.list_stat[0]; res.narrowings = s.list_stat[1]; res.reexpansions = s.list_stat[2];
    return res;
}
}   // namespace

int main()
{
    int failures = 0;
    struct Case { float margin; bool far; int regeom; };
    const Case cases[] = {{0.25f, false, 5}, {0.25f, true, 7}, {0.15f, false, 6}, {0.25f, false, 3}, {0.25f, true, 3}, {0.05f, false, 4},
                          {0.05f, true, 5}, {0.5f, false, 11}, {0.5f, true, 2}, {0.25f, false, 1}, {0.25f, true, 1}};
    int rebuilds = 0;
    for (const Case &c : cases) {
        const Result off = run_case(c.margin, c.far, c.regeom, false, 40);
        const Result on = run_case(c.margin, c.far, c.regeom, true, 40);
        std::printf("margin %.2f far %d regeom %d  kept: builds %d narrowings %d re-expansions %d failures %d   rebuilt: builds %d narrowings %d "
                    "re-expansions %d rebuilds %d refused %d failures %d\n", c.margin, (int)c.far, c.regeom, off.builds, off.narrowings, off.reexpansions,
                    off.failures, on.builds, on.narrowings, on.reexpansions, on.rebuilds, on.refused, on.failures);
        failures += off.failures + on.failures;
        rebuilds += on.rebuilds;
        if (off.rebuilds != 0) { std::printf("  rebuilds without the option\n"); ++failures; }
        // a quiet registration with the default margin or more: every drop of the length scale narrows -- the drop to 0.03 too, which builds
        // while the list is kept -- and a narrowing only ever replaces a build.  (With a thin margin or a far start a rebuilt list, tight
        // around its record, has less room to travel in than the wide one it replaces, and travel may build once more: performance only.)
        if (c.margin >= 0.25f && !c.far && (on.narrowings < 3 || on.builds > off.builds)) { std::printf("  expected every drop to narrow\n"); ++failures; }
    }
    if (rebuilds == 0) { std::printf("no case rebuilt a list\n"); ++failures; }
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
