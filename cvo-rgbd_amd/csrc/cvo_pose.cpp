// cvo_pose.cpp -- the pose queries of include/cvo_hip.h: cvo_hip_pose_hessian, cvo_hip_pose_score (and _score_many),
// cvo_hip_pose_scan, cvo_hip_pose_matches.  All but the scan put the context at a pose, rebuild A there as cvo_hip_flow keeps
// it (filter + PROC_FLOW, which records the kept list, + POST_REDUCE) and stream the kept list back (KeptView) with a
// kernel of their own; score, scan and matches stage through pinned memory and wait once.
#include "cvo_internal.h"

using namespace cvo_dev;
using namespace cvo_impl;

// ---- cvo_hip_pose_score (include/cvo_hip.h)
// Pinned staging of a context's score: its three passes go out back to back, each with its own image of the state
// fields it pushes and its own words to come back, so that a call -- or a batch of contexts -- waits once, at the end.
struct ScorePin {
    DevHead img[3];        // the state in front of pass p (0: the fixed cloud against itself, 1: the moving one, 2: the pose)
    double red[3][9];      // RED_FLOW .. RED_FLOW + 8 after pass p: [6] sum a, [8] members
    uint32_t ovf[3][16];   // DevState::ovf after pass p
    double out[3];         // k_pose_score_reduce: sum a d2, fixed rows matched, moving rows matched
};
static_assert(offsetof(DevState, xi) <= sizeof(DevHead) && offsetof(DevState, done) + sizeof(int32_t) <= sizeof(DevHead),
              "the pushed fields are fields of the head");

namespace cvo_impl {
namespace {

enum { kScoreFixed = 0, kScoreMoving = 1, kScorePose = 2 };

struct ScoreJob {
    float R[9], T[3], ell;
    bool self_pass[2];   // the norm of the fixed / moving cloud is computed (not the cloud's cached one)
};

bool self_norm_valid(const cvo_hip_ctx *ctx, const Cloud &c, float ell)
{
    uint32_t bits;
    std::memcpy(&bits, &ell, sizeof(bits));
    return c.self.valid && c.self.gen == c.gen && c.self.ell_bits == bits &&
           std::memcmp(&c.self.prm, &ctx->prm, sizeof(cvo_hip_params)) == 0;
}

// Everything a score is refused for, checked before anything is enqueued.
int score_check(cvo_hip_ctx *ctx, const char *who, const float *R, const float *T, float ell, const void *out)
{
    auto refuse = [&](const char *why) { return fail(ctx, CVO_HIP_ERR_INVALID, (std::string(who) + why).c_str()); };
    if (!R || !T || !out) return refuse(": null argument");
    if (!(std::isfinite(ell) && ell > 0.0f))
        return refuse(": ell must be finite and > 0");
    if (ctx->fixed.n <= 0 || ctx->moving.n <= 0)
        return refuse(": both clouds must be set");
    if (ctx->sharded && (ctx->row_lo > 0 || ctx->row_hi < ctx->fixed.n || ctx->srow_lo > 0 || ctx->srow_hi < ctx->moving.n))
        return refuse(": not on a sharded context (the overlap counts do not add up over shards)");
    if (multi_rank(ctx) || ctx->mailbox)
        return refuse(": not with a communicator, mailboxes or an all-reduce hook attached");
    return CVO_HIP_OK;
}

// The host's state image at pose (R, T) ...
void pose_set(cvo_hip_ctx *ctx, const float *R, const float *T)
{
    DevState *h = &ctx->st_host[kPollSlots];
    std::memcpy(h->R, R, sizeof(h->R));
    std::memcpy(h->T, T, sizeof(h->T));
    cvo_math::inverse_tf(R, T, h->Rt, h->t);
}

// ... and with the kernel constants of `ell`, the filter geometry of the context's clouds and its bounds (self: a cloud
// against itself, untransformed)
int pass_consts(cvo_hip_ctx *ctx, float ell, bool self)
{
    DevState *h = &ctx->st_host[kPollSlots];
    h->done = 0;
    h->kc = make_kconsts(ctx->dprm, ell);
    h->kc_ell = -1.0f;   // (never equal to an ell: prepare_iteration recomputes)
    const int rc = fill_filter_geometry(ctx, h);
    if (rc) return rc;
    compute_filter_bounds(h, self);
    return CVO_HIP_OK;
}

int pose_begin(cvo_hip_ctx *ctx, const float *R, const float *T, float ell)
{
    pose_set(ctx, R, T);
    return pass_consts(ctx, ell, false);
}

// One pass: the state fields of the host image, then the filter and PROC_FLOW over rows [rlo, rhi) of ca against cb
// (cb under [Rt|t] if tf_b) and POST_REDUCE -- cvo_hip_flow's member set and sums; the sums and the overflow flags
// go to pinned words of the pass's own.
int score_pass(cvo_hip_ctx *ctx, int p, const Cloud &ca, int rlo, int rhi, const Cloud &cb, int tf_b)
{
    if (!ctx->score_pin) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->score_pin, sizeof(ScorePin), hipHostMallocDefault));
    ScorePin *pin = ctx->score_pin;
    std::memcpy(static_cast<void *>(&pin->img[p]), static_cast<const void *>(&ctx->st_host[kPollSlots]), sizeof(DevHead));
    const char *dev = reinterpret_cast<const char *>(ctx->st);
    int rc = push_pose_fields(ctx, &pin->img[p], true);
    if (!rc) rc = zero_counters(ctx);
    if (!rc) rc = enqueue_filter(ctx, LIST_XY, ca, rlo, rhi, 0, cb, tf_b, 0);
    if (!rc) rc = enqueue_process(ctx, PROC_FLOW, LIST_XY, ctx->part_flow, ca.pos, ca.feat, 0, cb.pos, cb.feat, tf_b, 0, 0);
    if (!rc) rc = enqueue_flow_reduce(ctx, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(pin->red[p], dev + offsetof(DevState, red) + RED_FLOW * sizeof(double), sizeof(pin->red[p]),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(pin->ovf[p], dev + offsetof(DevState, ovf), sizeof(pin->ovf[p]), hipMemcpyDeviceToHost,
                                ctx->stream));
    return CVO_HIP_OK;
}

// The norms |f_X|^2, |f_Y|^2 of a context's clouds (cvo_hip_pose_score's self_fixed / self_moving; cvo_hip_pose_scan's, the same
// passes and the same per-cloud cache): the self passes the clouds' cached norms do not cover, enqueued without a wait.
// Sets job.self_pass.
int self_norms_enqueue(cvo_hip_ctx *ctx, ScoreJob &job)
{
    job.self_pass[0] = !self_norm_valid(ctx, ctx->fixed, job.ell);
    job.self_pass[1] = !self_norm_valid(ctx, ctx->moving, job.ell);
    // A cloud against itself, untransformed: the cloud stands in as both clouds of the context for the pass, so that the
    // filter geometry, the kept-list sizes and the entry form are its own -- the same bits whichever side it is on
    // (the fixed cloud's norm after cvo_hip_swap_moving_to_fixed is the moving cloud's one frame earlier).  Only the
    // cloud's own rows are listed: the padding rows (cvo_cloud.h, NaN features) are never a row of the pass, and as
    // columns they lie ~10 km from every row.
    for (int s = 0; s < 2; ++s) {
        if (!job.self_pass[s]) continue;
        const Cloud keep_f = ctx->fixed, keep_m = ctx->moving;
        const Cloud c = s == 0 ? keep_f : keep_m;
        ctx->fixed = c;
        ctx->moving = c;
        int rc = pass_consts(ctx, job.ell, true);
        if (!rc) rc = score_pass(ctx, s, ctx->fixed, 0, c.n, ctx->moving, 0);
        ctx->fixed = keep_f;
        ctx->moving = keep_m;
        if (rc) return rc;
    }
    return CVO_HIP_OK;
}

// After the wait: pass p of the staging overflowed a tile or kept list -- the list grows and the caller enqueues again (*redo)
int score_pass_grow(cvo_hip_ctx *ctx, int p, const char *who, bool *redo)
{
    const ScorePin *pin = ctx->score_pin;
    for (int l = 0; l < LIST_N; ++l) {
        if (!(pin->ovf[p][l] | pin->ovf[p][8 + l])) continue;
        const uint32_t cap = ctx->lists[l].cap;
        int rc = ensure_list(ctx, l, 0, 0, std::min(4.0e9, 2.0 * (double)cap + 1024.0));
        if (rc) return rc;
        if (ctx->lists[l].cap <= cap) return fail(ctx, CVO_HIP_ERR_NOMEM, (std::string(who) + ": a list cannot grow further").c_str());
        ++ctx->list_grows;
        *redo = true;
    }
    return CVO_HIP_OK;
}

// ... and when none did: the norms the self passes computed go to their clouds
void self_norms_store(cvo_hip_ctx *ctx, const ScoreJob &job)
{
    const ScorePin *pin = ctx->score_pin;
    uint32_t bits;
    std::memcpy(&bits, &job.ell, sizeof(bits));
    for (int s = 0; s < 2; ++s) {
        if (!job.self_pass[s]) continue;
        Cloud &c = s == 0 ? ctx->fixed : ctx->moving;
        c.self.valid = true;
        c.self.gen = c.gen;
        c.self.prm = ctx->prm;
        c.self.ell_bits = bits;
        c.self.sum = pin->red[s][6];
        c.self.nnz = (int64_t)pin->red[s][8];
    }
}

// The pass at the job's pose, enqueued on the context's stream without a wait -- behind the self passes the clouds' cached
// norms do not cover, if the caller wants the norms.  The context ends as cvo_hip_transform_pcd(ctx, R, T) leaves it.
int pose_pass_enqueue(cvo_hip_ctx *ctx, ScoreJob &job, bool norms)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = cloud_ready(ctx, ctx->fixed);
    if (!rc) rc = cloud_ready(ctx, ctx->moving);
    if (rc) return rc;
    pose_set(ctx, job.R, job.T);
    if (norms) rc = self_norms_enqueue(ctx, job);
    // A at the pose exactly as cvo_hip_pose_hessian rebuilds it (the same filter and PROC_FLOW pass): last, so that the
    // kept list the caller's pass streams is its
    if (!rc) rc = pass_consts(ctx, job.ell, false);
    if (rc) return rc;
    int rlo, rhi, slo, shi;
    shard_ranges(ctx, rlo, rhi, slo, shi);
    return score_pass(ctx, kScorePose, ctx->fixed, rlo, rhi, ctx->moving, 1);
}

// A context's whole score, enqueued without a wait: the norms, the pass at the pose, the score pass over the pose's kept list.
int score_enqueue(cvo_hip_ctx *ctx, ScoreJob &job)
{
    int rc = pose_pass_enqueue(ctx, job, true);
    if (rc) return rc;
    const size_t flag_off = (size_t)(PROC_BLOCKS + 4) * sizeof(double);
    const size_t nflag = (size_t)ctx->fixed.np + (size_t)ctx->moving.np;   // (both multiples of CLOUD_PAD)
    rc = ensure_buf(ctx, ctx->part_score, flag_off + nflag);
    if (rc) return rc;
    char *ps = static_cast<char *>(ctx->part_score.p);
    HIP_TRY(ctx, hipMemsetAsync(ps + flag_off, 0, nflag, ctx->stream));
    ScoreArgs sa{};
    sa.pos_a = ctx->fixed.pos;
    sa.pos_b = ctx->moving.pos;
    sa.kept = kept_view(ctx);
    sa.partials = reinterpret_cast<double *>(ps);
    sa.out = sa.partials + PROC_BLOCKS;
    sa.flag_a = reinterpret_cast<uint8_t *>(ps + flag_off);
    sa.flag_b = sa.flag_a + ctx->fixed.np;
    sa.na = ctx->fixed.np;
    sa.nb = ctx->moving.np;
    launch_pose_score(sa, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->score_pin->out, sa.out, sizeof(ctx->score_pin->out), hipMemcpyDeviceToHost, ctx->stream));
    ctx->have_tf = true;
    return CVO_HIP_OK;
}

// After the wait: a pass whose tile or kept list overflowed grows that list and the score is enqueued again (*redo);
// otherwise the result, and the norms the self passes computed go to their clouds.
int score_collect(cvo_hip_ctx *ctx, const ScoreJob &job, cvo_hip_pose_score_t *out, bool *redo)
{
    const ScorePin *pin = ctx->score_pin;
    *redo = false;
    for (int p = 0; p < 3; ++p) {
        if (p < 2 && !job.self_pass[p]) continue;
        const int rc = score_pass_grow(ctx, p, "cvo_hip_pose_score", redo);
        if (rc) return rc;
    }
    if (*redo) return CVO_HIP_OK;
    self_norms_store(ctx, job);
    cvo_hip_pose_score_t r{};
    r.inner = pin->red[kScorePose][6];
    r.nnz = (int64_t)pin->red[kScorePose][8];
    r.self_fixed = ctx->fixed.self.sum;
    r.nnz_fixed = ctx->fixed.self.nnz;
    r.self_moving = ctx->moving.self.sum;
    r.nnz_moving = ctx->moving.self.nnz;
    r.cos_angle = (r.self_fixed > 0.0 && r.self_moving > 0.0) ? r.inner / std::sqrt(r.self_fixed * r.self_moving) : 0.0;
    r.mean_d2 = r.nnz > 0 ? pin->out[0] / r.inner : 0.0;
    r.fixed_matched = (int32_t)pin->out[1];
    r.moving_matched = (int32_t)pin->out[2];
    r.n_fixed = ctx->fixed.n;
    r.n_moving = ctx->moving.n;
    r.ell = job.ell;
    *out = r;
    if (ctx->profiling) return drain_events(ctx);
    return CVO_HIP_OK;
}

// The scores of `count` checked contexts: every chain is enqueued, then the streams are waited for, once.
int score_batch(cvo_hip_ctx *const *ctxs, const float *R9, const float *T3, const float *ell, cvo_hip_pose_score_t *out,
                int count)
{
    std::vector<ScoreJob> jobs((size_t)count);
    std::vector<char> todo((size_t)count, 1);
    for (int k = 0; k < count; ++k) {
        std::memcpy(jobs[k].R, R9 + 9 * (size_t)k, sizeof(jobs[k].R));
        std::memcpy(jobs[k].T, T3 + 3 * (size_t)k, sizeof(jobs[k].T));
        jobs[k].ell = ell[k];
    }
    for (bool any = true; any;) {
        for (int k = 0; k < count; ++k) {
            if (!todo[k]) continue;
            const int rc = score_enqueue(ctxs[k], jobs[k]);
            if (rc) return rc;
        }
        for (int k = 0; k < count; ++k)
            if (todo[k]) HIP_TRY(ctxs[k], hipStreamSynchronize(ctxs[k]->stream));
        any = false;
        for (int k = 0; k < count; ++k) {
            if (!todo[k]) continue;
            bool redo = false;
            const int rc = score_collect(ctxs[k], jobs[k], &out[k], &redo);
            if (rc) return rc;
            todo[k] = redo ? 1 : 0;
            any = any || redo;
        }
    }
    return CVO_HIP_OK;
}

// A pinned staging buffer of at least `bytes`, made with room to spare.  (The old one is freed as it stands: a caller whose
// buffer may still be the source of an enqueued copy waits for its stream first.)
int ensure_pinned(cvo_hip_ctx *ctx, PinBuf &b, size_t bytes, const char *who)
{
    if (bytes <= b.bytes) return CVO_HIP_OK;
    if (b.p) HIP_TRY(ctx, hipHostFree(b.p));
    b = PinBuf{};
    const size_t grown = bytes * 5 / 4 + 4096;
    if (hipHostMalloc(&b.p, grown, hipHostMallocDefault) != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return fail(ctx, CVO_HIP_ERR_NOMEM, (std::string(who) + ": no pinned memory for the staging").c_str());
    }
    b.bytes = grown;
    return CVO_HIP_OK;
}

// ---- cvo_hip_pose_scan (include/cvo_hip.h)
// Per pose: [Rt | t] as cvo_hip_transform_pcd makes it, and the two constants of the culling test of k_pose_scan
// (cvo_scan.hip scan_near): scale >= |Rt|_2 and reach = sqrt(tau) + slack.
//   scale: |Rt|_2^2 = lambda_max(Rt Rt^T) <= 1 + |Rt Rt^T - I|_F -- 1 + ~1e-7 for a float32 rotation, and a bound for any matrix.
//   slack: with u = 2^-24, X = the largest |coordinate| of the fixed cloud, Z of the moving cloud, S = 3 max|Rt| Z + max|t|:
//     every partial sum of a row of apply_tf is at most S, so its six roundings leave a component within 6 u S and the row
//     within 6 sqrt(3) u S < 11 u S of the exact image; the kernel's transformed centre likewise: 22 u S together.  The kernel's
//     left-hand side -- three differences of numbers up to X and S, their squares' sum, a square root, two subtractions of
//     radii no larger than the clouds -- is within 12 u sqrt(3) (X + S) of its exact value.  A member's computed d2 < tau
//     bounds the distance of the computed rows by sqrt(tau) (1 + 4 u).  Needed: below 34 u sqrt(3) (X + S) + 4 u sqrt(tau);
//     taken: 64 u sqrt(3) (X + S) + 1e-6 sqrt(tau), rounded up.  (1e-5 m for clouds 1.5 m from the origin: culling loses nothing.)
void scan_pose_consts(const float *R, const float *T, float tau, double xabs, double zabs, float *tf)
{
    cvo_math::inverse_tf(R, T, tf, tf + 9);
    double g2 = 0.0, rmax = 0.0, tmax = 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            double g = r == c ? -1.0 : 0.0;
            for (int q = 0; q < 3; ++q) g += (double)tf[3 * r + q] * (double)tf[3 * c + q];
            g2 += g * g;
            rmax = std::max(rmax, std::fabs((double)tf[3 * r + c]));
        }
        tmax = std::max(tmax, std::fabs((double)tf[9 + r]));
    }
    const double S = 3.0 * rmax * zabs + tmax;
    const double u = 1.0 / 16777216.0;
    const double rt = std::sqrt((double)tau);
    tf[12] = (float)(std::sqrt(1.0 + std::sqrt(g2)) * 1.000001);
    tf[13] = (float)((rt * 1.000001 + 64.0 * u * std::sqrt(3.0) * (xabs + S)) * 1.000001);
    tf[14] = tf[15] = 0.0f;
}

double cloud_abs_max(const Cloud &c)
{
    double m = 0.0;
    for (int a = 0; a < 3; ++a) m = std::max(m, std::max(std::fabs((double)c.lo[a]), std::fabs((double)c.hi[a])));
    return m;
}

// Pinned staging of a scan: the state image the winner's pose is pushed from, the chunk's poses going up, its sums coming back
struct ScanStage {
    DevHead *img;
    float *tf;       // [m][SCAN_TF]
    double *out;     // [m][3]
};
size_t scan_stage_off_tf() { return (sizeof(DevHead) + 63) & ~(size_t)63; }
size_t scan_stage_bytes(int m) { return scan_stage_off_tf() + (size_t)m * (SCAN_TF * sizeof(float) + 3 * sizeof(double)); }
ScanStage scan_stage(cvo_hip_ctx *ctx, int m)
{
    char *b = static_cast<char *>(ctx->scan_stage.p);
    ScanStage st;
    st.img = reinterpret_cast<DevHead *>(b);
    st.tf = reinterpret_cast<float *>(b + scan_stage_off_tf());
    st.out = reinterpret_cast<double *>(b + scan_stage_off_tf() + (size_t)m * SCAN_TF * sizeof(float));
    return st;
}

int scan_run(cvo_hip_ctx *ctx, const float *R9, const float *T3, int count, float ell, cvo_hip_pose_scan_entry *out,
             cvo_hip_pose_scan_t *summary)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = cloud_ready(ctx, ctx->fixed);
    if (!rc) rc = cloud_ready(ctx, ctx->moving);
    if (rc) return rc;
    const int chunk = ctx->opt.scan_chunk > 0 ? ctx->opt.scan_chunk : SCAN_CHUNK;
    const int m = std::max(1, std::min(count, chunk));   // poses per launch: what the buffers are sized for
    const int nseg_a = (ctx->fixed.n + SEG - 1) / SEG, nseg_b = (ctx->moving.n + SEG - 1) / SEG;
    const int nblk = (nseg_a + 3) / 4;
    if (scan_stage_bytes(m) > ctx->scan_stage.bytes)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the last scan's state image may still be on its way)
    rc = ensure_pinned(ctx, ctx->scan_stage, scan_stage_bytes(m), "cvo_hip_pose_scan");
    if (rc) return rc;
    const size_t dev_tf = (size_t)m * SCAN_TF * sizeof(float), dev_out = (size_t)m * 3 * sizeof(double);
    rc = ensure_buf(ctx, ctx->scan_dev, dev_tf + dev_out + (size_t)3 * nblk * m * sizeof(double));
    if (rc) return rc;
    const ScanStage st = scan_stage(ctx, m);
    // the norms: the passes and the per-cloud cache of cvo_hip_pose_score, in front of the first chunk and behind the same wait
    ScoreJob job{};
    job.ell = ell;
    rc = self_norms_enqueue(ctx, job);
    if (rc) return rc;
    ScanArgs sa{};
    sa.pos_a = ctx->fixed.pos;
    sa.feat_a = ctx->fixed.feat;
    sa.seg_a = ctx->fixed.seg;
    sa.pos_b = ctx->moving.pos;
    sa.feat_b = ctx->moving.feat;
    sa.seg_b = ctx->moving.seg;
    char *dev = static_cast<char *>(ctx->scan_dev.p);
    sa.tf = reinterpret_cast<const float *>(dev);
    sa.out = reinterpret_cast<double *>(dev + dev_tf);
    sa.partials = reinterpret_cast<double *>(dev + dev_tf + dev_out);
    sa.kc = make_kconsts(ctx->dprm, ell);
    sa.nseg_a = nseg_a;
    sa.nseg_b = nseg_b;
    sa.nblk = nblk;
    const int weight = ctx->prm.color_scale > 0.0f ? 1 : 0;   // (the MATLAB object's weight, as enqueue_process picks it)
    const double xabs = cloud_abs_max(ctx->fixed), zabs = cloud_abs_max(ctx->moving);
    bool norms_done = false;
    for (int k0 = 0; k0 < count || !norms_done; k0 += m) {
        const int nk = std::max(0, std::min(m, count - k0));
        if (nk > 0) {
            for (int k = 0; k < nk; ++k)
                scan_pose_consts(R9 + 9 * (size_t)(k0 + k), T3 + 3 * (size_t)(k0 + k), sa.kc.tau, xabs, zabs, st.tf + (size_t)k * SCAN_TF);
            HIP_TRY(ctx, hipMemcpyAsync(dev, st.tf, (size_t)nk * SCAN_TF * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            sa.count = nk;
            launch_pose_scan(sa, weight, ctx->stream);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(st.out, sa.out, (size_t)nk * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the chunk's one wait
        while (!norms_done) {   // (a self pass that overflowed a list: the list grows, the self passes alone go out again)
            bool redo = false;
            for (int p = 0; p < 2; ++p) {
                if (!job.self_pass[p]) continue;
                rc = score_pass_grow(ctx, p, "cvo_hip_pose_scan", &redo);
                if (rc) return rc;
            }
            if (!redo) {
                self_norms_store(ctx, job);
                norms_done = true;
                break;
            }
            rc = self_norms_enqueue(ctx, job);
            if (rc) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (int k = 0; k < nk; ++k) {
            cvo_hip_pose_scan_entry e{};
            e.inner = st.out[3 * (size_t)k];
            e.nnz = (int64_t)st.out[3 * (size_t)k + 2];
            e.mean_d2 = e.nnz > 0 ? st.out[3 * (size_t)k + 1] / e.inner : 0.0;
            out[k0 + k] = e;
        }
    }
    cvo_hip_pose_scan_t r{};
    r.self_fixed = ctx->fixed.self.sum;
    r.nnz_fixed = ctx->fixed.self.nnz;
    r.self_moving = ctx->moving.self.sum;
    r.nnz_moving = ctx->moving.self.nnz;
    r.count = count;
    r.best = -1;
    r.n_fixed = ctx->fixed.n;
    r.n_moving = ctx->moving.n;
    r.ell = ell;
    const bool normed = r.self_fixed > 0.0 && r.self_moving > 0.0;
    const double norm = normed ? std::sqrt(r.self_fixed * r.self_moving) : 1.0;
    double top = 0.0;
    for (int k = 0; k < count; ++k) {
        out[k].cos_angle = normed ? out[k].inner / norm : 0.0;
        if (out[k].nnz > 0 && (r.best < 0 || out[k].inner > top)) {   // the largest inner, the first of equals
            r.best = k;
            top = out[k].inner;
        }
    }
    *summary = r;
    if (r.best < 0) return ctx->profiling ? drain_events(ctx) : CVO_HIP_OK;
    // the context ends as cvo_hip_transform_pcd(ctx, R_best, T_best) leaves it.  The fields go up from the scan's own pinned image,
    // in stream order behind the scan and without a wait: the image is next written behind the next scan's wait.
    rc = pose_begin(ctx, R9 + 9 * (size_t)r.best, T3 + 3 * (size_t)r.best, ell);
    if (rc) return rc;
    std::memcpy(static_cast<void *>(st.img), static_cast<const void *>(&ctx->st_host[kPollSlots]), sizeof(DevHead));
    rc = push_pose_fields(ctx, st.img, false);
    if (rc) return rc;
    ctx->have_tf = true;
    return ctx->profiling ? drain_events(ctx) : CVO_HIP_OK;
}

// ---- cvo_hip_pose_matches (include/cvo_hip.h)
// Layout of one side's output arrays, on the device (after the accumulators) and in the pinned staging alike:
// support [n] float64, count [n] int32, best [n] int32, best_w [n] float32, the side padded to 16 bytes.
struct MatchSide {
    size_t off, support, count, best, best_w, bytes;
};
MatchSide match_side(size_t off, int n)
{
    MatchSide m;
    m.off = off;
    m.support = off;
    m.count = m.support + (size_t)n * sizeof(double);
    m.best = m.count + (size_t)n * sizeof(int32_t);
    m.best_w = m.best + (size_t)n * sizeof(int32_t);
    m.bytes = (((size_t)n * 20) + 15) & ~(size_t)15;
    return m;
}

// The pass at the pose (cvo_hip_pose_score's, without the self passes), the matches pass over its kept list, and the
// copies of what the caller wants into pinned memory; no wait.
int matches_enqueue(cvo_hip_ctx *ctx, ScoreJob &job, const bool want[2])
{
    int rc = pose_pass_enqueue(ctx, job, false);
    if (rc) return rc;
    const int na = ctx->fixed.np, nb = ctx->moving.np;
    const size_t acc_off = sizeof(MatchCounters);
    const size_t acc_bytes = ((size_t)na + (size_t)nb) * sizeof(MatchAcc);
    const MatchSide sd[2] = {match_side(acc_off + acc_bytes, ctx->fixed.n),
                             match_side(acc_off + acc_bytes + match_side(0, ctx->fixed.n).bytes, ctx->moving.n)};
    rc = ensure_buf(ctx, ctx->part_matches, sd[1].off + sd[1].bytes);
    if (rc) return rc;
    // pinned: the counters, then the sides that are wanted
    const size_t stage_off[2] = {sizeof(MatchCounters), sizeof(MatchCounters) + (want[0] ? sd[0].bytes : 0)};
    const size_t stage_bytes = stage_off[1] + (want[1] ? sd[1].bytes : 0);
    rc = ensure_pinned(ctx, ctx->match_stage, stage_bytes, "cvo_hip_pose_matches");
    if (rc) return rc;
    char *pm = static_cast<char *>(ctx->part_matches.p);
    HIP_TRY(ctx, hipMemsetAsync(pm, 0, acc_off + acc_bytes, ctx->stream));
    MatchArgs ma{};
    ma.feat_a = ctx->fixed.feat;
    ma.feat_b = ctx->moving.feat;
    ma.kept = kept_view(ctx);
    ma.counters = reinterpret_cast<MatchCounters *>(pm);
    ma.acc_a = reinterpret_cast<MatchAcc *>(pm + acc_off);
    ma.acc_b = ma.acc_a + na;
    for (int s = 0; s < 2; ++s) {
        ma.out[s].support = reinterpret_cast<double *>(pm + sd[s].support);
        ma.out[s].count = reinterpret_cast<int32_t *>(pm + sd[s].count);
        ma.out[s].best = reinterpret_cast<int32_t *>(pm + sd[s].best);
        ma.out[s].best_w = reinterpret_cast<float *>(pm + sd[s].best_w);
    }
    ma.na = na;
    ma.nb = nb;
    ma.n_fixed = ctx->fixed.n;
    ma.n_moving = ctx->moving.n;
    ma.blocks_a = (na + BLOCK - 1) / BLOCK;
    ma.blocks_b = (nb + BLOCK - 1) / BLOCK;
    launch_pose_matches(ma, ctx->opt.matches_combine, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    char *stage = static_cast<char *>(ctx->match_stage.p);
    HIP_TRY(ctx, hipMemcpyAsync(stage, pm, sizeof(MatchCounters), hipMemcpyDeviceToHost, ctx->stream));
    for (int s = 0; s < 2; ++s)
        if (want[s] && sd[s].bytes)
            HIP_TRY(ctx, hipMemcpyAsync(stage + stage_off[s], pm + sd[s].off, sd[s].bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->have_tf = true;
    return CVO_HIP_OK;
}

// After the wait: a tile or kept list that overflowed grows and the call is enqueued again (*redo), as score_collect
// does; otherwise the summary and the caller's arrays.
int matches_collect(cvo_hip_ctx *ctx, const ScoreJob &job, const cvo_hip_point_matches *const side[2],
                    cvo_hip_pose_matches_t *summary, bool *redo)
{
    const ScorePin *pin = ctx->score_pin;
    *redo = false;
    const int rc = score_pass_grow(ctx, kScorePose, "cvo_hip_pose_matches", redo);
    if (rc || *redo) return rc;
    const char *stage = static_cast<const char *>(ctx->match_stage.p);
    MatchCounters cnt;
    std::memcpy(&cnt, stage, sizeof(cnt));
    cvo_hip_pose_matches_t r{};
    r.inner = pin->red[kScorePose][6];
    r.nnz = (int64_t)pin->red[kScorePose][8];
    r.n_fixed = ctx->fixed.n;
    r.n_moving = ctx->moving.n;
    r.fixed_matched = (int32_t)cnt.matched_a;
    r.moving_matched = (int32_t)cnt.matched_b;
    r.ell = job.ell;
    r.exact = cnt.inexact == 0 ? 1 : 0;
    *summary = r;
    size_t off = sizeof(MatchCounters);
    for (int s = 0; s < 2; ++s) {
        if (!side[s]) continue;
        const int n = s == 0 ? ctx->fixed.n : ctx->moving.n;
        const MatchSide m = match_side(off, n);
        if (side[s]->support) std::memcpy(side[s]->support, stage + m.support, (size_t)n * sizeof(double));
        if (side[s]->count) std::memcpy(side[s]->count, stage + m.count, (size_t)n * sizeof(int32_t));
        if (side[s]->best) std::memcpy(side[s]->best, stage + m.best, (size_t)n * sizeof(int32_t));
        if (side[s]->best_w) std::memcpy(side[s]->best_w, stage + m.best_w, (size_t)n * sizeof(float));
        off += m.bytes;
    }
    if (ctx->profiling) return drain_events(ctx);
    return CVO_HIP_OK;
}

}   // namespace
}   // namespace cvo_impl

extern "C" {

int cvo_hip_pose_hessian(cvo_hip_ctx *ctx, const float R[9], const float T[3], float ell,
                         cvo_hip_pose_hessian_t *out)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!R || !T || !out) return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_hessian: null argument");
    if (!(std::isfinite(ell) && ell > 0.0f))
        return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_hessian: ell must be finite and > 0");
    if (ctx->fixed.n <= 0 || ctx->moving.n <= 0)
        return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_hessian: both clouds must be set");
    if (multi_rank(ctx) || ctx->mailbox)
        return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_hessian: not with a communicator, mailboxes or an all-reduce "
                                              "hook attached (sums over ranks are the caller's)");
    int rc = cvo_hip_transform_pcd(ctx, R, T);
    if (rc) return rc;
    rc = pass_consts(ctx, ell, false);
    if (!rc) rc = push_state_fields(ctx, offsetof(DevState, kc), offsetof(DevState, xi) - offsetof(DevState, kc));
    if (rc) return rc;
    // A and its weights exactly as cvo_hip_flow keeps them: filter + PROC_FLOW, which records the kept list
    // (outside the loop the flow pass sums a: ProcessArgs::need_d2)
    int rlo, rhi, slo, shi;
    shard_ranges(ctx, rlo, rhi, slo, shi);
    for (bool redo = true; redo;) {
        rc = zero_counters(ctx);
        if (!rc) rc = enqueue_filter(ctx, LIST_XY, ctx->fixed, rlo, rhi, 0, ctx->moving, 1, 0);
        if (!rc) rc = enqueue_process(ctx, PROC_FLOW, LIST_XY, ctx->part_flow, ctx->fixed.pos,
                                      ctx->fixed.feat, 0, ctx->moving.pos, ctx->moving.feat, 1, 0, 0);
        if (!rc) rc = check_overflow_and_grow(ctx, &redo);
        if (rc) return rc;
    }
    // f and nnz: the flow partials reduced as cvo_hip_function_inner_product reduces them;
    // the Hessian pass over the kept list, then its fixed-order reduction
    rc = enqueue_flow_reduce(ctx, nullptr);
    if (!rc) rc = ensure_buf(ctx, ctx->part_hess, (size_t)(PROC_BLOCKS + 1) * NACC_HESS * sizeof(double));
    if (rc) return rc;
    HessArgs ha{};
    ha.pos_a = ctx->fixed.pos;
    ha.pos_b = ctx->moving.pos;
    ha.kept = kept_view(ctx);
    ha.partials = (double *)ctx->part_hess.p;
    ha.out = ha.partials + (size_t)PROC_BLOCKS * NACC_HESS;
    ha.inv_l2 = 1.0f / (ell * ell);
    ha.inv_l = 1.0f / ell;
    launch_pose_hessian(ha, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    double sums[NACC_HESS];
    HIP_TRY(ctx, hipMemcpyAsync(sums, ha.out, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
    double red[9];
    rc = fetch_red(ctx, RED_FLOW, 9, red);   // (synchronises the stream)
    if (rc) return rc;
    cvo_hip_pose_hessian_t r{};
    r.f = red[6];
    r.nnz = (int64_t)red[8];
    r.ell = ell;
    for (int k = 0; k < 6; ++k) r.g[k] = sums[k];
    for (int k = 0, q = 6; k < 6; ++k)
        for (int l = k; l < 6; ++l, ++q) r.H[6 * k + l] = r.H[6 * l + k] = sums[q];
    *out = r;
    if (ctx->profiling) return drain_events(ctx);
    return CVO_HIP_OK;
}

int cvo_hip_pose_score(cvo_hip_ctx *ctx, const float R[9], const float T[3], float ell, cvo_hip_pose_score_t *out)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    int rc = score_check(ctx, "cvo_hip_pose_score", R, T, ell, out);
    if (rc) return rc;
    return score_batch(&ctx, R, T, &ell, out, 1);
}

int cvo_hip_pose_score_many(cvo_hip_ctx *const *ctxs, const float *R9, const float *T3, const float *ell,
                            cvo_hip_pose_score_t *out, int count)
{
    cvo_lock::Api api_guard;
    if (count < 0) return CVO_HIP_ERR_INVALID;
    if (count == 0) return CVO_HIP_OK;
    if (!ctxs || !R9 || !T3 || !ell || !out) return CVO_HIP_ERR_INVALID;
    // (every context and argument before any context is touched)
    for (int k = 0; k < count; ++k) {
        if (!ctxs[k] || ctxs[k]->device != ctxs[0]->device) return CVO_HIP_ERR_INVALID;
        for (int q = 0; q < k; ++q)
            if (ctxs[q] == ctxs[k]) return fail(ctxs[0], CVO_HIP_ERR_INVALID, "cvo_hip_pose_score_many: a context twice");
    }
    for (int k = 0; k < count; ++k) {
        const int rc = score_check(ctxs[k], "cvo_hip_pose_score", R9 + 9 * (size_t)k, T3 + 3 * (size_t)k, ell[k], out + k);
        if (rc) return rc;
    }
    return score_batch(ctxs, R9, T3, ell, out, count);
}

int cvo_hip_pose_scan(cvo_hip_ctx *ctx, const float *R9, const float *T3, int count, float ell, cvo_hip_pose_scan_entry *out,
                      cvo_hip_pose_scan_t *summary)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (count < 0 || count > (1 << 20)) return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_scan: count must be 0 .. 2^20");
    if (count == 0 && !summary) return CVO_HIP_OK;
    const void *some = ctx;   // (count == 0: no arrays to hand over)
    int rc = score_check(ctx, "cvo_hip_pose_scan", count ? R9 : (const float *)some, count ? T3 : (const float *)some, ell,
                         (count && !out) ? nullptr : (const void *)summary);
    if (rc) return rc;
    if (ctx->fixed.n > SCAN_MAX_POINTS || ctx->moving.n > SCAN_MAX_POINTS)
        return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_scan: a cloud of more than 65536 points");
    for (size_t q = 0; q < (size_t)count * 9; ++q)
        if (!std::isfinite(R9[q])) return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_scan: a non-finite entry in R9");
    for (size_t q = 0; q < (size_t)count * 3; ++q)
        if (!std::isfinite(T3[q])) return fail(ctx, CVO_HIP_ERR_INVALID, "cvo_hip_pose_scan: a non-finite entry in T3");
    return scan_run(ctx, R9, T3, count, ell, out, summary);
}

int cvo_hip_pose_matches(cvo_hip_ctx *ctx, const float R[9], const float T[3], float ell,
                         const cvo_hip_point_matches *fixed, const cvo_hip_point_matches *moving,
                         cvo_hip_pose_matches_t *summary)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    int rc = score_check(ctx, "cvo_hip_pose_matches", R, T, ell, summary);
    if (rc) return rc;
    ScoreJob job{};
    std::memcpy(job.R, R, sizeof(job.R));
    std::memcpy(job.T, T, sizeof(job.T));
    job.ell = ell;
    const cvo_hip_point_matches *const side[2] = {fixed, moving};
    // (a side none of whose arrays is wanted costs no copy back either)
    const bool want[2] = {fixed && (fixed->support || fixed->count || fixed->best || fixed->best_w),
                          moving && (moving->support || moving->count || moving->best || moving->best_w)};
    const cvo_hip_point_matches *const copy[2] = {want[0] ? side[0] : nullptr, want[1] ? side[1] : nullptr};
    for (bool redo = true; redo;) {
        rc = matches_enqueue(ctx, job, want);
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        rc = matches_collect(ctx, job, copy, summary, &redo);
        if (rc) return rc;
    }
    return CVO_HIP_OK;
}

}   // extern "C"
