// cvo_fe_settings.cpp -- the settings of a front-end context (include/cvo_frontend.h): what each accepts, its setter
// and its getter.  No kernel is launched here.  Every setter has one shape:
//
//     setter_begin      a context, and no frame in flight
//     the rule          cvo_fe_rules.h's sentence, "set_x: " in front
//     its refusals      which other settings stand against it, in a fixed order
//     same_setting      both absent, or the bytes in force again: nothing to do
//     its buffers       built in locals, so that a failure leaves the context as it was
//     settle            the stream idle: nothing reads what the old graphs read
//     hand_over, store_setting, what it releases, drop_graphs
//
// What each setter keeps and releases when it is cleared differs on purpose; DESIGN.md 4.9 has the table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_fe_ctx.h"
#include "cvo_fe_rules.h"
#include "cvo_lidar.h"
#include "cvo_lock.h"
#include "cvo_unpack.h"

using namespace cvo_fe;
namespace rules = cvo_fe_rules;

namespace cvo_fe_rules __attribute__((visibility("hidden"))) {

// what cvo_fe_set_camera accepts
bool model_ok(const cvo_fe_camera_model &m)
{
    const float v[10] = {m.depth_scale, m.fx, m.fy, m.cx, m.cy, m.dist[0], m.dist[1], m.dist[2], m.dist[3], m.dist[4]};
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return m.depth_scale > 0.0f && m.fx > 0.0f && m.fy > 0.0f;
}

// a rotation, as a depth camera's and a stereo rig's must be: within 1e-3 (largest absolute entry of R R^T - I) of
// orthonormal, with a positive determinant
bool rotation_ok(const float Rf[9])
{
    double R[9];
    for (int q = 0; q < 9; ++q) R[q] = (double)Rf[q];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2];
            if (!(std::fabs(e - (i == j ? 1.0 : 0.0)) <= 1e-3)) return false;
        }
    const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;
}

// what cvo_fe_set_depth_camera accepts
bool rig_ok(const cvo_fe_depth_camera &r)
{
    if (r.width < 8 || r.width > 8192 || r.height < 8 || r.height > 8192) return false;
    const float *f = &r.depth_scale;   // the 24 floats after the two sizes
    static_assert(sizeof(cvo_fe_depth_camera) == 2 * sizeof(int32_t) + 24 * sizeof(float), "no padding");
    for (int q = 0; q < 24; ++q)
        if (!std::isfinite(f[q])) return false;
    if (!(r.depth_scale > 0.0f && r.fx > 0.0f && r.fy > 0.0f)) return false;
    if (r.max_range > 0.0f && r.max_range <= r.min_range) return false;
    return rotation_ok(r.R);
}

// what cvo_fe_set_stereo_rig accepts
bool srig_ok(const cvo_fe_stereo_rig &r)
{
    static_assert(sizeof(cvo_fe_lens) == 9 * sizeof(float), "36 bytes, no padding");
    static_assert(sizeof(cvo_fe_stereo_rig) == 42 * sizeof(float), "168 bytes, no padding");
    const float *f = &r.left.fx;   // floats only
    for (int q = 0; q < 42; ++q)
        if (!std::isfinite(f[q])) return false;
    if (!(r.left.fx > 0.0f && r.left.fy > 0.0f && r.right.fx > 0.0f && r.right.fy > 0.0f && r.fx > 0.0f && r.fy > 0.0f))
        return false;
    if (!(r.depth_scale > 0.0f && r.baseline > 0.0f)) return false;
    return rotation_ok(r.R_left) && rotation_ok(r.R_right);
}

// what cvo_fe_set_lidar accepts
bool lidar_ok(const cvo_fe_lidar &l)
{
    static_assert(sizeof(cvo_fe_lidar) == 5 * sizeof(int32_t) + 15 * sizeof(float), "80 bytes, no padding");
    if (l.max_points < 1 || l.max_points > FE_LIDAR_MAX_POINTS || l.splat < 0 || l.splat > 3) return false;
    const float *f = l.R;   // the 15 floats after the two sizes
    for (int q = 0; q < 15; ++q)
        if (!std::isfinite(f[q])) return false;
    if (l.occl_rel < 0.0f) return false;
    if (l.occl_rx < 0 || l.occl_rx > FE_LIDAR_RMAX || l.occl_ry < 0 || l.occl_ry > FE_LIDAR_RMAX) return false;
    if (l.max_range > 0.0f && l.max_range <= l.min_range) return false;
    return rotation_ok(l.R) && l.pad_ == 0;
}

// what cvo_fe_set_lidar_sweep accepts
bool sweep_ok(const cvo_fe_lidar_sweep &sw)
{
    static_assert(sizeof(cvo_fe_lidar_sweep) == 32, "32 bytes, no padding");
    if (!std::isfinite(sw.time_origin) || !std::isfinite(sw.time_scale) || !std::isfinite(sw.phase0) || !std::isfinite(sw.s_ref))
        return false;
    if (!(sw.s_ref >= 0.0f && sw.s_ref <= 1.0f) || sw.pad_ != 0) return false;
    if (sweep_field_mode(sw)) {
        if (sw.time_offset < 12 || sw.time_offset % 4 != 0 || sw.time_scale == 0.0f || sw.direction != 0) return false;
        return sw.mode == CVO_FE_SWEEP_TIME_F32 || sw.time_origin == 0.0f;
    }
    if (sw.mode != CVO_FE_SWEEP_AZIMUTH) return false;
    return (sw.direction == 1 || sw.direction == -1) && sw.phase0 >= 0.0f && sw.phase0 < 1.0f && sw.time_origin == 0.0f;
}

// what cvo_fe_set_lidar_motion accepts
bool twist_ok(const float twist[6])
{
    double w2 = 0.0, v2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(twist[k]) || !std::isfinite(twist[3 + k])) return false;
        w2 += (double)twist[k] * twist[k];
        v2 += (double)twist[3 + k] * twist[3 + k];
    }
    return w2 <= (double)CVO_FE_SWEEP_MAX_ROTATION * CVO_FE_SWEEP_MAX_ROTATION &&
           v2 <= (double)CVO_FE_SWEEP_MAX_TRANSLATION * CVO_FE_SWEEP_MAX_TRANSLATION;
}

// what cvo_fe_set_depth_gate accepts
bool gate_ok(const cvo_fe_depth_gate &g)
{
    static_assert(sizeof(cvo_fe_depth_gate) == 3 * sizeof(float) + 3 * sizeof(int32_t), "24 bytes, no padding");
    if (!std::isfinite(g.min_range) || !std::isfinite(g.max_range) || !std::isfinite(g.jump_rel)) return false;
    if (g.jump_rel < 0.0f) return false;
    if (g.max_range > 0.0f && g.max_range <= g.min_range) return false;
    if (g.grow < 0 || g.grow > FE_GATE_MAX_GROW) return false;
    return (g.hole_border == 0 || g.hole_border == 1) && g.pad_ == 0;
}

// what cvo_fe_set_stereo accepts
bool stereo_ok(const cvo_fe_stereo &s)
{
    static_assert(sizeof(cvo_fe_stereo) == sizeof(float) + 7 * sizeof(int32_t), "32 bytes, no padding");
    if (!std::isfinite(s.baseline) || !(s.baseline > 0.0f)) return false;
    if (s.max_disp < 8 || s.max_disp > 128 || s.max_disp % 8 != 0) return false;
    if (s.min_disp < 1) return false;
    if (!(1 <= s.p1 && s.p1 <= s.p2 && s.p2 <= 255)) return false;
    if (s.uniqueness < 0 || s.uniqueness > 99) return false;
    return s.lr_max >= -1 && s.lr_max <= 8 && s.pad_ == 0;
}

}   // namespace cvo_fe_rules

using namespace cvo_fe_rules;
using Ctx = cvo_fe_ctx;

namespace {

// "<name>: <why>"
int refuse(cvo_fe_ctx *ctx, const char *name, const char *why)
{
    return fail(ctx, CVO_HIP_ERR_INVALID, (std::string(name) + ": " + why).c_str());
}

// the opening of every setter, under the API lock
int setter_begin(cvo_fe_ctx *ctx, const char *name)
{
    if (!ctx) return CVO_HIP_ERR_INVALID;
    return ctx->pending ? refuse(ctx, name, "a frame is in flight") : CVO_HIP_OK;
}

// nothing to do: the setting is absent and stays so, or the bytes in force are given again
template <class S> bool same_setting(const S *p, bool has, const S &cur)
{
    return p ? has && std::memcmp(p, &cur, sizeof(S)) == 0 : !has;
}

// No frame is in flight: once the stream is idle nothing reads what the old graphs read, so what was built may take
// the place of what the context holds.  A failure's error is taken from the runtime as no_memory() takes it, so that
// the next frame does not find it.
int settle(cvo_fe_ctx *ctx, const char *name)
{
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) return CVO_HIP_OK;
    (void)hipGetLastError();
    return fail(ctx, CVO_HIP_ERR_HIP, name, e);
}

template <class S> void store_setting(bool &has, S &cur, const S *p)
{
    has = p != nullptr;
    cur = p ? *p : S{};
}

// every getter of a structure: the setting, or zeroes and "not set"
template <class S> int get_setting(const cvo_fe_ctx *ctx, bool cvo_fe_ctx::*has, S cvo_fe_ctx::*value, S *out, int *set)
{
    cvo_lock::Api api_guard;
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    *out = ctx->*has ? ctx->*value : S{};
    if (set) *set = ctx->*has ? 1 : 0;
    return CVO_HIP_OK;
}

// the setter of a plain number no buffer depends on: nothing to build and nothing to wait for.  Which path launches a
// frame has and which instance of the selector it launches are part of a captured graph.
template <class V> int set_number(cvo_fe_ctx *ctx, const char *name, bool accepted, const char *rule, V cvo_fe_ctx::*value, V given)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, name)) return rc;
    if (!accepted) return refuse(ctx, name, rule);
    if (given == ctx->*value) return CVO_HIP_OK;
    ctx->*value = given;
    drop_graphs(ctx);
    return CVO_HIP_OK;
}

template <class V> int get_number(const cvo_fe_ctx *ctx, V cvo_fe_ctx::*value, V *out)
{
    cvo_lock::Api api_guard;
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    *out = ctx->*value;
    return CVO_HIP_OK;
}

// A depth plane and its plane of flags, rect_plane(np) entries each, both or neither: built unless the context has
// them (`have`: the locals then stay empty).  CVO_HIP_OK, or CVO_HIP_ERR_NOMEM behind no_memory().  The gate and the mask (they share theirs), the median stage, the infill
// stage and the cull of a scan source each hold such a pair.
int plane_and_flags(cvo_fe_ctx *ctx, bool have, Dev<uint16_t> &plane, Dev<uint8_t> &flags, const char *what)
{
    const size_t n = rect_plane(ctx->np);
    if (have || (dev_alloc(plane, n) && dev_alloc(flags, n))) return CVO_HIP_OK;
    return no_memory(ctx, what);
}

int gate_buffers(cvo_fe_ctx *ctx, Dev<uint16_t> &ungated, Dev<uint8_t> &flags)
{
    return plane_and_flags(ctx, (bool)ctx->ungated, ungated, flags, "device memory for the ungated depth and the gate's flags");
}

// the packed right image and its staging, for a stereo context under a pixel format; both or neither (left empty for a
// context that has them, or one in BGR8)
int packed_right_buffers(cvo_fe_ctx *ctx, Dev<uint8_t> &packed_r, Pin<uint8_t> &h_packed_r)
{
    const size_t n = ctx->pix_row * (size_t)ctx->pix_rows;
    if (!unpacks(ctx) || ctx->packed_r || (dev_alloc(packed_r, n) && pin_alloc(h_packed_r, n))) return CVO_HIP_OK;
    return no_memory(ctx, "device and pinned memory for the packed right image");
}

}   // namespace

extern "C" {

int cvo_fe_check_depth_camera(const cvo_fe_depth_camera *rig) { return rig && rig_ok(*rig) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_depth_gate(const cvo_fe_depth_gate *gate) { return gate && gate_ok(*gate) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_stereo(const cvo_fe_stereo *st) { return st && stereo_ok(*st) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_stereo_paths(uint32_t mask) { return mask >= 1u && mask <= (uint32_t)CVO_FE_PATHS_8 ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_lidar(const cvo_fe_lidar *l) { return l && lidar_ok(*l) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_lidar_sweep(const cvo_fe_lidar_sweep *sw) { return sw && sweep_ok(*sw) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }
int cvo_fe_check_stereo_rig(const cvo_fe_stereo_rig *rig) { return rig && srig_ok(*rig) ? CVO_HIP_OK : CVO_HIP_ERR_INVALID; }

int cvo_fe_check_select_mode(int mode)
{
    return mode == CVO_FE_SELECT_IMAGE || mode == CVO_FE_SELECT_DEPTH ? CVO_HIP_OK : CVO_HIP_ERR_INVALID;
}

// the getters of the structures
int cvo_fe_get_depth_camera(const Ctx *c, cvo_fe_depth_camera *out, int *set) { return get_setting(c, &Ctx::has_rig, &Ctx::rig, out, set); }
int cvo_fe_get_depth_gate(const Ctx *c, cvo_fe_depth_gate *out, int *set) { return get_setting(c, &Ctx::has_gate, &Ctx::gate, out, set); }
int cvo_fe_get_stereo(const Ctx *c, cvo_fe_stereo *out, int *set) { return get_setting(c, &Ctx::has_stereo, &Ctx::stereo, out, set); }
int cvo_fe_get_stereo_speckle(const Ctx *c, cvo_fe_speckle *out, int *set) { return get_setting(c, &Ctx::has_speckle, &Ctx::speckle, out, set); }
int cvo_fe_get_depth_median(const Ctx *c, cvo_fe_depth_median *out, int *set) { return get_setting(c, &Ctx::has_median, &Ctx::median, out, set); }
int cvo_fe_get_depth_infill(const Ctx *c, cvo_fe_depth_infill *out, int *set) { return get_setting(c, &Ctx::has_infill, &Ctx::infill, out, set); }
int cvo_fe_get_lidar(const Ctx *c, cvo_fe_lidar *out, int *set) { return get_setting(c, &Ctx::has_lidar, &Ctx::lidar, out, set); }
int cvo_fe_get_lidar_sweep(const Ctx *c, cvo_fe_lidar_sweep *out, int *set) { return get_setting(c, &Ctx::has_sweep, &Ctx::sweep, out, set); }
int cvo_fe_get_stereo_rig(const Ctx *c, cvo_fe_stereo_rig *out, int *set) { return get_setting(c, &Ctx::has_srig, &Ctx::srig, out, set); }
// ... and of the plain numbers
int cvo_fe_get_stereo_paths(const Ctx *c, uint32_t *mask) { return get_number(c, &Ctx::stereo_paths, mask); }
int cvo_fe_get_select_mode(const Ctx *c, int *mode) { return get_number(c, &Ctx::select_mode, mode); }
int cvo_fe_get_pixel_format(const Ctx *c, int *format) { return get_number(c, &Ctx::pixfmt, format); }

int cvo_fe_set_depth_camera(cvo_fe_ctx *ctx, const cvo_fe_depth_camera *rig)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_depth_camera")) return rc;
    if (rig && !rig_ok(*rig)) return refuse(ctx, "set_depth_camera", rules::depth_camera);
    if (rig && ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_depth_camera: stereo is set, there is no depth image");
    if (rig && ctx->has_lidar)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_depth_camera: a scan source is set, there is no depth image");
    if (same_setting(rig, ctx->has_rig, ctx->rig)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    const int dw = rig ? rig->width : ctx->iw, dh = rig ? rig->height : ctx->ih;   // (without a rig: the input size)
    const size_t dnp = (size_t)dw * dh;
    Dev<uint16_t> new_depth;
    Pin<uint16_t> new_host;
    Dev<float2> new_rays;
    Dev<uint32_t> new_z;
    Dev<uint8_t> new_fdepth;   // (under a float depth format: the float image and its staging follow the size as well)
    Pin<uint8_t> new_fhost;
    const bool resize = dw != ctx->dw || dh != ctx->dh;   // the pinned staging image follows the depth size
    if (resize && !pin_alloc(new_host, dnp)) return no_memory(ctx, "set_depth_camera: pinned memory for the depth image");
    if (resize && converts(ctx) && !(dev_alloc(new_fdepth, dnp * depth_item(ctx)) && pin_alloc(new_fhost, dnp * depth_item(ctx))))
        return no_memory(ctx, "set_depth_camera: device and pinned memory for the float depth image");
    if (rig) {
        const size_t nr = (size_t)(dw + 1) * (dh + 1), nz = rect_plane(ctx->np);
        std::vector<float> t;
        std::vector<float2> inter;
        try { t.resize(2 * nr); inter.resize(nr); } catch (const std::bad_alloc &) {
            return fail(ctx, CVO_HIP_ERR_NOMEM, "set_depth_camera");
        }
        if (cvo_fe_depth_rays(rig, t.data(), t.data() + nr) != CVO_HIP_OK)
            return fail(ctx, CVO_HIP_ERR_INVALID, "set_depth_camera: depth_rays");
        for (size_t q = 0; q < nr; ++q) inter[q] = make_float2(t[q], t[nr + q]);
        if (!dev_alloc(new_depth, dnp) || !dev_alloc(new_rays, nr) || (!ctx->zbuf && !dev_alloc(new_z, nz)))
            return no_memory(ctx, "set_depth_camera: device memory for the raw depth, the rays and the z-buffer");
        hipError_t e = hipStreamSynchronize(ctx->stream);   // (settle(), with the upload behind it under one message)
        if (e == hipSuccess) e = hipMemcpy(new_rays.get(), inter.data(), nr * sizeof(float2), hipMemcpyHostToDevice);
        // the z-buffer is armed here and by every frame's k_fe_depth_final after it
        if (e == hipSuccess) e = hipMemset(new_z ? new_z.get() : ctx->zbuf.get(), 0xFF, nz * sizeof(uint32_t));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, CVO_HIP_ERR_HIP, "set_depth_camera: upload of the rays", e);
        }
    } else if (const int rc = settle(ctx, "set_depth_camera")) return rc;
    // whole: the old raw depth and rays go, with or without new ones
    ctx->rig_depth = std::move(new_depth);
    ctx->rays = std::move(new_rays);
    hand_over(ctx->zbuf, new_z);
    hand_over(ctx->h_depth, new_host);
    hand_over(ctx->fdepth, new_fdepth);
    hand_over(ctx->h_fdepth, new_fhost);
    store_setting(ctx->has_rig, ctx->rig, rig);
    ctx->dw = dw;
    ctx->dh = dh;
    drop_graphs(ctx);
    return CVO_HIP_OK;
}

int cvo_fe_set_depth_gate(cvo_fe_ctx *ctx, const cvo_fe_depth_gate *gate)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_depth_gate")) return rc;
    if (gate && !gate_ok(*gate)) return refuse(ctx, "set_depth_gate", rules::depth_gate);
    if (same_setting(gate, ctx->has_gate, ctx->gate)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint16_t> ungated;
    Dev<uint8_t> flags;
    if (gate && gate_buffers(ctx, ungated, flags)) return CVO_HIP_ERR_NOMEM;
    if (const int rc = settle(ctx, "set_depth_gate")) return rc;
    hand_over(ctx->ungated, ungated);
    hand_over(ctx->gate_flags, flags);
    store_setting(ctx->has_gate, ctx->gate, gate);
    drop_graphs(ctx);   // (the gate's numbers and the planes of a frame are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_stereo(cvo_fe_ctx *ctx, const cvo_fe_stereo *st)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_stereo")) return rc;
    if (st && !stereo_ok(*st)) return refuse(ctx, "set_stereo", rules::stereo);
    if (st && ctx->has_rig) return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo: a depth camera is set");
    if (st && ctx->has_lidar) return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo: a scan source is set");
    if (st && ctx->rectify)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo: the camera model has a lens distortion; the pair must be rectified");
    if (!st && ctx->has_srig) return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo: a stereo rig is set: clear the rig first");
    if (same_setting(st, ctx->has_stereo, ctx->stereo)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)ctx->np;
    Dev<uint8_t> right_img, right_gray, flags;
    Pin<uint8_t> h_right;
    Dev<uint64_t> census;
    Dev<uint16_t> sum, disparity, table;
    Dev<uint32_t> win;
    Pin<uint16_t> h_table;
    Dev<uint8_t> packed_r;   // (under a pixel format: the right image arrives packed as the left one does)
    Pin<uint8_t> h_packed_r;
    Dev<uint8_t> full_right;
    if (st) {
        // (all but the cost sums come with the first settings and stay; the table has room for the largest max_disp)
        if (!ctx->right_img &&
            !(dev_alloc(right_img, np * 3) && dev_alloc(right_gray, np) && dev_alloc(flags, np) && pin_alloc(h_right, (size_t)ctx->iw * ctx->ih * 3) &&
              dev_alloc(census, 2 * np) && dev_alloc(disparity, np) && dev_alloc(win, np) && dev_alloc(table, 16 * 128) &&
              pin_alloc(h_table, 16 * 128)))
            return no_memory(ctx, "set_stereo: device and pinned memory for the right image and the matcher's planes");
        if ((!ctx->sgm_sum || !ctx->has_stereo || st->max_disp != ctx->stereo.max_disp) && !dev_alloc(sum, np * (size_t)st->max_disp))
            return no_memory(ctx, "set_stereo: device memory for the cost sums");
        if (packed_right_buffers(ctx, packed_r, h_packed_r) != CVO_HIP_OK) return CVO_HIP_ERR_NOMEM;
        // (under input binning: the right image arrives at the input size as the left one does)
        if (ctx->has_bin && !ctx->full_right && !dev_alloc(full_right, (size_t)ctx->iw * ctx->ih * 3))
            return no_memory(ctx, "set_stereo: device memory for the input-size right image");
    }
    if (const int rc = settle(ctx, "set_stereo")) return rc;
    hand_over(ctx->full_right, full_right);
    hand_over(ctx->right_img, right_img);
    hand_over(ctx->right_gray, right_gray);
    hand_over(ctx->stereo_flags, flags);
    hand_over(ctx->h_right, h_right);
    hand_over(ctx->census, census);
    hand_over(ctx->disparity, disparity);
    hand_over(ctx->stereo_win, win);
    hand_over(ctx->depth_table, table);
    hand_over(ctx->h_depth_table, h_table);
    hand_over(ctx->sgm_sum, sum);
    hand_over(ctx->packed_r, packed_r);
    hand_over(ctx->h_packed_r, h_packed_r);
    if (!st) ctx->sgm_sum.reset();   // (the one large buffer: a context back on depth images does not keep it)
    store_setting(ctx->has_stereo, ctx->stereo, st);
    ctx->table_fx = ctx->table_scale = 0.0f;   // (the table depends on baseline, min_disp and max_disp: made again)
    drop_graphs(ctx);   // (the settings and the planes of a frame are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_stereo_paths(cvo_fe_ctx *ctx, uint32_t mask)
{
    return set_number(ctx, "set_stereo_paths", cvo_fe_check_stereo_paths(mask) == CVO_HIP_OK, rules::stereo_paths, &Ctx::stereo_paths, mask);
}

int cvo_fe_set_select_mode(cvo_fe_ctx *ctx, int mode)
{
    return set_number(ctx, "set_select_mode", cvo_fe_check_select_mode(mode) == CVO_HIP_OK, rules::select_mode, &Ctx::select_mode, mode);
}

int cvo_fe_set_stereo_speckle(cvo_fe_ctx *ctx, const cvo_fe_speckle *sp)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_stereo_speckle")) return rc;
    if (sp && cvo_fe_check_speckle(sp) != CVO_HIP_OK) return refuse(ctx, "set_stereo_speckle", rules::stereo_speckle);
    if (same_setting(sp, ctx->has_speckle, ctx->speckle)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint32_t> words;
    if (sp && !ctx->speckle_words && !dev_alloc(words, 3 * (size_t)ctx->np + 1))
        return no_memory(ctx, "set_stereo_speckle: device memory for the parents, the sums and the sizes");
    if (const int rc = settle(ctx, "set_stereo_speckle")) return rc;
    hand_over(ctx->speckle_words, words);
    if (!sp) ctx->speckle_words.reset();
    store_setting(ctx->has_speckle, ctx->speckle, sp);
    drop_graphs(ctx);   // (whether a frame has the filter's launches, their numbers and planes are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_depth_median(cvo_fe_ctx *ctx, const cvo_fe_depth_median *m)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_depth_median")) return rc;
    if (m && cvo_fe_check_depth_median(m) != CVO_HIP_OK) return refuse(ctx, "set_depth_median", rules::depth_median);
    if (same_setting(m, ctx->has_median, ctx->median)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint16_t> unfiltered;
    Dev<uint8_t> flags;
    if (m && plane_and_flags(ctx, (bool)ctx->unfiltered, unfiltered, flags,
                             "set_depth_median: device memory for the unfiltered depth and the stage's flags"))
        return CVO_HIP_ERR_NOMEM;
    if (const int rc = settle(ctx, "set_depth_median")) return rc;
    hand_over(ctx->unfiltered, unfiltered);
    hand_over(ctx->median_flags, flags);
    if (!m) {
        ctx->unfiltered.reset();
        ctx->median_flags.reset();
    }
    store_setting(ctx->has_median, ctx->median, m);
    drop_graphs(ctx);   // (whether a frame has the stage's launch, its numbers and where the producers write are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_depth_infill(cvo_fe_ctx *ctx, const cvo_fe_depth_infill *f)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_depth_infill")) return rc;
    if (f && cvo_fe_check_depth_infill(f) != CVO_HIP_OK) return refuse(ctx, "set_depth_infill", rules::depth_infill);
    if (same_setting(f, ctx->has_infill, ctx->infill)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint16_t> sparse;
    Dev<uint8_t> flags;
    if (f && plane_and_flags(ctx, (bool)ctx->sparse, sparse, flags,
                             "set_depth_infill: device memory for the sparse depth and the stage's flags"))
        return CVO_HIP_ERR_NOMEM;
    if (const int rc = settle(ctx, "set_depth_infill")) return rc;
    hand_over(ctx->sparse, sparse);
    hand_over(ctx->infill_flags, flags);
    if (!f) {
        ctx->sparse.reset();
        ctx->infill_flags.reset();
    }
    store_setting(ctx->has_infill, ctx->infill, f);
    drop_graphs(ctx);   // (whether a frame has the stage's launch, its numbers and where the producers write are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_pixel_format(cvo_fe_ctx *ctx, int format)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_pixel_format")) return rc;
    size_t row = 0;
    int rows = 0;
    if (!fe_unpack_layout(format, ctx->iw, ctx->ih, &row, &rows))   // (under input binning: the input size)
        return refuse(ctx, "set_pixel_format", "a CVO_FE_PIXEL_* format that fits the context's size (YUY2, UYVY: an even width; "
                                               "NV12: an even width and height)");
    if (format == ctx->pixfmt) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    const bool on = format != CVO_FE_PIXEL_BGR8;
    Dev<uint8_t> packed, packed_r;
    Pin<uint8_t> h_packed, h_packed_r;
    // (the sizes follow the format: built anew for each, the right image's only for a context under stereo)
    if (on && !(dev_alloc(packed, row * (size_t)rows) && pin_alloc(h_packed, row * (size_t)rows) &&
                (!ctx->has_stereo || (dev_alloc(packed_r, row * (size_t)rows) && pin_alloc(h_packed_r, row * (size_t)rows)))))
        return no_memory(ctx, "set_pixel_format: device and pinned memory for the packed image");
    if (const int rc = settle(ctx, "set_pixel_format")) return rc;
    ctx->packed = std::move(packed);   // (all four replaced or, back in BGR8, freed)
    ctx->packed_r = std::move(packed_r);
    ctx->h_packed = std::move(h_packed);
    ctx->h_packed_r = std::move(h_packed_r);
    ctx->pixfmt = format;
    ctx->pix_row = on ? row : 0;
    ctx->pix_rows = on ? rows : 0;
    drop_graphs(ctx);   // (whether a frame has the stage's launch, its instance and what is uploaded are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_get_input_binning(const Ctx *c, cvo_fe_binning *out, int *set) { return get_setting(c, &Ctx::has_bin, &Ctx::bin, out, set); }

int cvo_fe_set_input_binning(cvo_fe_ctx *ctx, const cvo_fe_binning *b)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_input_binning")) return rc;
    if (b && cvo_fe_check_binning(b, ctx->d.w, ctx->d.h) != CVO_HIP_OK) return refuse(ctx, "set_input_binning", rules::binning);
    const int iw = (b ? b->factor : 1) * ctx->d.w, ih = (b ? b->factor : 1) * ctx->d.h;
    size_t row = 0;
    int rows = 0;
    if (unpacks(ctx) && !fe_unpack_layout(ctx->pixfmt, iw, ih, &row, &rows))
        return refuse(ctx, "set_input_binning", "the pixel format in force does not fit the input size, factor times the context's");
    if (same_setting(b, ctx->has_bin, ctx->bin)) return CVO_HIP_OK;
    // (a vignette belongs to the sensor's pixels: it does not follow a change of the input size)
    if (ctx->photo_vignette && (iw != ctx->iw || ih != ctx->ih))
        return refuse(ctx, "set_input_binning", ("a vignette of " + std::to_string(ctx->iw) + " x " + std::to_string(ctx->ih) +
                                                 " is set and the input size would become " + std::to_string(iw) + " x " +
                                                 std::to_string(ih) + ": set the photometric stage off first, and again with a "
                                                 "vignette of that size").c_str());
    FE_HIP(hipSetDevice(ctx->device));
    // Everything that holds a caller's image follows the input size: the staging of the colour image, of the right one
    // (a context that has had stereo set), of the depth image (unless a depth camera sizes it), the float and the
    // packed images.  A change of depth_min alone builds nothing.
    const bool resize = iw != ctx->iw || ih != ctx->ih;
    const size_t inp = (size_t)iw * ih, ditem = depth_item(ctx), packed_bytes = row * (size_t)rows;
    Dev<uint8_t> full_img, full_right, packed, packed_r, fdepth;
    Dev<uint16_t> full_depth;
    Pin<uint8_t> h_img, h_right, h_packed, h_packed_r, h_fdepth;
    Pin<uint16_t> h_depth;
    if (resize) {
        bool ok = pin_alloc(h_img, inp * 3) && (!b || (dev_alloc(full_img, inp * 3) && dev_alloc(full_depth, inp)));
        if (ctx->h_right) ok = ok && pin_alloc(h_right, inp * 3) && (!b || dev_alloc(full_right, inp * 3));
        if (!ctx->has_rig) ok = ok && pin_alloc(h_depth, inp);
        if (!ctx->has_rig && converts(ctx)) ok = ok && dev_alloc(fdepth, inp * ditem) && pin_alloc(h_fdepth, inp * ditem);
        if (unpacks(ctx)) ok = ok && dev_alloc(packed, packed_bytes) && pin_alloc(h_packed, packed_bytes);
        if (unpacks(ctx) && ctx->packed_r) ok = ok && dev_alloc(packed_r, packed_bytes) && pin_alloc(h_packed_r, packed_bytes);
        if (!ok) return no_memory(ctx, "set_input_binning: device and pinned memory for the images of the input size");
    }
    if (const int rc = settle(ctx, "set_input_binning")) return rc;
    if (resize) {
        ctx->full_img = std::move(full_img);   // (the three replaced or, at off, freed)
        ctx->full_right = std::move(full_right);
        ctx->full_depth = std::move(full_depth);
        ctx->h_img = std::move(h_img);
        hand_over(ctx->h_right, h_right);
        hand_over(ctx->h_depth, h_depth);
        hand_over(ctx->fdepth, fdepth);
        hand_over(ctx->h_fdepth, h_fdepth);
        hand_over(ctx->packed, packed);
        hand_over(ctx->h_packed, h_packed);
        hand_over(ctx->packed_r, packed_r);
        hand_over(ctx->h_packed_r, h_packed_r);
        ctx->iw = iw;
        ctx->ih = ih;
        if (!ctx->has_rig) { ctx->dw = iw; ctx->dh = ih; }
        if (unpacks(ctx)) { ctx->pix_row = row; ctx->pix_rows = rows; }
    }
    store_setting(ctx->has_bin, ctx->bin, b);
    drop_graphs(ctx);   // (whether a frame has the bin's launch, its numbers and where the uploads land are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_get_photometric(const Ctx *c, cvo_fe_photometric *out, int *set) { return get_setting(c, &Ctx::has_photo, &Ctx::photo, out, set); }

int cvo_fe_set_photometric(cvo_fe_ctx *ctx, const cvo_fe_photometric *p, const uint16_t *response, const uint16_t *vignette,
                           size_t vignette_stride)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_photometric")) return rc;
    if (p && p->flags == 0u && !response && !vignette) p = nullptr;   // (the other spelling of "off")
    if (p && cvo_fe_check_photometric(p, response != nullptr, vignette != nullptr) != CVO_HIP_OK)
        return refuse(ctx, "set_photometric", rules::photometric);
    const size_t vrow = (size_t)ctx->iw * 2;
    if (p && vignette && (vignette_stride < vrow || vignette_stride % 2 != 0))
        return refuse(ctx, "set_photometric", ("a vignette of " + std::to_string(ctx->iw) + " x " + std::to_string(ctx->ih) +
                                               " uint16, the size of the images a frame takes, in rows an even number of "
                                               "bytes, at least the row's, apart").c_str());
    if (!p && !ctx->has_photo) return CVO_HIP_OK;   // (tables cannot be compared: a setting given again is made again)
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint16_t> resp, vig;
    Dev<FePhotoHeader> hdr;
    Pin<FePhotoHeader> h_hdr;
    Dev<FePhotoState> state;
    Pin<cvo_fe_photometric_frame> h_rec;
    if (p) {
        const size_t inp = (size_t)ctx->iw * ctx->ih;
        const bool automatic = (p->flags & CVO_FE_PHOTO_AUTO) != 0;
        if (!(dev_alloc(hdr, 1) && pin_alloc(h_hdr, 1) && (!response || dev_alloc(resp, 768)) && (!vignette || dev_alloc(vig, inp)) &&
              (!automatic || (dev_alloc(state, 1) && pin_alloc(h_rec, 1)))))
            return no_memory(ctx, "set_photometric: device and pinned memory for the tables, the header and the state");
        hipError_t e = hipSuccess;
        if (response) e = hipMemcpy(resp.get(), response, 768 * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && vignette)
            e = hipMemcpy2D(vig.get(), vrow, vignette, vignette_stride, vrow, (size_t)ctx->ih, hipMemcpyHostToDevice);
        // the state starts at zero: the sums, and the lock open
        if (e == hipSuccess && automatic) e = hipMemset(state.get(), 0, sizeof(FePhotoState));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (settle(), behind the uploads under one message)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, CVO_HIP_ERR_HIP, "set_photometric: upload of the tables", e);
        }
    } else if (const int rc = settle(ctx, "set_photometric")) return rc;
    // whole: everything of the old setting goes, with or without a new one
    ctx->photo_response = std::move(resp);
    ctx->photo_vignette = std::move(vig);
    ctx->photo_hdr = std::move(hdr);
    ctx->h_photo_hdr = std::move(h_hdr);
    ctx->photo_state = std::move(state);
    ctx->h_photo_rec = std::move(h_rec);
    store_setting(ctx->has_photo, ctx->photo, p);
    for (uint32_t &g : ctx->photo_gain) g = 4096u;
    ctx->photo_rearm = false;   // (the new state's lock is open)
    ctx->photo_frame = cvo_fe_photometric_frame{};
    drop_graphs(ctx);   // (whether a frame has the stage's launches, their instances, numbers and tables are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_photometric_gain(cvo_fe_ctx *ctx, const float gain[3])
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!gain) return fail(ctx, CVO_HIP_ERR_INVALID, "set_photometric_gain: bad argument");
    if (!ctx->has_photo || !(ctx->photo.flags & CVO_FE_PHOTO_GAIN))
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_photometric_gain: the stage is not set with CVO_FE_PHOTO_GAIN (cvo_fe_set_photometric)");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(gain[c]) || gain[c] < 0.0625f || gain[c] > 15.99f)
            return refuse(ctx, "set_photometric_gain", rules::photometric_gain);
    for (int c = 0; c < 3; ++c) {   // (read by the next submit: no graph holds it)
        const float scaled = gain[c] * 4096.0f;
        ctx->photo_gain[c] = (uint32_t)(scaled + 0.5f);
    }
    return CVO_HIP_OK;
}

int cvo_fe_photometric_rearm(cvo_fe_ctx *ctx)
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!ctx->has_photo || !(ctx->photo.flags & CVO_FE_PHOTO_AUTO))
        return fail(ctx, CVO_HIP_ERR_INVALID, "photometric_rearm: the stage is not set with CVO_FE_PHOTO_AUTO (cvo_fe_set_photometric)");
    ctx->photo_rearm = true;   // (travels in the next frame's header)
    return CVO_HIP_OK;
}

int cvo_fe_get_photometric_frame(const cvo_fe_ctx *ctx, cvo_fe_photometric_frame *out)
{
    cvo_lock::Api api_guard;
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    if (!ctx->has_photo) return CVO_HIP_ERR_INVALID;
    *out = ctx->photo_frame;
    return CVO_HIP_OK;
}

int cvo_fe_bin_camera(const cvo_fe_camera_model *in, int factor, cvo_fe_camera_model *out)
{
    if (!in || !out || factor < 2 || factor > 4 || !model_ok(*in)) return CVO_HIP_ERR_INVALID;
    const float f = (float)factor, c = 0.5f * (float)(factor - 1);
    cvo_fe_camera_model m = *in;   // (depth_scale and dist unchanged)
    m.fx = in->fx / f;
    m.fy = in->fy / f;
    m.cx = (in->cx - c) / f;
    m.cy = (in->cy - c) / f;
    *out = m;
    return CVO_HIP_OK;
}

int cvo_fe_bin_stereo_rig(const cvo_fe_stereo_rig *in, int factor, cvo_fe_stereo_rig *out)
{
    if (!in || !out || factor < 2 || factor > 4 || !srig_ok(*in)) return CVO_HIP_ERR_INVALID;
    const float f = (float)factor, c = 0.5f * (float)(factor - 1);
    cvo_fe_stereo_rig r = *in;   // (the rotations, the baseline and depth_scale unchanged)
    for (cvo_fe_lens *l : {&r.left, &r.right}) {
        l->fx = l->fx / f;
        l->fy = l->fy / f;
        l->cx = (l->cx - c) / f;
        l->cy = (l->cy - c) / f;
    }
    r.fx = r.fx / f;
    r.fy = r.fy / f;
    r.cx = (r.cx - c) / f;
    r.cy = (r.cy - c) / f;
    *out = r;
    return CVO_HIP_OK;
}

int cvo_fe_set_depth_format(cvo_fe_ctx *ctx, int format, float unit)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_depth_format")) return rc;
    if (!fe_depth_format_ok(format, unit))
        return refuse(ctx, "set_depth_format", "a CVO_FE_DEPTH_* format, a finite unit in [2^-20, 2^20], and a unit of 1 under "
                                               "CVO_FE_DEPTH_U16");
    if (format == ctx->depthfmt && unit == ctx->depth_unit) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint8_t> fdepth;
    Pin<uint8_t> h_fdepth;
    const size_t bytes = (size_t)ctx->dw * ctx->dh * fe_depth_item(format);
    const bool on = format != CVO_FE_DEPTH_U16, sized = on && fe_depth_item(format) == depth_item(ctx) && converts(ctx);
    if (on && !sized && !(dev_alloc(fdepth, bytes) && pin_alloc(h_fdepth, bytes)))
        return no_memory(ctx, "set_depth_format: device and pinned memory for the float depth image");
    if (const int rc = settle(ctx, "set_depth_format")) return rc;
    if (!sized) {   // (both replaced or, back in U16, freed)
        ctx->fdepth = std::move(fdepth);
        ctx->h_fdepth = std::move(h_fdepth);
    }
    ctx->depthfmt = format;
    ctx->depth_unit = unit;
    drop_graphs(ctx);   // (the format, the unit and the float image are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_get_depth_format(const cvo_fe_ctx *ctx, int *format, float *unit)
{
    cvo_lock::Api api_guard;
    if (!ctx || !format || !unit) return CVO_HIP_ERR_INVALID;
    *format = ctx->depthfmt;
    *unit = ctx->depth_unit;
    return CVO_HIP_OK;
}

int cvo_fe_set_lidar(cvo_fe_ctx *ctx, const cvo_fe_lidar *l)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_lidar")) return rc;
    if (l && !lidar_ok(*l)) return refuse(ctx, "set_lidar", rules::lidar);
    if (l && ctx->has_stereo) return fail(ctx, CVO_HIP_ERR_INVALID, "set_lidar: stereo is set");
    if (l && ctx->has_rig) return fail(ctx, CVO_HIP_ERR_INVALID, "set_lidar: a depth camera is set");
    if (same_setting(l, ctx->has_lidar, ctx->lidar)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Pin<uint8_t> h_scan;
    Dev<uint8_t> d_scan, flags;
    Dev<uint16_t> p0;
    Dev<uint32_t> z;
    const size_t nz = rect_plane(ctx->np);
    if (l) {
        const size_t bytes = lidar_scan_bytes(l->max_points, ctx->scan_record);   // (a sweep stays: its record size too)
        const bool resize = !ctx->has_lidar || l->max_points != ctx->lidar.max_points;
        if (resize && !(pin_alloc(h_scan, bytes) && dev_alloc(d_scan, bytes)))
            return no_memory(ctx, "set_lidar: pinned and device memory for a scan of max_points points");
        if (!ctx->zbuf && !dev_alloc(z, nz)) return no_memory(ctx, "set_lidar: device memory for the z-buffer");
        if (l->occl_rel > 0.0f && plane_and_flags(ctx, (bool)ctx->lidar_p0, p0, flags,
                                                  "set_lidar: device memory for the plane before culling and the flags"))
            return CVO_HIP_ERR_NOMEM;
        if (h_scan) std::memset(h_scan.get(), 0, FE_LIDAR_HEADER);   // (a scan of no points until the first frame)
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);   // (settle(), with the arming behind it under one message)
    // a new z-buffer is armed here; every frame's k_fe_depth_final arms it after that
    if (e == hipSuccess && z) e = hipMemset(z.get(), 0xFF, nz * sizeof(uint32_t));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, CVO_HIP_ERR_HIP, "set_lidar", e);
    }
    hand_over(ctx->h_scan, h_scan);
    hand_over(ctx->d_scan, d_scan);
    hand_over(ctx->zbuf, z);
    hand_over(ctx->lidar_p0, p0);
    hand_over(ctx->lidar_flags, flags);
    if (!l) {   // (given back: a depth camera set later makes its own z-buffer; the sweep goes with the scan source)
        ctx->h_scan.reset();
        ctx->d_scan.reset();
        ctx->zbuf.reset();
        store_setting<cvo_fe_lidar_sweep>(ctx->has_sweep, ctx->sweep, nullptr);
        ctx->scan_record = 12;
        for (float &t : ctx->lidar_twist) t = 0.0f;
    }
    if (!l || !(l->occl_rel > 0.0f)) {
        ctx->lidar_p0.reset();
        ctx->lidar_flags.reset();
    }
    store_setting(ctx->has_lidar, ctx->lidar, l);
    drop_graphs(ctx);   // (the kind of a frame, the settings, the scan's capacity and the planes are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_lidar_sweep(cvo_fe_ctx *ctx, const cvo_fe_lidar_sweep *sw)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_lidar_sweep")) return rc;
    if (sw && !sweep_ok(*sw)) return refuse(ctx, "set_lidar_sweep",
                      "a mode of CVO_FE_SWEEP_*, finite members, time_offset >= 12 and a multiple of 4, time_scale not 0, "
                      "direction +1 or -1 under the azimuth mode and 0 otherwise, phase0 in [0, 1), s_ref in [0, 1], "
                      "time_origin 0 outside the float mode, pad_ 0");
    if (sw && !ctx->has_lidar) return fail(ctx, CVO_HIP_ERR_INVALID, "set_lidar_sweep: no scan source (cvo_fe_set_lidar)");
    if (!sw && !ctx->has_sweep) return CVO_HIP_OK;   // (the sweep in force given again is set again: the twist is zero after it)
    FE_HIP(hipSetDevice(ctx->device));
    Pin<uint8_t> h_scan;
    Dev<uint8_t> d_scan;
    const size_t record = lidar_record_bytes(sweep_time_offset(sw));
    if (record != ctx->scan_record) {   // (a record with or without its time word: the staging and its copy follow)
        const size_t bytes = lidar_scan_bytes(ctx->lidar.max_points, record);
        if (!(pin_alloc(h_scan, bytes) && dev_alloc(d_scan, bytes)))
            return no_memory(ctx, "set_lidar_sweep: pinned and device memory for a scan of max_points points");
        std::memset(h_scan.get(), 0, FE_LIDAR_HEADER);   // (a scan of no points until the first frame)
    }
    if (const int rc = settle(ctx, "set_lidar_sweep")) return rc;
    hand_over(ctx->h_scan, h_scan);
    hand_over(ctx->d_scan, d_scan);
    ctx->scan_record = record;
    store_setting(ctx->has_sweep, ctx->sweep, sw);
    for (float &t : ctx->lidar_twist) t = 0.0f;
    drop_graphs(ctx);   // (the kernel's instance, the sweep's words and the size of the copy are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_lidar_motion(cvo_fe_ctx *ctx, const float twist[6])
{
    cvo_lock::Api api_guard;
    if (!ctx) return CVO_HIP_ERR_INVALID;
    if (!twist) return fail(ctx, CVO_HIP_ERR_INVALID, "set_lidar_motion: bad argument");
    if (!ctx->has_sweep) return fail(ctx, CVO_HIP_ERR_INVALID, "set_lidar_motion: no sweep (cvo_fe_set_lidar_sweep)");
    if (!twist_ok(twist)) return refuse(ctx, "set_lidar_motion", rules::lidar_motion);
    for (int k = 0; k < 6; ++k) ctx->lidar_twist[k] = twist[k];   // (read by the next submit: no graph holds it)
    return CVO_HIP_OK;
}

int cvo_fe_get_lidar_motion(const cvo_fe_ctx *ctx, float twist[6])
{
    cvo_lock::Api api_guard;
    if (!ctx || !twist) return CVO_HIP_ERR_INVALID;
    for (int k = 0; k < 6; ++k) twist[k] = ctx->lidar_twist[k];
    return CVO_HIP_OK;
}

int cvo_fe_set_stereo_rig(cvo_fe_ctx *ctx, const cvo_fe_stereo_rig *rig)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_stereo_rig")) return rc;
    if (rig && !srig_ok(*rig)) return refuse(ctx, "set_stereo_rig", rules::stereo_rig);
    if (rig && !ctx->has_stereo) return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo_rig: stereo is not set (cvo_fe_set_stereo)");
    if (rig && ctx->custom)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo_rig: a camera model is set; the rig is the camera: clear the model first");
    if (same_setting(rig, ctx->has_srig, ctx->srig)) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint8_t> raw_l, raw_r, valid;
    Dev<int32_t> new_map;
    if (rig) {
        const size_t np = (size_t)ctx->np, plane = rect_plane(ctx->np);
        std::vector<int32_t> map;
        try { map.resize(4 * plane); } catch (const std::bad_alloc &) { return fail(ctx, CVO_HIP_ERR_NOMEM, "set_stereo_rig"); }
        for (int k = 0; k < 2; ++k)
            if (cvo_fe_stereo_rig_map(rig, k, ctx->d.w, ctx->d.h, map.data() + 2 * k * plane, map.data() + (2 * k + 1) * plane) !=
                CVO_HIP_OK)
                return fail(ctx, CVO_HIP_ERR_INVALID, "set_stereo_rig: stereo_rig_map");
        // (the raw images and the validity plane come with the first rig and stay until it is cleared; the map is new)
        if ((!ctx->srig_raw_l && !(dev_alloc(raw_l, np * 3) && dev_alloc(raw_r, np * 3) && dev_alloc(valid, plane))) ||
            !dev_alloc(new_map, 4 * plane))
            return no_memory(ctx, "set_stereo_rig: device memory for the raw pair, the maps and the validity plane");
        hipError_t e = hipMemcpy(new_map.get(), map.data(), 4 * plane * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (settle(), behind the upload under one message)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, CVO_HIP_ERR_HIP, "set_stereo_rig: upload of the maps", e);
        }
    } else if (const int rc = settle(ctx, "set_stereo_rig")) return rc;
    hand_over(ctx->srig_raw_l, raw_l);
    hand_over(ctx->srig_raw_r, raw_r);
    hand_over(ctx->srig_valid, valid);
    ctx->srig_map = std::move(new_map);
    if (!rig) {   // (given back with the rig)
        ctx->srig_raw_l.reset();
        ctx->srig_raw_r.reset();
        ctx->srig_valid.reset();
    }
    store_setting(ctx->has_srig, ctx->srig, rig);
    ctx->table_fx = ctx->table_scale = 0.0f;   // (the table follows the rig's baseline: made again)
    drop_graphs(ctx);   // (the rig's buffers and numbers are part of a captured graph)
    return CVO_HIP_OK;
}

int cvo_fe_set_mask(cvo_fe_ctx *ctx, const uint8_t *mask, size_t stride)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_mask")) return rc;
    const int w = ctx->d.w, h = ctx->d.h;
    if (mask && stride < (size_t)w) return fail(ctx, CVO_HIP_ERR_INVALID, "set_mask: stride below the width");
    if (!mask && !ctx->has_mask) return CVO_HIP_OK;
    FE_HIP(hipSetDevice(ctx->device));
    Dev<uint16_t> ungated;
    Dev<uint8_t> flags, d_mask;
    Pin<uint8_t> h_mask;
    if (mask && gate_buffers(ctx, ungated, flags)) return CVO_HIP_ERR_NOMEM;
    // (the mask's device plane and its staging image come and go together)
    if (mask && !ctx->d_mask && !(dev_alloc(d_mask, rect_plane(ctx->np)) && pin_alloc(h_mask, (size_t)ctx->np)))
        return no_memory(ctx, "set_mask: device and pinned memory for the mask");
    if (const int rc = settle(ctx, "set_mask")) return rc;   // (no upload reads the staging image any more)
    hand_over(ctx->ungated, ungated);
    hand_over(ctx->gate_flags, flags);
    hand_over(ctx->d_mask, d_mask);
    hand_over(ctx->h_mask, h_mask);
    if (mask) {
        copy_rows(ctx->h_mask.get(), mask, stride, (size_t)w, h);
        ctx->mask_dirty = true;
    }
    // new contents go to the same address: only a mask that appears or disappears changes a frame's sequence
    if ((mask != nullptr) != ctx->has_mask) {
        ctx->has_mask = mask != nullptr;
        drop_graphs(ctx);
    }
    return CVO_HIP_OK;
}

int cvo_fe_set_camera(cvo_fe_ctx *ctx, const cvo_fe_camera_model *model)
{
    cvo_lock::Api api_guard;
    if (const int rc = setter_begin(ctx, "set_camera")) return rc;
    if (model && !model_ok(*model)) return refuse(ctx, "set_camera", rules::camera);
    if (model && ctx->has_srig)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_camera: a stereo rig is set and is the camera: clear the rig first");
    if (same_setting(model, ctx->custom, ctx->cam)) return CVO_HIP_OK;
    const bool bent = model && distorts(model->dist);
    if (bent && ctx->has_stereo)
        return fail(ctx, CVO_HIP_ERR_INVALID, "set_camera: stereo is set and takes a rectified pair: dist must be zero");
    if (bent) {   // (a model without distortion changes numbers only: no buffer, and nothing to wait for)
        const size_t np = (size_t)ctx->np, plane = rect_plane(ctx->np);
        std::vector<int32_t> map;
        try { map.resize(2 * plane); } catch (const std::bad_alloc &) { return fail(ctx, CVO_HIP_ERR_NOMEM, "set_camera"); }
        if (cvo_fe_rectify_map(model, ctx->d.w, ctx->d.h, map.data(), map.data() + plane) != CVO_HIP_OK)
            return fail(ctx, CVO_HIP_ERR_INVALID, "set_camera: rectify_map");
        FE_HIP(hipSetDevice(ctx->device));
        Dev<uint8_t> raw_img;
        Dev<uint16_t> raw_depth;
        Dev<int32_t> new_map;
        const bool first = !ctx->raw_img;   // (the two raw buffers come and go together)
        if ((first && !(dev_alloc(raw_img, np * 3) && dev_alloc(raw_depth, np))) || !dev_alloc(new_map, 2 * plane))
            return no_memory(ctx, "set_camera: device memory for the raw images and the map");
        hipError_t e = hipMemcpy(new_map.get(), map.data(), 2 * plane * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (settle(), behind the upload under one message)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, CVO_HIP_ERR_HIP, "set_camera: upload of the map", e);
        }
        hand_over(ctx->raw_img, raw_img);
        hand_over(ctx->raw_depth, raw_depth);
        ctx->rect_map = std::move(new_map);
    }
    store_setting(ctx->custom, ctx->cam, model);
    ctx->rectify = bent;
    drop_graphs(ctx);
    return CVO_HIP_OK;
}

// (not get_setting: it reports the camera in force, which is a stereo rig's or the table's where no model is set)
int cvo_fe_get_camera(const cvo_fe_ctx *ctx, cvo_fe_camera_model *out, int *custom)
{
    cvo_lock::Api api_guard;
    if (!ctx || !out) return CVO_HIP_ERR_INVALID;
    float cam[5];
    camera_in_force(ctx, ctx->p_seq, cam);
    const float *dist = ctx->cam.dist;   // (all zero without a caller's model, and under a stereo rig: it has none)
    *out = cvo_fe_camera_model{cam[0], cam[1], cam[2], cam[3], cam[4], {dist[0], dist[1], dist[2], dist[3], dist[4]}};
    if (custom) *custom = ctx->custom || ctx->has_srig ? 1 : 0;
    return CVO_HIP_OK;
}

// the two plain fields beside the settings: neither is part of a captured graph's sequence (both are in its key)
int cvo_fe_set_device_output(cvo_fe_ctx *ctx, int on)
{
    if (const int rc = setter_begin(ctx, "set_device_output")) return rc;
    ctx->device_output = on != 0;
    return CVO_HIP_OK;
}

int cvo_fe_set_num_want(cvo_fe_ctx *ctx, int num_want)
{
    if (!ctx || num_want < 1) return CVO_HIP_ERR_INVALID;
    ctx->num_want = num_want;
    return CVO_HIP_OK;
}

}   // extern "C"
