// cvo_fe_calib.cpp -- the host-only calibration helpers of include/cvo_frontend.h: the rectification map of a camera
// model, the ray table of a depth camera, the depth table of the stereo matcher, the rig of a stereo calibration and
// its maps, and the twist of a scanner from a camera's motion.  Float64 on the host, operation by operation; no
// context and no call of the runtime.  The tables are held to their numpy restatements by bytes, and the arithmetic
// contract of the library (-ffp-contract=off) is what keeps them so.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "cvo_frontend.h"
#include "cvo_fe_rules.h"

using namespace cvo_fe_rules;

namespace {

// The lens model of include/cvo_frontend.h for a colour or a depth camera, operation by operation (float64,
// nothing contracted).  The tables made from it are held to their numpy restatements by bytes, so every
// parenthesis here is part of the contract.
struct Lens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    template <class M>
    explicit Lens(const M &m)
        : fx(m.fx), fy(m.fy), cx(m.cx), cy(m.cy), k1(m.dist[0]), k2(m.dist[1]), p1(m.dist[2]), p2(m.dist[3]), k3(m.dist[4])
    {
    }
    // the radial factor and the tangential shift at the ideal point (x, y)
    void terms(double x, double y, double &rad, double &dx, double &dy) const
    {
        const double r2 = x * x + y * y;
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
        dx = (2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x);
        dy = p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y;
    }
    // the pixel at which the camera sees the ideal point (x, y)
    void project(double x, double y, double &us, double &vs) const
    {
        double rad, dx, dy;
        terms(x, y, rad, dx, dy);
        const double xd = x * rad + dx, yd = y * rad + dy;
        us = fx * xd + cx;
        vs = fy * yd + cy;
    }
};

// a source position as the entry of a map: clamped to [-1, w] x [-1, h] and in 1/32 pixel (the rectification contract)
inline void map_entry(double us, double vs, double wmax, double hmax, int32_t &qu, int32_t &qv)
{
    if (!(us >= -1.0)) us = -1.0;   // (also what is not a number)
    if (us > wmax) us = wmax;
    if (!(vs >= -1.0)) vs = -1.0;
    if (vs > hmax) vs = hmax;
    qu = (int32_t)std::nearbyint(32.0 * us);   // ties to even (the default rounding mode)
    qv = (int32_t)std::nearbyint(32.0 * vs);
}

}   // namespace

extern "C" {

int cvo_fe_rectify_map(const cvo_fe_camera_model *model, int width, int height, int32_t *qu, int32_t *qv)
{
    if (!model || !qu || !qv || width < 1 || height < 1 || !model_ok(*model)) return CVO_HIP_ERR_INVALID;
    const Lens lens(*model);
    const double wmax = (double)width, hmax = (double)height;
    for (int v = 0; v < height; ++v) {
        const double y = ((double)v - lens.cy) / lens.fy;
        for (int u = 0; u < width; ++u) {
            const double x = ((double)u - lens.cx) / lens.fx;
            double us, vs;
            lens.project(x, y, us, vs);
            const size_t i = (size_t)v * width + u;
            map_entry(us, vs, wmax, hmax, qu[i], qv[i]);
        }
    }
    return CVO_HIP_OK;
}

int cvo_fe_depth_rays(const cvo_fe_depth_camera *rig, float *xn, float *yn)
{
    if (!rig || !xn || !yn || !rig_ok(*rig)) return CVO_HIP_ERR_INVALID;
    const Lens lens(*rig);
    const bool bent = distorts(rig->dist);
    const double nan = std::nan("");
    for (int j = 0; j <= rig->height; ++j) {
        const double py = (double)j - 0.5, yd = (py - lens.cy) / lens.fy;
        for (int i = 0; i <= rig->width; ++i) {
            const double px = (double)i - 0.5, xd = (px - lens.cx) / lens.fx;
            double x = xd, y = yd;
            if (bent) {
                for (int it = 0; it < 20; ++it) {   // the fixed-point step
                    double rad, dx, dy;
                    lens.terms(x, y, rad, dx, dy);
                    x = (xd - dx) / rad;
                    y = (yd - dy) / rad;
                }
                double us, vs;   // the forward check
                lens.project(x, y, us, vs);
                if (!(std::fabs(us - px) <= 1.0 / 32.0 && std::fabs(vs - py) <= 1.0 / 32.0)) x = y = nan;
            }
            const size_t c = (size_t)j * ((size_t)rig->width + 1) + i;
            xn[c] = (float)x;
            yn[c] = (float)y;
        }
    }
    return CVO_HIP_OK;
}

int cvo_fe_stereo_depth_table(const cvo_fe_stereo *st, float fx, float depth_scale, uint16_t *out)
{
    if (!st || !out || !stereo_ok(*st) || !std::isfinite(fx) || !std::isfinite(depth_scale) || !(fx > 0.0f) ||
        !(depth_scale > 0.0f))
        return CVO_HIP_ERR_INVALID;
    // contract 9, operation by operation in float64 (nothing can be contracted: there is no addition)
    const double num = (((double)fx * (double)st->baseline) * (double)depth_scale) * 16.0;
    const int n = 16 * st->max_disp, q0 = 16 * st->min_disp;
    for (int q = 0; q < n; ++q) {
        double u = 0.0;
        if (q >= q0) u = std::nearbyint(num / (double)q);   // (ties to even: the default rounding mode)
        out[q] = (u >= 1.0 && u <= 65535.0) ? (uint16_t)u : (uint16_t)0;
    }
    return CVO_HIP_OK;
}

int cvo_fe_lidar_twist(const float T_cam[16], const cvo_fe_lidar *l, float sweep_fraction, float twist[6])
{
    if (!T_cam || !l || !twist || !std::isfinite(sweep_fraction) || !(sweep_fraction > 0.0f)) return CVO_HIP_ERR_INVALID;
    for (int q = 0; q < 16; ++q)
        if (!std::isfinite(T_cam[q])) return CVO_HIP_ERR_INVALID;
    cvo_fe_lidar checked = *l;
    checked.max_points = 1;   // (not read)
    float Rc[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rc[3 * r + c] = T_cam[4 * r + c];
    if (!lidar_ok(checked) || !rotation_ok(Rc)) return CVO_HIP_ERR_INVALID;
    // M = [R | T]^-1 = [R^T | -R^T T]: the later camera's pose in the earlier camera's frame
    double M[9], m[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (double)T_cam[4 * c + r];
        m[r] = -((double)T_cam[r] * T_cam[3] + (double)T_cam[4 + r] * T_cam[7] + (double)T_cam[8 + r] * T_cam[11]);
    }
    // X^-1 M X with X = [Rx | Tx]: the rotation Rx^T M Rx, the translation Rx^T (M Tx + m - Tx)
    double Rx[9], Tx[3], MRx[9], S[9], u[3], t[3];
    for (int q = 0; q < 9; ++q) Rx[q] = (double)l->R[q];
    for (int q = 0; q < 3; ++q) Tx[q] = (double)l->T[q];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) MRx[3 * r + c] = M[3 * r] * Rx[c] + M[3 * r + 1] * Rx[3 + c] + M[3 * r + 2] * Rx[6 + c];
        u[r] = (M[3 * r] * Tx[0] + M[3 * r + 1] * Tx[1] + M[3 * r + 2] * Tx[2]) + m[r] - Tx[r];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) S[3 * r + c] = Rx[r] * MRx[c] + Rx[3 + r] * MRx[3 + c] + Rx[6 + r] * MRx[6 + c];
        t[r] = Rx[r] * u[0] + Rx[3 + r] * u[1] + Rx[6 + r] * u[2];
    }
    // the logarithm: w = theta * axis from the antisymmetric part, v = V^-1 t, V^-1 = I - W/2 + k W^2
    const double ax[3] = {0.5 * (S[7] - S[5]), 0.5 * (S[2] - S[6]), 0.5 * (S[3] - S[1])};   // sin(theta) * axis
    const double sn = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const double cs = 0.5 * ((S[0] + S[4] + S[8]) - 1.0);
    const double theta = std::atan2(sn, cs);
    if (!(theta * (double)sweep_fraction <= (double)CVO_FE_SWEEP_MAX_ROTATION)) return CVO_HIP_ERR_INVALID;
    if (theta > 3.0) return CVO_HIP_ERR_INVALID;   // (too near a half turn for the logarithm, whatever the fraction)
    const double f = theta < 1e-6 ? 1.0 + theta * theta / 6.0 : theta / sn;   // theta / sin(theta)
    const double w[3] = {f * ax[0], f * ax[1], f * ax[2]};
    // (1 - (theta/2) cot(theta/2)) / theta^2, from the angle itself: 1 - cos from the matrix would keep the matrix's rounding
    const double t2 = theta * theta;
    const double k = theta < 1e-2 ? 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0
                                  : (1.0 - 0.5 * theta * std::cos(0.5 * theta) / std::sin(0.5 * theta)) / t2;
    const double wt[3] = {w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0]};
    const double wwt[3] = {w[1] * wt[2] - w[2] * wt[1], w[2] * wt[0] - w[0] * wt[2], w[0] * wt[1] - w[1] * wt[0]};
    double out[6];
    for (int q = 0; q < 3; ++q) {
        out[q] = w[q] * (double)sweep_fraction;
        out[3 + q] = ((t[q] - 0.5 * wt[q]) + k * wwt[q]) * (double)sweep_fraction;
    }
    float res[6];
    for (int q = 0; q < 6; ++q) res[q] = (float)out[q];
    if (!twist_ok(res)) return CVO_HIP_ERR_INVALID;
    for (int q = 0; q < 6; ++q) twist[q] = res[q];
    return CVO_HIP_OK;
}

int cvo_fe_stereo_rectify(const cvo_fe_stereo_calib *calib, int width, int height, cvo_fe_stereo_rig *out, float depth_scale)
{
    static_assert(sizeof(cvo_fe_stereo_calib) == 30 * sizeof(float), "120 bytes, no padding");
    if (!calib || !out || width < 1 || height < 1) return CVO_HIP_ERR_INVALID;
    const float *cf = &calib->left.fx;   // floats only
    for (int q = 0; q < 30; ++q)
        if (!std::isfinite(cf[q])) return CVO_HIP_ERR_INVALID;
    if (!std::isfinite(depth_scale) || !(depth_scale > 0.0f)) return CVO_HIP_ERR_INVALID;
    if (!(calib->left.fx > 0.0f && calib->left.fy > 0.0f && calib->right.fx > 0.0f && calib->right.fy > 0.0f))
        return CVO_HIP_ERR_INVALID;
    if (!rotation_ok(calib->R)) return CVO_HIP_ERR_INVALID;
    // the helper of the rig contract, step by step in float64
    double R[9], T[3];
    for (int q = 0; q < 9; ++q) R[q] = (double)calib->R[q];
    for (int q = 0; q < 3; ++q) T[q] = (double)calib->T[q];
    // 1: the axis-angle of R
    const double c = (((R[0] + R[4]) + R[8]) - 1.0) / 2.0;
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double n = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double angle = std::atan2(n / 2.0, c);
    if (!(angle <= 0.5)) return CVO_HIP_ERR_INVALID;
    double k[3] = {0.0, 0.0, 0.0};
    if (n > 0.0)
        for (int q = 0; q < 3; ++q) k[q] = v[q] / n;
    // 2: half the way each, by Rodrigues' formula
    const double K[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
    double KK[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) KK[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
    double Rl0[9], Rr0[9];
    const double sl = std::sin(angle / 2.0), cl = 1.0 - std::cos(angle / 2.0);
    for (int q = 0; q < 9; ++q) {
        const double eye = (q % 4 == 0) ? 1.0 : 0.0;
        Rl0[q] = (eye + sl * K[q]) + cl * KK[q];
        Rr0[q] = (eye - sl * K[q]) + cl * KK[q];
    }
    // 3: the direction from the left centre to the right one
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = (Rr0[3 * i] * T[0] + Rr0[3 * i + 1] * T[1]) + Rr0[3 * i + 2] * T[2];
    const double b = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (!(b > 0.0)) return CVO_HIP_ERR_INVALID;
    const double e1[3] = {-t[0] / b, -t[1] / b, -t[2] / b};
    if (!(e1[0] > 0.0 && e1[0] >= std::fabs(e1[1]) && e1[0] >= std::fabs(e1[2]))) return CVO_HIP_ERR_INVALID;
    // 4: (0, 0, 1) x e1 = (-e1.y, e1.x, 0)
    const double n2 = std::sqrt(e1[1] * e1[1] + e1[0] * e1[0]);
    const double e2[3] = {-e1[1] / n2, e1[0] / n2, 0.0};
    const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double W[9] = {e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], e3[0], e3[1], e3[2]};
    double Rk[2][9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Rk[0][3 * i + j] = (W[3 * i] * Rl0[j] + W[3 * i + 1] * Rl0[3 + j]) + W[3 * i + 2] * Rl0[6 + j];
            Rk[1][3 * i + j] = (W[3 * i] * Rr0[j] + W[3 * i + 1] * Rr0[3 + j]) + W[3 * i + 2] * Rr0[6 + j];
        }
    // 5, 6: one focal length, and the centre that puts the mean of the two optical axes in the middle of the image
    const double f = ((double)calib->left.fy + (double)calib->right.fy) / 2.0;
    const double mx = (f * Rk[0][2] / Rk[0][8] + f * Rk[1][2] / Rk[1][8]) / 2.0;
    const double my = (f * Rk[0][5] / Rk[0][8] + f * Rk[1][5] / Rk[1][8]) / 2.0;
    // 7
    cvo_fe_stereo_rig r{};
    r.left = calib->left;
    r.right = calib->right;
    for (int q = 0; q < 9; ++q) { r.R_left[q] = (float)Rk[0][q]; r.R_right[q] = (float)Rk[1][q]; }
    r.fx = r.fy = (float)f;
    r.cx = (float)(((double)width - 1.0) / 2.0 - mx);
    r.cy = (float)(((double)height - 1.0) / 2.0 - my);
    r.baseline = (float)b;
    r.depth_scale = depth_scale;
    if (!srig_ok(r)) return CVO_HIP_ERR_INVALID;   // (a baseline that rounds to 0, a centre that overflows)
    *out = r;
    return CVO_HIP_OK;
}

int cvo_fe_stereo_rig_map(const cvo_fe_stereo_rig *rig, int which, int width, int height, int32_t *qu, int32_t *qv)
{
    if (!rig || !qu || !qv || width < 1 || height < 1 || (which != 0 && which != 1) || !srig_ok(*rig)) return CVO_HIP_ERR_INVALID;
    const Lens lens(which ? rig->right : rig->left);
    double R[9];
    for (int q = 0; q < 9; ++q) R[q] = (double)(which ? rig->R_right : rig->R_left)[q];
    const double fx = (double)rig->fx, fy = (double)rig->fy, cx = (double)rig->cx, cy = (double)rig->cy;
    const double wmax = (double)width, hmax = (double)height;
    for (int v = 0; v < height; ++v) {
        const double yr = ((double)v - cy) / fy;
        for (int u = 0; u < width; ++u) {
            const double xr = ((double)u - cx) / fx;
            // R^T applied to (xr, yr, 1): from the rectified frame back into the camera's
            const double X = (R[0] * xr + R[3] * yr) + R[6];
            const double Y = (R[1] * xr + R[4] * yr) + R[7];
            const double Z = (R[2] * xr + R[5] * yr) + R[8];
            double us = -1.0, vs = -1.0;
            if (Z > 0.0) lens.project(X / Z, Y / Z, us, vs);
            const size_t i = (size_t)v * width + u;
            map_entry(us, vs, wmax, hmax, qu[i], qv[i]);
        }
    }
    return CVO_HIP_OK;
}

}   // extern "C"
