// cvo_class.cpp -- C++ registration objects over the C-ABI (see include/cvo.hpp).
#include "cvo.hpp"
#include "cvo_fe_rules.h"

#include <cmath>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace cvo_hip {

Affine3f::Affine3f()
{
    std::memset(m, 0, sizeof(m));
    m[0] = m[5] = m[10] = m[15] = 1.0f;
}

void Affine3f::translation(float t[3]) const
{
    t[0] = m[3]; t[1] = m[7]; t[2] = m[11];
}

void Affine3f::linear(float r[9]) const
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[3 * i + j] = m[4 * i + j];
}

void Affine3f::quaternion(float q[4]) const
{   // Eigen's quaternion-from-matrix (Shoemake), float
    const float m00 = m[0], m11 = m[5], m22 = m[10];
    float t = m00 + m11 + m22;
    float x, y, z, w;
    if (t > 0.0f) {
        t = std::sqrt(t + 1.0f);
        w = 0.5f * t;
        t = 0.5f / t;
        x = (m[9] - m[6]) * t;
        y = (m[2] - m[8]) * t;
        z = (m[4] - m[1]) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > m[5 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[5 * i] - m[5 * j] - m[5 * k] + 1.0f);
        float qv[3];
        qv[i] = 0.5f * t;
        t = 0.5f / t;
        w = (m[4 * k + j] - m[4 * j + k]) * t;
        qv[j] = (m[4 * j + i] + m[4 * i + j]) * t;
        qv[k] = (m[4 * k + i] + m[4 * i + k]) * t;
        x = qv[0]; y = qv[1]; z = qv[2];
    }
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

registration::registration(int mode, int device, void *stream)
    : init(false), iter(0), ctx_(nullptr), have_moving_(false), n_iter_(0), fe_(nullptr), fe_w_(0), fe_h_(0),
      fe_points_(0), device_(device), camera_(), have_camera_(false), depth_camera_(), have_depth_camera_(false),
      depth_gate_(), have_depth_gate_(false), mask_rows_(0), mask_cols_(0), have_mask_(false), stereo_(), have_stereo_(false),
      stereo_rig_(), have_stereo_rig_(false), stereo_paths_(CVO_FE_PATHS_4), stereo_speckle_(), have_stereo_speckle_(false),
      depth_median_(), have_depth_median_(false), depth_infill_(), have_depth_infill_(false), lidar_(), have_lidar_(false), lidar_sweep_(), have_lidar_sweep_(false), lidar_motion_(), select_mode_(CVO_FE_SELECT_IMAGE),
      pixel_format_(CVO_FE_PIXEL_BGR8), depth_format_(CVO_FE_DEPTH_U16), depth_unit_(1.0f), binning_(), have_binning_(false),
      photometric_(), have_photometric_(false), photo_rows_(0), photo_cols_(0), photo_gain_{1.0f, 1.0f, 1.0f}
{
    check(cvo_hip_default_params(mode, &params_), "cvo_hip_default_params");
    check(cvo_hip_init_state(&params_, &state_), "cvo_hip_init_state");
    check(cvo_hip_create(device, stream, &params_, &ctx_), "cvo_hip_create");
}

registration::~registration()
{
    if (fe_) cvo_fe_destroy(fe_);
    cvo_hip_destroy(ctx_);
}

// a call of the front end that did not succeed: what it was, the status, and why (`why` null: the front end's own text)
void registration::fe_check(int rc, const char *what, const char *why)
{
    if (rc == CVO_HIP_OK) return;
    throw std::runtime_error(std::string(what) + ": " + cvo_hip_error_string(rc) + " (" + (why ? why : cvo_fe_last_error(fe_)) +
                             ")");
}

// what the setters stored before the first image, for the front end that image created
void registration::apply_stored_settings()
{
    try {
        // (in front of the pixel format, which is then checked at the input size)
        if (have_binning_) fe_check(cvo_fe_set_input_binning(fe_, &binning_), "cvo_fe_set_input_binning");
        if (have_camera_) fe_check(cvo_fe_set_camera(fe_, &camera_), "cvo_fe_set_camera");
        if (have_depth_camera_) fe_check(cvo_fe_set_depth_camera(fe_, &depth_camera_), "cvo_fe_set_depth_camera");
        if (have_depth_gate_) fe_check(cvo_fe_set_depth_gate(fe_, &depth_gate_), "cvo_fe_set_depth_gate");
        if (have_stereo_) fe_check(cvo_fe_set_stereo(fe_, &stereo_), "cvo_fe_set_stereo");
        if (have_stereo_rig_) fe_check(cvo_fe_set_stereo_rig(fe_, &stereo_rig_), "cvo_fe_set_stereo_rig");
        fe_check(cvo_fe_set_stereo_paths(fe_, stereo_paths_), "cvo_fe_set_stereo_paths");
        if (have_stereo_speckle_) fe_check(cvo_fe_set_stereo_speckle(fe_, &stereo_speckle_), "cvo_fe_set_stereo_speckle");
        fe_check(cvo_fe_set_select_mode(fe_, select_mode_), "cvo_fe_set_select_mode");
        if (have_depth_median_) fe_check(cvo_fe_set_depth_median(fe_, &depth_median_), "cvo_fe_set_depth_median");
        if (have_depth_infill_) fe_check(cvo_fe_set_depth_infill(fe_, &depth_infill_), "cvo_fe_set_depth_infill");
        if (have_lidar_) fe_check(cvo_fe_set_lidar(fe_, &lidar_), "cvo_fe_set_lidar");
        if (have_lidar_sweep_) {
            fe_check(cvo_fe_set_lidar_sweep(fe_, &lidar_sweep_), "cvo_fe_set_lidar_sweep");
            fe_check(cvo_fe_set_lidar_motion(fe_, lidar_motion_), "cvo_fe_set_lidar_motion");
        }
        fe_check(cvo_fe_set_pixel_format(fe_, pixel_format_), "cvo_fe_set_pixel_format");
        fe_check(cvo_fe_set_depth_format(fe_, depth_format_, depth_unit_), "cvo_fe_set_depth_format");
        if (have_photometric_) apply_photometric();   // (behind the binning: the vignette is of the input size)
        if (have_mask_) {
            const bool fits = mask_rows_ == fe_h_ && mask_cols_ == fe_w_;
            fe_check(fits ? cvo_fe_set_mask(fe_, mask_.data(), (size_t)mask_cols_) : CVO_HIP_ERR_INVALID, "cvo_fe_set_mask",
                     fits ? nullptr : "the mask must have the colour image's size");
        }
    } catch (...) {
        // (no front end without its settings: the next image tries again instead of falling back to the table)
        cvo_fe_destroy(fe_);
        fe_ = nullptr;
        throw;
    }
}

// pcd_generator::load_image + create_pointcloud (ref src/cvo.cpp:321-341): cvo asks for
// the raw colour features (type 1), acvo for the HSV ones (type 0, ref
// src/adaptive_cvo.cpp:451,462).  The cloud never leaves the device: the front end's
// output arrays go straight into cvo_hip_set_*_device.
// `stereo`: `dep` is the right colour image of a rectified pair (cvo_fe_submit_stereo) and `rgb` the left one.
// `scan`: a LiDAR frame (cvo_fe_submit_lidar); `dep` is `rgb` again and is not read.
// `on_device`: the two views' `data` is device memory (cvo_fe_submit_device, cvo_fe_submit_stereo_device).
void registration::cloud_from_images(int dataset_seq, const image_view &rgb, const image_view &dep, bool stereo,
                                     const scan_view *scan, bool on_device)
{
    if (scan && !have_lidar_) throw std::runtime_error("set_pcd_lidar(): no scan source: set_lidar() first");
    if (!scan && have_lidar_)
        throw std::runtime_error("set_pcd(): a scan source is set, a frame is an image and a scan: set_pcd_lidar()");
    if (stereo && !have_stereo_) throw std::runtime_error("set_pcd_stereo(): no stereo settings: set_stereo() first");
    if (!stereo && have_stereo_)
        throw std::runtime_error("set_pcd(): stereo is set, a frame is a pair of colour images: set_pcd_stereo()");
    const bool own_size = !stereo && have_depth_camera_;
    if (!rgb.data || !dep.data || (!own_size && (rgb.rows != dep.rows || rgb.cols != dep.cols)))
        throw std::runtime_error(stereo ? "set_pcd_stereo(): the two colour images must have the same size"
                                        : "set_pcd(): colour and depth image must have the same size");
    if (own_size && (dep.rows != depth_camera_.height || dep.cols != depth_camera_.width))
        throw std::runtime_error("set_pcd(): the depth image must have the depth camera's size");
    // (input binning: the images are factor times the front end's size each way)
    const int bin = have_binning_ ? binning_.factor : 1;
    if (!fe_) {
        if (rgb.cols % bin != 0 || rgb.rows % bin != 0)
            throw std::runtime_error("set_pcd(): the image size is no multiple of the input binning's factor");
        const int rc = cvo_fe_create(device_, nullptr, rgb.cols / bin, rgb.rows / bin, &fe_);
        if (rc != CVO_HIP_OK) throw std::runtime_error(std::string("cvo_fe_create: ") + cvo_hip_error_string(rc));
        fe_w_ = rgb.cols / bin; fe_h_ = rgb.rows / bin;
        cvo_fe_set_device_output(fe_, 1);
        apply_stored_settings();
    }
    if (rgb.cols != bin * fe_w_ || rgb.rows != bin * fe_h_)
        throw std::runtime_error("set_pcd(): the image size changed within a sequence");
    const int ftype = params_.mode == CVO_HIP_MODE_ACVO ? CVO_FE_FEATURES_HSV : CVO_FE_FEATURES_RGB;
    int rc = scan   ? cvo_fe_submit_lidar(fe_, (const uint8_t *)rgb.data, rgb.step, scan->points, scan->stride_bytes,
                                          scan->num_points, dataset_seq, ftype)
             : on_device ? (stereo ? cvo_fe_submit_stereo_device(fe_, rgb.data, rgb.step, dep.data, dep.step, dataset_seq, ftype)
                                   : cvo_fe_submit_device(fe_, rgb.data, rgb.step, dep.data, dep.step, dataset_seq, ftype))
             : stereo ? cvo_fe_submit_stereo(fe_, (const uint8_t *)rgb.data, rgb.step, (const uint8_t *)dep.data, dep.step,
                                           dataset_seq, ftype)
                    : cvo_fe_submit(fe_, (const uint8_t *)rgb.data, rgb.step, (const uint16_t *)dep.data, dep.step,
                                    dataset_seq, ftype);
    const float *d_pos = nullptr, *d_feat = nullptr;
    if (rc == CVO_HIP_OK) rc = cvo_fe_collect_device(fe_, &d_pos, &d_feat, &fe_points_);
    fe_check(rc, "front end");
    if (init == false) {   // ref src/cvo.cpp:325-334
        std::cout << "initializing cvo..." << std::endl;
        check(cvo_hip_set_fixed_device(ctx_, d_pos, d_feat, fe_points_, CVO_HIP_FEAT_ROWMAJOR),
              "cvo_hip_set_fixed_device");
        std::cout << "first pcd generated!" << std::endl;
        init = true;
        return;
    }
    check(cvo_hip_set_moving_device(ctx_, d_pos, d_feat, fe_points_, CVO_HIP_FEAT_ROWMAJOR),
          "cvo_hip_set_moving_device");
    have_moving_ = true;
    std::cout << "num moving: " << fe_points_ << std::endl;   // ref src/cvo.cpp:343-347
}

// A setting given (`value`) or cleared (null): to the front end at once if there is one, and kept for the one the
// first image creates.  A refusal by the front end throws and leaves what was kept as it was.
template <class S>
void registration::store(int (*set)(cvo_fe_ctx *, const S *), const char *what, const S *value, S &kept, bool &have)
{
    if (fe_) fe_check(set(fe_, value), what);
    if (value) kept = *value;
    have = value != nullptr;
}

// (Without a front end yet, the host-only checks below refuse what its setters refuse: the answer does not wait
// for the first image.)
// "set_x(): " in front of the sentence the setter puts "set_x: " in front of (cvo_fe_rules.h)
namespace rules = cvo_fe_rules;

static std::runtime_error refused(const char *name, const char *rule)
{
    return std::runtime_error(std::string(name) + "(): " + rule);
}

void registration::set_camera(const cvo_fe_camera_model &model)
{
    int32_t qu = 0, qv = 0;
    if (cvo_fe_rectify_map(&model, 1, 1, &qu, &qv) != CVO_HIP_OK)
        throw refused("set_camera", rules::camera);
    if (!fe_ && have_stereo_rig_) throw std::runtime_error("set_camera(): a stereo rig is set: clear the rig first");
    store<cvo_fe_camera_model>(cvo_fe_set_camera, "cvo_fe_set_camera", &model, camera_, have_camera_);
}

void registration::clear_camera()
{
    store<cvo_fe_camera_model>(cvo_fe_set_camera, "cvo_fe_set_camera", nullptr, camera_, have_camera_);
}

void registration::set_depth_camera(const cvo_fe_depth_camera &rig)
{
    if (!fe_ && cvo_fe_check_depth_camera(&rig) != CVO_HIP_OK)
        throw refused("set_depth_camera", rules::depth_camera);
    if (!fe_ && have_lidar_) throw std::runtime_error("set_depth_camera(): a scan source is set");
    store<cvo_fe_depth_camera>(cvo_fe_set_depth_camera, "cvo_fe_set_depth_camera", &rig, depth_camera_, have_depth_camera_);
}

void registration::clear_depth_camera()
{
    store<cvo_fe_depth_camera>(cvo_fe_set_depth_camera, "cvo_fe_set_depth_camera", nullptr, depth_camera_, have_depth_camera_);
}

void registration::set_depth_gate(const cvo_fe_depth_gate &gate)
{
    if (!fe_ && cvo_fe_check_depth_gate(&gate) != CVO_HIP_OK)
        throw refused("set_depth_gate", rules::depth_gate);
    store<cvo_fe_depth_gate>(cvo_fe_set_depth_gate, "cvo_fe_set_depth_gate", &gate, depth_gate_, have_depth_gate_);
}

void registration::clear_depth_gate()
{
    store<cvo_fe_depth_gate>(cvo_fe_set_depth_gate, "cvo_fe_set_depth_gate", nullptr, depth_gate_, have_depth_gate_);
}

void registration::set_depth_median(const cvo_fe_depth_median &median)
{
    if (!fe_ && cvo_fe_check_depth_median(&median) != CVO_HIP_OK)
        throw refused("set_depth_median", rules::depth_median);
    store<cvo_fe_depth_median>(cvo_fe_set_depth_median, "cvo_fe_set_depth_median", &median, depth_median_, have_depth_median_);
}

void registration::clear_depth_median()
{
    store<cvo_fe_depth_median>(cvo_fe_set_depth_median, "cvo_fe_set_depth_median", nullptr, depth_median_, have_depth_median_);
}

void registration::set_depth_infill(const cvo_fe_depth_infill &infill)
{
    if (!fe_ && cvo_fe_check_depth_infill(&infill) != CVO_HIP_OK)
        throw refused("set_depth_infill", rules::depth_infill);
    store<cvo_fe_depth_infill>(cvo_fe_set_depth_infill, "cvo_fe_set_depth_infill", &infill, depth_infill_, have_depth_infill_);
}

void registration::clear_depth_infill()
{
    store<cvo_fe_depth_infill>(cvo_fe_set_depth_infill, "cvo_fe_set_depth_infill", nullptr, depth_infill_, have_depth_infill_);
}

void registration::set_lidar(const cvo_fe_lidar &lidar)
{
    if (!fe_ && cvo_fe_check_lidar(&lidar) != CVO_HIP_OK)
        throw refused("set_lidar", rules::lidar);
    if (!fe_ && (have_stereo_ || have_depth_camera_))
        throw std::runtime_error("set_lidar(): stereo or a depth camera is set");
    store<cvo_fe_lidar>(cvo_fe_set_lidar, "cvo_fe_set_lidar", &lidar, lidar_, have_lidar_);
}

void registration::clear_lidar()
{
    store<cvo_fe_lidar>(cvo_fe_set_lidar, "cvo_fe_set_lidar", nullptr, lidar_, have_lidar_);
    have_lidar_sweep_ = false;   // (the sweep goes with the scan source)
    for (float &t : lidar_motion_) t = 0.0f;
}

void registration::set_lidar_sweep(const cvo_fe_lidar_sweep &sweep)
{
    if (!fe_ && cvo_fe_check_lidar_sweep(&sweep) != CVO_HIP_OK)
        throw std::runtime_error("set_lidar_sweep(): a mode of CVO_FE_SWEEP_*, finite members, time_offset >= 12 and a "
                                 "multiple of 4, time_scale not 0, direction +1 or -1 under the azimuth mode and 0 "
                                 "otherwise, phase0 in [0, 1), s_ref in [0, 1], pad_ 0");
    if (!fe_ && !have_lidar_) throw std::runtime_error("set_lidar_sweep(): no scan source: set_lidar() first");
    store<cvo_fe_lidar_sweep>(cvo_fe_set_lidar_sweep, "cvo_fe_set_lidar_sweep", &sweep, lidar_sweep_, have_lidar_sweep_);
    for (float &t : lidar_motion_) t = 0.0f;
}

void registration::clear_lidar_sweep()
{
    store<cvo_fe_lidar_sweep>(cvo_fe_set_lidar_sweep, "cvo_fe_set_lidar_sweep", nullptr, lidar_sweep_, have_lidar_sweep_);
    for (float &t : lidar_motion_) t = 0.0f;
}

void registration::set_lidar_motion(const float twist[6])
{
    if (!twist) throw std::runtime_error("set_lidar_motion(): a twist holds six numbers");
    if (!have_lidar_sweep_) throw std::runtime_error("set_lidar_motion(): no sweep: set_lidar_sweep() first");
    double w2 = 0.0, v2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        w2 += (double)twist[k] * twist[k];
        v2 += (double)twist[3 + k] * twist[3 + k];
    }
    // (NaN fails both comparisons)
    if (!(w2 <= (double)CVO_FE_SWEEP_MAX_ROTATION * CVO_FE_SWEEP_MAX_ROTATION) ||
        !(v2 <= (double)CVO_FE_SWEEP_MAX_TRANSLATION * CVO_FE_SWEEP_MAX_TRANSLATION))
        throw refused("set_lidar_motion", rules::lidar_motion);
    if (fe_) fe_check(cvo_fe_set_lidar_motion(fe_, twist), "cvo_fe_set_lidar_motion");
    for (int k = 0; k < 6; ++k) lidar_motion_[k] = twist[k];
}

void registration::set_select_mode(int mode)
{
    if (!fe_ && cvo_fe_check_select_mode(mode) != CVO_HIP_OK)
        throw refused("set_select_mode", rules::select_mode);
    if (fe_) fe_check(cvo_fe_set_select_mode(fe_, mode), "cvo_fe_set_select_mode");
    select_mode_ = mode;
}

void registration::set_pixel_format(int format)
{
    // (before the first image there is no size yet: 2 x 2 fits every format, and a size the format does not fit throws
    // when that image creates the front end)
    if (!fe_ && cvo_fe_check_pixel_format(format, 2, 2) != CVO_HIP_OK)
        throw std::runtime_error("set_pixel_format(): one of CVO_FE_PIXEL_*");
    if (fe_) fe_check(cvo_fe_set_pixel_format(fe_, format), "cvo_fe_set_pixel_format");
    pixel_format_ = format;
}

void registration::set_input_binning(const cvo_fe_binning &binning)
{
    // (before the first image there is no size yet: 1 x 1 fits every factor, and a size over the limit throws when that
    // image creates the front end)
    if (!fe_ && cvo_fe_check_binning(&binning, 1, 1) != CVO_HIP_OK) throw refused("set_input_binning", rules::binning);
    store<cvo_fe_binning>(cvo_fe_set_input_binning, "cvo_fe_set_input_binning", &binning, binning_, have_binning_);
}

void registration::clear_input_binning()
{
    store<cvo_fe_binning>(cvo_fe_set_input_binning, "cvo_fe_set_input_binning", nullptr, binning_, have_binning_);
}

// the stored photometric setting to the front end: its tables, then the gains
void registration::apply_photometric()
{
    const uint16_t *vig = photo_vignette_.empty() ? nullptr : photo_vignette_.data();
    const int bin = have_binning_ ? binning_.factor : 1;
    const bool fits = !vig || (photo_rows_ == bin * fe_h_ && photo_cols_ == bin * fe_w_);
    fe_check(fits ? cvo_fe_set_photometric(fe_, &photometric_, photo_response_.empty() ? nullptr : photo_response_.data(), vig,
                                           (size_t)photo_cols_ * 2)
                  : CVO_HIP_ERR_INVALID,
             "cvo_fe_set_photometric", fits ? nullptr : "the vignette must have the size of the images handed over");
    if (photometric_.flags & CVO_FE_PHOTO_GAIN) fe_check(cvo_fe_set_photometric_gain(fe_, photo_gain_), "cvo_fe_set_photometric_gain");
}

void registration::set_photometric(const cvo_fe_photometric &photometric, const uint16_t *response, const uint16_t *vignette,
                                   int vignette_rows, int vignette_cols, size_t vignette_step)
{
    if (cvo_fe_check_photometric(&photometric, response != nullptr, vignette != nullptr) != CVO_HIP_OK)
        throw refused("set_photometric", rules::photometric);
    if (vignette && (vignette_rows < 1 || vignette_cols < 1 || vignette_step < (size_t)vignette_cols * 2 || vignette_step % 2 != 0))
        throw std::runtime_error("set_photometric(): a vignette of rows x cols uint16, rows an even number of bytes, at least the row's, apart");
    // kept first (the front end takes the dense copy); a refusal by the front end puts back what was kept before
    const cvo_fe_photometric old = photometric_;
    const bool had = have_photometric_;
    std::vector<uint16_t> old_r = photo_response_, old_v = photo_vignette_;
    const int old_rows = photo_rows_, old_cols = photo_cols_;
    const float old_gain[3] = {photo_gain_[0], photo_gain_[1], photo_gain_[2]};
    photometric_ = photometric;
    have_photometric_ = true;
    photo_response_.assign(response, response ? response + 768 : response);
    photo_vignette_.clear();
    for (int y = 0; vignette && y < vignette_rows; ++y) {
        const uint16_t *row = (const uint16_t *)((const uint8_t *)vignette + (size_t)y * vignette_step);
        photo_vignette_.insert(photo_vignette_.end(), row, row + vignette_cols);
    }
    photo_rows_ = vignette ? vignette_rows : 0;
    photo_cols_ = vignette ? vignette_cols : 0;
    for (float &g : photo_gain_) g = 1.0f;
    if (!fe_) return;
    try {
        apply_photometric();
    } catch (...) {
        photometric_ = old; have_photometric_ = had;
        photo_response_ = old_r; photo_vignette_ = old_v;
        photo_rows_ = old_rows; photo_cols_ = old_cols;
        for (int c = 0; c < 3; ++c) photo_gain_[c] = old_gain[c];
        throw;
    }
}

void registration::clear_photometric()
{
    if (fe_) fe_check(cvo_fe_set_photometric(fe_, nullptr, nullptr, nullptr, 0), "cvo_fe_set_photometric");
    have_photometric_ = false;
    photo_response_.clear();
    photo_vignette_.clear();
    photo_rows_ = photo_cols_ = 0;
}

void registration::set_photometric_gain(const float gain[3])
{
    if (!gain || !have_photometric_ || !(photometric_.flags & CVO_FE_PHOTO_GAIN))
        throw std::runtime_error("set_photometric_gain(): set_photometric() with CVO_FE_PHOTO_GAIN first");
    for (int c = 0; c < 3; ++c)
        if (!(gain[c] >= 0.0625f && gain[c] <= 15.99f)) throw refused("set_photometric_gain", rules::photometric_gain);
    if (fe_) fe_check(cvo_fe_set_photometric_gain(fe_, gain), "cvo_fe_set_photometric_gain");
    for (int c = 0; c < 3; ++c) photo_gain_[c] = gain[c];
}

void registration::set_depth_format(int format, float unit)
{
    if (!fe_ && cvo_fe_check_depth_format(format, unit) != CVO_HIP_OK)
        throw std::runtime_error("set_depth_format(): one of CVO_FE_DEPTH_*, a finite unit in [2^-20, 2^20], and a unit of 1 "
                                 "under CVO_FE_DEPTH_U16");
    if (fe_) fe_check(cvo_fe_set_depth_format(fe_, format, unit), "cvo_fe_set_depth_format");
    depth_format_ = format;
    depth_unit_ = unit;
}

void registration::set_stereo(const cvo_fe_stereo &stereo)
{
    if (!fe_ && cvo_fe_check_stereo(&stereo) != CVO_HIP_OK)
        throw refused("set_stereo", rules::stereo);
    if (!fe_ && have_lidar_) throw std::runtime_error("set_stereo(): a scan source is set");
    store<cvo_fe_stereo>(cvo_fe_set_stereo, "cvo_fe_set_stereo", &stereo, stereo_, have_stereo_);
}

void registration::clear_stereo()
{
    if (!fe_ && have_stereo_rig_) throw std::runtime_error("clear_stereo(): a stereo rig is set: clear the rig first");
    store<cvo_fe_stereo>(cvo_fe_set_stereo, "cvo_fe_set_stereo", nullptr, stereo_, have_stereo_);
}

void registration::set_stereo_paths(unsigned mask)
{
    if (!fe_ && cvo_fe_check_stereo_paths(mask) != CVO_HIP_OK)
        throw refused("set_stereo_paths", rules::stereo_paths);
    if (fe_) fe_check(cvo_fe_set_stereo_paths(fe_, mask), "cvo_fe_set_stereo_paths");
    stereo_paths_ = mask;
}

void registration::set_stereo_speckle(const cvo_fe_speckle &speckle)
{
    if (!fe_ && cvo_fe_check_speckle(&speckle) != CVO_HIP_OK)
        throw refused("set_stereo_speckle", rules::stereo_speckle);
    store<cvo_fe_speckle>(cvo_fe_set_stereo_speckle, "cvo_fe_set_stereo_speckle", &speckle, stereo_speckle_, have_stereo_speckle_);
}

void registration::clear_stereo_speckle()
{
    store<cvo_fe_speckle>(cvo_fe_set_stereo_speckle, "cvo_fe_set_stereo_speckle", nullptr, stereo_speckle_, have_stereo_speckle_);
}

void registration::set_stereo_rig(const cvo_fe_stereo_rig &rig)
{
    if (!fe_ && cvo_fe_check_stereo_rig(&rig) != CVO_HIP_OK)
        throw refused("set_stereo_rig", rules::stereo_rig);
    if (!fe_ && (!have_stereo_ || have_camera_))
        throw std::runtime_error("set_stereo_rig(): after set_stereo(), and without a camera model");
    store<cvo_fe_stereo_rig>(cvo_fe_set_stereo_rig, "cvo_fe_set_stereo_rig", &rig, stereo_rig_, have_stereo_rig_);
}

void registration::clear_stereo_rig()
{
    store<cvo_fe_stereo_rig>(cvo_fe_set_stereo_rig, "cvo_fe_set_stereo_rig", nullptr, stereo_rig_, have_stereo_rig_);
}

// the mask given or cleared (null); with a front end that one holds the bytes, and no second copy is kept here
void registration::store_mask(const image_view *mask)
{
    if (fe_) fe_check(cvo_fe_set_mask(fe_, mask ? (const uint8_t *)mask->data : nullptr, mask ? mask->step : 0), "cvo_fe_set_mask");
    mask_.clear();
    if (mask && !fe_) {
        mask_.resize((size_t)mask->rows * mask->cols);
        for (int y = 0; y < mask->rows; ++y)
            std::memcpy(mask_.data() + (size_t)y * mask->cols, (const uint8_t *)mask->data + (size_t)y * mask->step,
                        (size_t)mask->cols);
        mask_rows_ = mask->rows;
        mask_cols_ = mask->cols;
    }
    have_mask_ = mask != nullptr;
}

void registration::set_mask(const image_view &mask)
{
    if (!mask.data || mask.rows < 1 || mask.cols < 1 || mask.step < (size_t)mask.cols)
        throw std::runtime_error("set_mask(): a mask of rows x cols bytes, step >= cols");
    if (fe_ && (mask.rows != fe_h_ || mask.cols != fe_w_))
        throw std::runtime_error("set_mask(): the mask must have the colour image's size");
    store_mask(&mask);
}

void registration::set_mask(const uint8_t *mask, size_t stride)
{
    if (!fe_) throw std::runtime_error("set_mask(): no image yet, so no size: use the image_view form");
    set_mask(image_view{mask, fe_h_, fe_w_, stride});
}

void registration::clear_mask() { store_mask(nullptr); }


void registration::set_pcd(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img,
                           const std::string &, const std::string &)
{
    cloud_from_images(dataset_seq, RGB_img, dep_img, false);
}

void registration::set_pcd_stereo(const int dataset_seq, const image_view &left_img, const image_view &right_img)
{
    cloud_from_images(dataset_seq, left_img, right_img, true);
}

void registration::set_pcd_lidar(const int dataset_seq, const image_view &RGB_img, const void *points, size_t stride_bytes,
                                 int num_points)
{
    const scan_view scan{points, stride_bytes, num_points};
    cloud_from_images(dataset_seq, RGB_img, RGB_img, false, &scan);
}

void registration::run_cvo_lidar(const int dataset_seq, const image_view &RGB_img, const void *points, size_t stride_bytes,
                                 int num_points)
{
    const scan_view scan{points, stride_bytes, num_points};
    run_images(dataset_seq, RGB_img, RGB_img, false, &scan);
}

void registration::run_cvo(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img,
                           const std::string &, const std::string &)
{
    run_images(dataset_seq, RGB_img, dep_img, false);
}

void registration::run_cvo_stereo(const int dataset_seq, const image_view &left_img, const image_view &right_img)
{
    run_images(dataset_seq, left_img, right_img, true);
}

void registration::set_pcd_on_device(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img)
{
    cloud_from_images(dataset_seq, RGB_img, dep_img, false, nullptr, true);
}

void registration::run_cvo_on_device(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img)
{
    run_images(dataset_seq, RGB_img, dep_img, false, nullptr, true);
}

void registration::set_pcd_stereo_on_device(const int dataset_seq, const image_view &left_img, const image_view &right_img)
{
    cloud_from_images(dataset_seq, left_img, right_img, true, nullptr, true);
}

void registration::run_cvo_stereo_on_device(const int dataset_seq, const image_view &left_img, const image_view &right_img)
{
    run_images(dataset_seq, left_img, right_img, true, nullptr, true);
}

void registration::run_images(int dataset_seq, const image_view &rgb, const image_view &second, bool stereo,
                              const scan_view *scan, bool on_device)
{   // ref src/cvo.cpp:422-435
    const bool first = !init;
    cloud_from_images(dataset_seq, rgb, second, stereo, scan, on_device);
    if (first) return;
    align();
    std::cout << "Total iterations: " << iter << std::endl;
    std::cout << "RKHS-SE(3) Object Transformation Estimate: \n";
    for (int r = 0; r < 4; ++r)
        std::cout << transform.m[4 * r] << " " << transform.m[4 * r + 1] << " " << transform.m[4 * r + 2] << " "
                  << transform.m[4 * r + 3] << std::endl;
}

void registration::check(int status, const char *what)
{
    if (status == CVO_HIP_OK) return;
    std::string msg = std::string(what) + ": " + cvo_hip_error_string(status);
    if (ctx_) msg += std::string(" (") + cvo_hip_last_error(ctx_) + ")";
    throw std::runtime_error(msg);
}

void registration::publish()
{
    std::memcpy(transform.m, state_.transform, sizeof(transform.m));
    std::memcpy(prev_transform.m, state_.prev_transform, sizeof(prev_transform.m));
    std::memcpy(accum_transform.m, state_.accum_transform, sizeof(accum_transform.m));
    iter = state_.iter;
}

void registration::set_pcd(const point_cloud_view &pc)
{   // ref src/cvo.cpp:319-357
    if (init == false) {
        std::cout << "initializing cvo..." << std::endl;
        check(cvo_hip_set_fixed(ctx_, pc.positions, pc.features, pc.num_points, pc.feat_layout),
              "cvo_hip_set_fixed");
        std::cout << "first pcd generated!" << std::endl;
        init = true;
        return;
    }
    check(cvo_hip_set_moving(ctx_, pc.positions, pc.features, pc.num_points, pc.feat_layout),
          "cvo_hip_set_moving");
    have_moving_ = true;
}

void registration::align()
{   // ref src/cvo.cpp:361-420; the moving cloud becomes the fixed one (:417)
    if (!have_moving_) throw std::runtime_error("align(): set_pcd() must precede each align()");
    check(cvo_hip_align(ctx_, &state_, nullptr, 0, &n_iter_), "cvo_hip_align");
    check(cvo_hip_swap_moving_to_fixed(ctx_), "cvo_hip_swap_moving_to_fixed");
    have_moving_ = false;
    publish();
}

void registration::align(cvo_hip_pose_hessian_t *out)
{
    if (!out) {
        align();
        return;
    }
    if (!have_moving_) throw std::runtime_error("align(): set_pcd() must precede each align()");
    check(cvo_hip_align(ctx_, &state_, nullptr, 0, &n_iter_), "cvo_hip_align");
    check(cvo_hip_pose_hessian(ctx_, state_.R, state_.T, state_.ell, out), "cvo_hip_pose_hessian");
    check(cvo_hip_swap_moving_to_fixed(ctx_), "cvo_hip_swap_moving_to_fixed");
    have_moving_ = false;
    publish();
}

void registration::align(cvo_hip_pose_score_t *score, float score_ell, cvo_hip_pose_hessian_t *hessian)
{
    if (!have_moving_) throw std::runtime_error("align(): set_pcd() must precede each align()");
    check(cvo_hip_align(ctx_, &state_, nullptr, 0, &n_iter_), "cvo_hip_align");
    if (hessian) check(cvo_hip_pose_hessian(ctx_, state_.R, state_.T, state_.ell, hessian), "cvo_hip_pose_hessian");
    if (score)
        check(cvo_hip_pose_score(ctx_, state_.R, state_.T, score_ell > 0.0f ? score_ell : params_.ell_init, score),
              "cvo_hip_pose_score");
    check(cvo_hip_swap_moving_to_fixed(ctx_), "cvo_hip_swap_moving_to_fixed");
    have_moving_ = false;
    publish();
}

void registration::pose_score(const float R[9], const float T[3], float ell, cvo_hip_pose_score_t *out)
{
    check(cvo_hip_pose_score(ctx_, R, T, ell, out), "cvo_hip_pose_score");
}

void registration::pose_scan(const float *R9, const float *T3, int count, float ell, cvo_hip_pose_scan_entry *out,
                             cvo_hip_pose_scan_t *summary)
{
    check(cvo_hip_pose_scan(ctx_, R9, T3, count, ell, out, summary), "cvo_hip_pose_scan");
}

void registration::pose_matches(const float R[9], const float T[3], float ell, const cvo_hip_point_matches *fixed,
                                const cvo_hip_point_matches *moving, cvo_hip_pose_matches_t *summary)
{
    check(cvo_hip_pose_matches(ctx_, R, T, ell, fixed, moving, summary), "cvo_hip_pose_matches");
}

void registration::align_many(registration *const *objects, int count)
{
    std::vector<cvo_hip_ctx *> ctxs((size_t)count);
    std::vector<cvo_hip_state *> states((size_t)count);
    std::vector<int> iters((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        if (!objects[i] || !objects[i]->have_moving_)
            throw std::runtime_error("align_many(): set_pcd() must precede align() for every object");
        ctxs[(size_t)i] = objects[i]->ctx_;
        states[(size_t)i] = &objects[i]->state_;
    }
    const int rc = cvo_hip_align_many(ctxs.data(), states.data(), iters.data(), count);
    if (rc != CVO_HIP_OK) {
        for (int i = 0; i < count; ++i) {
            const char *d = cvo_hip_last_error(ctxs[(size_t)i]);
            if (d && d[0]) throw std::runtime_error(std::string("cvo_hip_align_many: ") + d);
        }
        throw std::runtime_error(std::string("cvo_hip_align_many: ") + cvo_hip_error_string(rc));
    }
    for (int i = 0; i < count; ++i) {
        registration *o = objects[i];
        o->n_iter_ = iters[(size_t)i];
        o->check(cvo_hip_swap_moving_to_fixed(o->ctx_), "cvo_hip_swap_moving_to_fixed");
        o->have_moving_ = false;
        o->publish();
    }
}

void registration::run_cvo(const point_cloud_view &pc)
{   // ref src/cvo.cpp:422-435
    if (init == false) {
        set_pcd(pc);
    } else {
        set_pcd(pc);
        align();
        std::cout << "Total iterations: " << iter << std::endl;
        std::cout << "RKHS-SE(3) Object Transformation Estimate: \n";
        for (int r = 0; r < 4; ++r)
            std::cout << transform.m[4 * r] << " " << transform.m[4 * r + 1] << " "
                      << transform.m[4 * r + 2] << " " << transform.m[4 * r + 3] << std::endl;
    }
}

}   // namespace cvo_hip

namespace acvo {

float acvo::function_inner_product(const cvo_hip::point_cloud_view *cloud_a,
                                   const cvo_hip::point_cloud_view *cloud_b)
{   // ref src/adaptive_cvo.cpp:385-439: two arbitrary clouds and the current ell; nothing else is read
    if (!cloud_a || !cloud_b || cloud_a->feat_layout != cloud_b->feat_layout)
        check(CVO_HIP_ERR_INVALID, "function_inner_product");
    float out = 0.0f;
    check(cvo_hip_function_inner_product_clouds(ctx_, state_.ell, cloud_a->positions, cloud_a->features,
                                                cloud_a->num_points, cloud_b->positions, cloud_b->features,
                                                cloud_b->num_points, cloud_a->feat_layout, &out),
          "cvo_hip_function_inner_product_clouds");
    return out;
}

}   // namespace acvo
