// cvo_fe_rules.h -- what each setting of the front end accepts, once: the sentence a refusal gives, and the predicate
// it describes.  The setters (cvo_fe_settings.cpp) say "set_x: " + sentence, the registration objects' checks in front
// of the first image (cvo_class.cpp) "set_x(): " + sentence.  Where the two have always worded a rule differently
// (the sweep, the pixel format, the depth format) each keeps its own text where it is said, and nothing is shared.
#ifndef CVO_FE_RULES_H
#define CVO_FE_RULES_H

#include "cvo_frontend.h"

// (internal to the library: not among its exported symbols)
namespace cvo_fe_rules __attribute__((visibility("hidden"))) {

constexpr const char *camera = "members must be finite and fx, fy, depth_scale positive";
constexpr const char *depth_camera =
    "size in [8, 8192], finite members, fx, fy, depth_scale positive, max_range above min_range, R a rotation";
constexpr const char *depth_gate =
    "finite members, jump_rel >= 0, max_range above min_range, grow in [0, 3], hole_border 0 or 1, pad_ 0";
constexpr const char *stereo =
    "baseline positive and finite, max_disp a multiple of 8 in [8, 128], min_disp >= 1, 1 <= p1 <= p2 <= 255, "
    "uniqueness in [0, 99], lr_max in [-1, 8], pad_ 0";
constexpr const char *stereo_paths = "a non-empty subset of the eight bits, 1 <= mask <= 0xFF";
constexpr const char *select_mode = "CVO_FE_SELECT_IMAGE or CVO_FE_SELECT_DEPTH";
constexpr const char *stereo_speckle = "max_size in [1, 2^26], max_diff in [0, 65535]";
constexpr const char *depth_median = "radius 1 or 2, fill_min in [0, (2*radius+1)^2 - 1], pad_ 0";
constexpr const char *depth_infill = "gap_x in [0, 15], gap_y in [0, 31], jump_rel finite and >= 0, pad_ 0";
constexpr const char *lidar =
    "max_points in [1, 2^21], splat in [0, 3], finite members, occl_rel >= 0, occl_rx and occl_ry in [0, 7], "
    "max_range above min_range, R a rotation, pad_ 0";
constexpr const char *lidar_motion = "finite members, |w| <= 1 radian and |v| <= 64 metres per sweep";
constexpr const char *stereo_rig =
    "finite members, every fx, fy, depth_scale and baseline positive, R_left and R_right rotations";
constexpr const char *binning =
    "factor 2, 3 or 4, depth_min in [1, factor^2], pad_ 0, factor times the context's width and height at most 8192";
constexpr const char *photometric =
    "flags a non-empty OR of CVO_FE_PHOTO_* without both GAIN and AUTO, 0 <= lo <= hi <= 255, min_count >= 1, per_channel 0 "
    "or 1, every target at most 65535, 1 <= gain_min <= gain_max <= 65535, pad_ 0, a response table exactly with "
    "CVO_FE_PHOTO_RESPONSE and a vignette exactly with CVO_FE_PHOTO_VIGNETTE";
constexpr const char *photometric_gain = "three finite gains in [1/16, 15.99]";
// The predicates (cvo_fe_settings.cpp), for the setters and for the host-only helpers that take the same structures.
bool model_ok(const cvo_fe_camera_model &m);
bool rotation_ok(const float R[9]);
bool rig_ok(const cvo_fe_depth_camera &r);
bool srig_ok(const cvo_fe_stereo_rig &r);
bool lidar_ok(const cvo_fe_lidar &l);
bool sweep_ok(const cvo_fe_lidar_sweep &sw);
bool twist_ok(const float twist[6]);
bool gate_ok(const cvo_fe_depth_gate &g);
bool stereo_ok(const cvo_fe_stereo &s);

inline bool distorts(const float dist[5])
{
    bool any = false;
    for (int q = 0; q < 5; ++q) any = any || dist[q] != 0.0f;
    return any;
}

}   // namespace cvo_fe_rules

#endif
