// cvo.hpp -- C++ host-side mirror of the reference's registration objects
// cvo::cvo (ref cpp/rkhs_registration/include/cvo.hpp:55-193) and acvo::acvo
// (ref include/adaptive_cvo.hpp:57-196), backed by the HIP C-ABI (cvo_hip.h).
//
// Same public surface: members init, iter, transform, prev_transform,
// accum_transform; methods set_pcd(), align(), run_cvo(); acvo additionally
// function_inner_product().  The reference's set_pcd()/run_cvo() take
// cv::Mat RGB/depth images and run the pcd_generator front end; here they take
// either an image_view pair (plain pointers in place of cv::Mat; the front end
// then runs on the GPU behind cvo_frontend.h) or directly the
// point_cloud a front end produced (positions + 5 features,
// ref include/data_type.h:59-71).  State carry-over between frames follows
// the reference object exactly (ell and R,T are not reset in cvo; acvo resets
// ell per pair): SURVEY 8a quirks 1-4, 10, 13.
//
// Error behaviour: the reference methods are void and fail by UB; these throw
// std::runtime_error carrying the C-ABI status text.
#pragma once

#include <string>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_hip.h"

namespace cvo_hip {

// Stand-in for the cv::Mat arguments of set_pcd() / run_cvo(): what cv::imread gives
// -- rows x cols pixels, `step` bytes per row; the colour image 3 bytes per pixel in
// file (B, G, R) order (or packed in the format of set_pixel_format()), the depth image one uint16 per pixel.
struct image_view {
    const void *data;
    int rows, cols;
    size_t step;
};

// Stand-in for Eigen::Affine3f: 4x4 row-major, matrix()(r,c) access.
struct Affine3f {
    float m[16];
    Affine3f();
    struct View {
        float *p;
        float &operator()(int r, int c) { return p[4 * r + c]; }
        float operator()(int r, int c) const { return p[4 * r + c]; }
    };
    View matrix() { return View{m}; }
    const float *data() const { return m; }
    void translation(float t[3]) const;
    void linear(float r[9]) const;
    // unit quaternion (x, y, z, w) of the rotation block, as
    // Eigen::Quaternionf(transform.linear()) gives it (ref src/cvo_main.cpp:61-64)
    void quaternion(float q[4]) const;
};

// A point cloud as the front end hands it over (ref data_type.h:59-71).
struct point_cloud_view {
    int num_points;
    const float *positions;   // n x 3 AoS
    const float *features;    // n x 5
    int feat_layout;          // CVO_HIP_FEAT_COLMAJOR (Eigen default) or _ROWMAJOR
};

class registration {
  public:
    bool init;
    int iter;
    Affine3f transform;
    Affine3f prev_transform;
    Affine3f accum_transform;

    explicit registration(int mode, int device = 0, void *stream = nullptr);
    ~registration();
    registration(const registration &) = delete;
    registration &operator=(const registration &) = delete;

    void set_pcd(const point_cloud_view &pc);
    void align();
    // align() that also evaluates the pose Hessian of the CVO objective at the final pose and length scale, before
    // the moving cloud becomes the fixed one (cvo_hip_pose_hessian; -H is the information-like quantity, no noise
    // model implied).  out == nullptr: plain align().  The registration is the same bit for bit either way.
    void align(cvo_hip_pose_hessian_t *out);
    // align() that also scores the registration at the final pose (cvo_hip_pose_score: the normalised CVO inner
    // product and the overlap) at length scale score_ell -- 0: params' ell_init, one scale for every pair of a
    // sequence -- and, if hessian is not null, evaluates the pose Hessian as align(hessian) does.  score == nullptr:
    // no score.  The registration is the same bit for bit either way.
    void align(cvo_hip_pose_score_t *score, float score_ell, cvo_hip_pose_hessian_t *hessian = nullptr);
    // cvo_hip_pose_score of the clouds set, at the pose (R, T) and length scale ell
    void pose_score(const float R[9], const float T[3], float ell, cvo_hip_pose_score_t *out);
    // cvo_hip_pose_scan of the clouds set: the scores of `count` candidate poses (R9 count x 9, T3 count x 3) at length scale
    // ell in one call -- out[k] belongs to pose k, summary->best is the index of the largest inner product (-1: no pose has
    // a member).  Where to start an align() whose true motion may be out of the kernel's reach.
    void pose_scan(const float *R9, const float *T3, int count, float ell, cvo_hip_pose_scan_entry *out,
                   cvo_hip_pose_scan_t *summary);
    // cvo_hip_pose_matches of the clouds set, at the pose (R, T) and length scale ell: which points matched.  fixed /
    // moving: the caller's arrays of one entry per point of that cloud, in the order the cloud was handed over (null: that
    // side is not wanted); summary: the counts and the inner product, cvo_hip_pose_score's of the same name.
    void pose_matches(const float R[9], const float T[3], float ell, const cvo_hip_point_matches *fixed,
                      const cvo_hip_point_matches *moving, cvo_hip_pose_matches_t *summary);
    void run_cvo(const point_cloud_view &pc);
    // The reference's own signatures (ref include/cvo.hpp:171-192): images in, the front
    // end (pcd_generator) runs first -- on the GPU.  The two paths are dead parameters
    // there too (ref src/cvo.cpp:332,341).
    void set_pcd(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img,
                 const std::string &pcd_pth = std::string(), const std::string &pcd_dso_pth = std::string());
    void run_cvo(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img,
                 const std::string &pcd_pth = std::string(), const std::string &pcd_dso_pth = std::string());
    // A camera of the caller's for the image form of set_pcd() / run_cvo() in place of the table row of
    // dataset_seq (which is then ignored): cvo_fe_set_camera.  A model with lens distortion makes every frame
    // start with the rectification of both images on the device (the contract: cvo_frontend.h).  May be called
    // before the first image; throws for a model the front end refuses.  clear_camera(): back to the table.
    void set_camera(const cvo_fe_camera_model &model);
    void clear_camera();
    // A depth camera of its own for the image form of set_pcd() / run_cvo(): cvo_fe_set_depth_camera.  The depth
    // image_view of every following frame is then rig.height x rig.width and is registered into the colour
    // camera's frame on the device (the contract: cvo_frontend.h).  May be called before the first image; throws
    // for a rig the front end refuses.  clear_depth_camera(): depth is registered to colour again.
    void set_depth_camera(const cvo_fe_depth_camera &rig);
    void clear_depth_camera();
    // A gate on the depth values for the image form of set_pcd() / run_cvo(): cvo_fe_set_depth_gate.  Pixels out
    // of range or on / beside a depth discontinuity give no point (the contract: cvo_frontend.h).  May be called
    // before the first image; throws for a gate the front end refuses.  clear_depth_gate(): no gate.
    void set_depth_gate(const cvo_fe_depth_gate &gate);
    void clear_depth_gate();
    // The median stage on the depth plane, in front of the gate, for the image form of set_pcd() / run_cvo(), depth or
    // stereo: cvo_fe_set_depth_median (the median contract: cvo_frontend.h).  A pixel with a depth takes the lower median
    // of its 3 x 3 or 5 x 5 window, and with fill_min > 0 a small hole is filled.  May be called before the first image;
    // throws for settings the front end refuses.  clear_depth_median(): no filter, a new object's state.
    void set_depth_median(const cvo_fe_depth_median &median);
    void clear_depth_median();
    // The infill stage on the depth plane, directly behind whatever fills it and in front of the median stage, for the
    // image form of set_pcd() / run_cvo() of every kind of frame: cvo_fe_set_depth_infill (the infill contract:
    // cvo_frontend.h).  A run of at most gap_x pixels without depth in a row, then of at most gap_y in a column, bounded
    // by depths of one surface, is bridged linearly in inverse depth.  May be called before the first image; throws for
    // settings the front end refuses.  clear_depth_infill(): no stage, a new object's state.
    void set_depth_infill(const cvo_fe_depth_infill &infill);
    void clear_depth_infill();
    // The selector's mode for the image form of set_pcd() / run_cvo(), depth or stereo: cvo_fe_set_select_mode
    // (CVO_FE_SELECT_IMAGE, a new object's: the reference's selector; CVO_FE_SELECT_DEPTH: a pixel without depth does
    // not compete, so the cloud holds the points asked for -- the selection contract: cvo_frontend.h).  A setting of
    // its own, before or after the first image; throws for a mode the front end refuses.
    void set_select_mode(int mode);
    // The pixel format of every colour image of the image form of set_pcd() / run_cvo() of every kind of frame, both
    // images of a stereo pair: cvo_fe_set_pixel_format (CVO_FE_PIXEL_BGR8, a new object's; the unpack contract:
    // cvo_frontend.h).  An image_view's rows and cols stay the picture's, and its step is the pitch of the packed rows
    // (cvo_fe_pixel_layout: NV12's chroma rows follow the picture's at the same pitch).  A setting of its own, before
    // or after the first image; throws for a format the front end refuses -- one the image size does not fit included,
    // which before the first image shows when that image arrives.
    void set_pixel_format(int format);
    // Input binning for the image form of set_pcd() / run_cvo() of every kind of frame: cvo_fe_set_input_binning (the
    // binning contract: cvo_frontend.h).  Every image handed over -- both of a stereo pair, the depth image unless a
    // depth camera is set -- is then `factor` (2, 3 or 4) times the front end's size each way and is binned on the device
    // in front of everything else.  Before the first image: that image's size over the factor is the front end's size.
    // With a front end: its size stays, and the images are factor times it from then on.  THE CAMERAS AND THE MASK OF
    // THE OBJECT DESCRIBE THE BINNED IMAGE: hand set_camera() cvo_fe_bin_camera's model and set_stereo_rig()
    // cvo_fe_bin_stereo_rig's rig, or the cloud comes out factor times too large.  Throws for what the front end
    // refuses.  clear_input_binning(): off, a new object's state.
    void set_input_binning(const cvo_fe_binning &binning);
    void clear_input_binning();
    // The photometric stage for the colour images of the image form of set_pcd() / run_cvo() of every kind of frame, both
    // images of a stereo pair: cvo_fe_set_photometric (the photometric contract: cvo_frontend.h).  `response`: 3 x 256
    // uint16 (B G R) with CVO_FE_PHOTO_RESPONSE, else null; `vignette`: Q12 gains of the size of the images handed over,
    // rows `vignette_step` bytes apart, with CVO_FE_PHOTO_VIGNETTE, else null.  Both are copied.  A setting of its own,
    // before or after the first image; throws for what the front end refuses -- a vignette of another size than the
    // images included, which before the first image shows when that image arrives.  set_photometric_gain(): the gains
    // (B G R) of the frames that follow under CVO_FE_PHOTO_GAIN (cvo_fe_set_photometric_gain); 1 after
    // set_photometric().  clear_photometric(): off, a new object's state.
    void set_photometric(const cvo_fe_photometric &photometric, const uint16_t *response = nullptr,
                         const uint16_t *vignette = nullptr, int vignette_rows = 0, int vignette_cols = 0,
                         size_t vignette_step = 0);
    void clear_photometric();
    void set_photometric_gain(const float gain[3]);
    // The format of the depth image of the image form of set_pcd() / run_cvo(): cvo_fe_set_depth_format
    // (CVO_FE_DEPTH_U16 with unit 1, a new object's; CVO_FE_DEPTH_F32 / CVO_FE_DEPTH_F16: the depth image_view's data is
    // float32 / float16 in `unit` metres per value and its step the pitch of those rows -- the depth-format contract:
    // cvo_frontend.h).  A setting of its own, before or after the first image; throws for what the front end refuses.
    void set_depth_format(int format, float unit = 1.0f);
    // set_pcd() / run_cvo() and the stereo pair for images that lie in DEVICE memory already: the views' `data` is
    // device memory of this object's device, in the layout of the host forms (the pixel and depth formats in force), and
    // never touches host memory: cvo_fe_submit_device / cvo_fe_submit_stereo_device (the device-input contract:
    // cvo_frontend.h).  What wrote the images must have completed before the call; they are read before it returns.
    void set_pcd_on_device(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img);
    void run_cvo_on_device(const int dataset_seq, const image_view &RGB_img, const image_view &dep_img);
    void set_pcd_stereo_on_device(const int dataset_seq, const image_view &left_img, const image_view &right_img);
    void run_cvo_stereo_on_device(const int dataset_seq, const image_view &left_img, const image_view &right_img);
    // A mask for every following frame: rows x cols bytes of the colour image's size, `step` bytes apart,
    // non-zero = no point from this pixel (cvo_fe_set_mask).  The bytes are copied.  May be called before the
    // first image: the copy is handed to the front end when it is created, and a mask of another size than that
    // image throws then.  The form without a size takes the size of the images seen so far, so it throws
    // before the first one.  clear_mask(): no mask.
    void set_mask(const image_view &mask);
    void set_mask(const uint8_t *mask, size_t stride);
    void clear_mask();
    // A rectified stereo pair in place of the depth image: cvo_fe_set_stereo.  A frame is then two colour images of
    // one size and goes in through set_pcd_stereo() / run_cvo_stereo() -- the image form of set_pcd() / run_cvo() for
    // two colour views, the left one the frame's colour image; a semi-global matcher on the device fills the depth
    // (the contract: cvo_frontend.h).  May be called before the first image; throws for settings the front end
    // refuses, and beside a depth camera or a camera model with lens distortion.  clear_stereo(): depth images again.
    void set_stereo(const cvo_fe_stereo &stereo);
    void clear_stereo();
    // The rig of a RAW stereo pair: cvo_fe_set_stereo_rig.  The pairs of set_pcd_stereo() / run_cvo_stereo() are then as
    // the two cameras deliver them and both images are rectified on the device in front of the matcher; the rig is the
    // camera of the frame (the contract: cvo_frontend.h; cvo_fe_stereo_rectify makes a rig from a calibration).  After
    // set_stereo(); throws for a rig the front end refuses, without stereo settings and beside a camera model.  While
    // a rig is set set_camera() and clear_stereo() throw.  clear_stereo_rig(): rectified pairs again.
    // The matcher's path mask: cvo_fe_set_stereo_paths (CVO_FE_PATHS_4, a new object's; CVO_FE_PATHS_8; any non-empty
    // subset of the eight bits; one launch per path).  A setting of its own beside set_stereo(): with or without
    // stereo settings, before or after the first image; throws for a mask the front end refuses.
    void set_stereo_paths(unsigned mask);
    // The matcher's speckle filter: cvo_fe_set_stereo_speckle (the speckle contract: cvo_frontend.h).  Components of the
    // disparity plane of max_size pixels at the most give no point.  A setting of its own beside set_stereo(), kept
    // across frames: with or without stereo settings, before or after the first image; throws for settings the front
    // end refuses.  clear_stereo_speckle(): no filter, a new object's state.
    void set_stereo_speckle(const cvo_fe_speckle &speckle);
    void clear_stereo_speckle();
    void set_stereo_rig(const cvo_fe_stereo_rig &rig);
    void clear_stereo_rig();
    void set_pcd_stereo(const int dataset_seq, const image_view &left_img, const image_view &right_img);
    void run_cvo_stereo(const int dataset_seq, const image_view &left_img, const image_view &right_img);
    // A LiDAR scan in place of the depth image: cvo_fe_set_lidar.  A frame is then a colour image and a scan and goes in
    // through set_pcd_lidar() / run_cvo_lidar() -- the image form of set_pcd() / run_cvo() with `num_points` records
    // `stride_bytes` apart, x y z first, in place of the depth image; the scan is projected into the colour camera on
    // the device (the LiDAR contract: cvo_frontend.h).  May be called before the first image; throws for settings the
    // front end refuses, and beside stereo or a depth camera.  clear_lidar(): depth images again.
    void set_lidar(const cvo_fe_lidar &lidar);
    void clear_lidar();
    // Motion compensation of a spinning scan: cvo_fe_set_lidar_sweep (the sweep contract: cvo_frontend.h).  Needs
    // set_lidar() first and goes with clear_lidar().  set_lidar_motion(): the scanner's own motion over one sweep, in
    // its own frame, w (radians per sweep) then v (metres per sweep), for the frames that follow
    // (cvo_fe_set_lidar_motion; cvo_fe_lidar_twist makes it from `transform`); zero after set_lidar_sweep().  May be
    // called before the first image; throw for what the front end refuses.  clear_lidar_sweep(): no compensation.
    void set_lidar_sweep(const cvo_fe_lidar_sweep &sweep);
    void clear_lidar_sweep();
    void set_lidar_motion(const float twist[6]);
    void set_pcd_lidar(const int dataset_seq, const image_view &RGB_img, const void *points, size_t stride_bytes,
                       int num_points);
    void run_cvo_lidar(const int dataset_seq, const image_view &RGB_img, const void *points, size_t stride_bytes,
                       int num_points);
    int num_points_last_frame() const { return fe_points_; }
    // Batched mode: align() of `count` objects (each with its moving cloud set) in
    // one call, their kernel launches shared (cvo_hip_align_many).  The result of
    // every object is what its own align() would have given.
    static void align_many(registration *const *objects, int count);

    int num_iterations() const { return n_iter_; }   // loop bodies executed by the last align()
    cvo_hip_ctx *context() { return ctx_; }
    const cvo_hip_state &state() const { return state_; }

  protected:
    cvo_hip_ctx *ctx_;
    cvo_hip_params params_;
    cvo_hip_state state_;
    bool have_moving_;
    int n_iter_;
    cvo_fe_ctx *fe_;           // front end, created with the first image (its size is fixed then)
    int fe_w_, fe_h_, fe_points_;
    int device_;
    cvo_fe_camera_model camera_;   // what set_camera() gave, for the front end created with the first image
    bool have_camera_;
    cvo_fe_depth_camera depth_camera_;   // what set_depth_camera() gave, likewise
    bool have_depth_camera_;
    cvo_fe_depth_gate depth_gate_;       // what set_depth_gate() gave, likewise
    bool have_depth_gate_;
    std::vector<uint8_t> mask_;          // what set_mask() gave (dense rows), likewise
    int mask_rows_, mask_cols_;
    bool have_mask_;
    cvo_fe_stereo stereo_;               // what set_stereo() gave, likewise
    bool have_stereo_;
    cvo_fe_stereo_rig stereo_rig_;       // what set_stereo_rig() gave, likewise
    bool have_stereo_rig_;
    uint32_t stereo_paths_;              // what set_stereo_paths() gave, likewise (CVO_FE_PATHS_4 without a call)
    cvo_fe_speckle stereo_speckle_;      // what set_stereo_speckle() gave, likewise
    bool have_stereo_speckle_;
    cvo_fe_depth_median depth_median_;   // what set_depth_median() gave, likewise
    bool have_depth_median_;
    cvo_fe_depth_infill depth_infill_;   // what set_depth_infill() gave, likewise
    bool have_depth_infill_;
    cvo_fe_lidar lidar_;                 // what set_lidar() gave, likewise
    bool have_lidar_;
    cvo_fe_lidar_sweep lidar_sweep_;     // what set_lidar_sweep() gave, likewise, and the twist of set_lidar_motion()
    bool have_lidar_sweep_;
    float lidar_motion_[6];
    int select_mode_;                    // what set_select_mode() gave, likewise (CVO_FE_SELECT_IMAGE without a call)
    int pixel_format_;                   // what set_pixel_format() gave, likewise (CVO_FE_PIXEL_BGR8 without a call)
    int depth_format_;                   // what set_depth_format() gave, likewise (CVO_FE_DEPTH_U16, unit 1 without a call)
    float depth_unit_;
    cvo_fe_binning binning_;             // what set_input_binning() gave, likewise
    bool have_binning_;
    cvo_fe_photometric photometric_;     // what set_photometric() gave, likewise, with its tables (dense rows) and the gains
    bool have_photometric_;
    std::vector<uint16_t> photo_response_, photo_vignette_;
    int photo_rows_, photo_cols_;
    float photo_gain_[3];
    void check(int status, const char *what);
    void fe_check(int status, const char *what, const char *why = nullptr);
    void apply_stored_settings();
    void apply_photometric();
    template <class S>
    void store(int (*set)(cvo_fe_ctx *, const S *), const char *what, const S *value, S &kept, bool &have);
    void store_mask(const image_view *mask);
    void publish();
    struct scan_view {   // the scan of a LiDAR frame: what stands in the depth image's place
        const void *points;
        size_t stride_bytes;
        int num_points;
    };
    void cloud_from_images(int dataset_seq, const image_view &rgb, const image_view &dep, bool stereo,
                           const scan_view *scan = nullptr, bool on_device = false);
    void run_images(int dataset_seq, const image_view &rgb, const image_view &second, bool stereo,
                    const scan_view *scan = nullptr, bool on_device = false);
};

}   // namespace cvo_hip

namespace cvo {
class cvo : public cvo_hip::registration {
  public:
    explicit cvo(int device = 0, void *stream = nullptr)
        : cvo_hip::registration(CVO_HIP_MODE_CVO, device, stream) {}
};
}   // namespace cvo

namespace acvo {
class acvo : public cvo_hip::registration {
  public:
    explicit acvo(int device = 0, void *stream = nullptr)
        : cvo_hip::registration(CVO_HIP_MODE_ACVO, device, stream) {}
    // ref include/adaptive_cvo.hpp:179, src/adaptive_cvo.cpp:385-439 (public, never called in
    // the tree): the inner-product statistic of two arbitrary clouds at the current
    // length-scale.  Reads nothing else and changes nothing: a pending set_pcd() stays pending.
    float function_inner_product(const cvo_hip::point_cloud_view *cloud_a,
                                 const cvo_hip::point_cloud_view *cloud_b);
};
}   // namespace acvo
