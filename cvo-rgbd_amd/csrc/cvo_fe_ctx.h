// cvo_fe_ctx.h -- the front end's context and what every translation unit that touches it needs: the structure
// itself, the owners of its buffers, the error and allocation helpers of its entry points, and the one-line views
// that say which buffer plays which part under the settings in force.  Internal to csrc/: cvo_frontend.hip (the
// kernels and a frame's sequence) and cvo_fe_settings.cpp (the setters and getters) include it.
#ifndef CVO_FE_CTX_H
#define CVO_FE_CTX_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cvo_frontend.h"
#include "cvo_depthfmt.h"
#include "cvo_photo.h"

constexpr int FE_LEVELS = 3;
constexpr int FE_GATE_MAX_GROW = 3;   // the largest `grow` k_fe_depth_gate is built for

// (FeCtrl is a parameter of kernels in cvo_frontend.hip's unnamed namespace and so part of their names: it stays in
// an unnamed namespace, which keeps those names what they were.  It is a plain block of ints, the same in every
// translation unit.)
namespace {

// device-resident control words of one frame
struct FeCtrl {
    int n[2][3];        // pixels chosen at level 0 / 1 / 2 by selection pass 0 / 1
    int pot[2];         // potential of pass 0 / 1
    int redo;           // pass 1 runs
    int do_sub;         // the map is sub-sampled
    int char_th;        // ... with this threshold on the random bytes
    int num_have;       // pixels chosen by the pass that counts
    int in_map;         // pixels in the map when the cloud was emitted
    int pad2_[2];
    int num_points;     // selected pixels with depth
    int changed;        // hysteresis sweep flag
    int pad_;
};

}   // namespace

struct FeDims {
    int w, h;
    int wl[FE_LEVELS], hl[FE_LEVELS];
    int w32, h32;
};

struct FeGraph {
    uint64_t key = 0;
    uint64_t cam_gen = 0;   // the context's camera generation the graph was captured at
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// A buffer and its release.  Every buffer of the context is held by one of these, and so is every buffer a
// setter builds: whatever is not handed on frees itself.  Launch sites take the raw pointer (get()).
struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
struct PinFree { void operator()(void *p) const { (void)hipHostFree(p); } };
template <class T> using Dev = std::unique_ptr<T, DevFree>;   // device memory
template <class T> using Pin = std::unique_ptr<T, PinFree>;   // pinned host memory

struct cvo_fe_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    FeDims d{};
    int np = 0, nblk = 0, nchunks = 0;
    int num_want = 3000;
    int cap = 0;
    // device
    Dev<uint8_t> img, gray, pattern, tmp8, st8, edges;
    Dev<uint16_t> depth;
    Dev<uint32_t> hsv;
    Dev<float> I[FE_LEVELS], ag[FE_LEVELS], dx0, dy0, map;
    Dev<float> ths, ths_s, pos, feat;
    Dev<int> sdiv, hdiv, cnt, mag, blk_cnt;
    Dev<short2> grad;
    Dev<FeCtrl> ctrl;
    // pinned host
    Pin<uint8_t> h_img;
    Pin<uint16_t> h_depth;
    Pin<FeCtrl> h_ctrl;
    Pin<float> h_pos, h_feat;
    cvo_fe_info info{};
    std::vector<FeGraph> graphs;   // one frame's device work, captured per (camera, features, ...)
    int copied = 0;            // points of the cloud already on their way to h_pos / h_feat
    bool pending = false;      // a frame was submitted and not collected yet
    bool device_output = false;   // collect_device() will be used: no copy of the cloud to the host
    int p_seq = 0, p_ftype = 0;
    // the caller's camera (cvo_fe_set_camera); without one the table row of dataset_seq
    cvo_fe_camera_model cam{};
    bool custom = false;
    bool rectify = false;      // ... and its dist is not all zero: frames start with k_fe_rectify
    uint64_t cam_gen = 0;      // counts the changes of camera: part of a captured graph's key
    // with the first distorting model: the upload targets of such frames and the map (qu, then qv)
    Dev<uint8_t> raw_img;
    Dev<uint16_t> raw_depth;
    Dev<int32_t> rect_map;     // 2 planes of rect_plane(np) entries
    // the caller's depth camera (cvo_fe_set_depth_camera); without one depth is registered to colour
    cvo_fe_depth_camera rig{};
    bool has_rig = false;      // frames start with k_fe_depth_warp / k_fe_depth_final
    int dw = 0, dh = 0;        // the size of the depth image a frame takes: the rig's, or the colour image's (iw x ih below)
    // with the first rig: the upload target of the depth image, the ray table and the z-buffer
    Dev<uint16_t> rig_depth;
    Dev<float2> rays;          // (dh + 1) * (dw + 1)
    Dev<uint32_t> zbuf;        // rect_plane(np) entries, FE_Z_EMPTY between frames
    // the caller's gate and mask (cvo_fe_set_depth_gate, cvo_fe_set_mask); with either, frames pass k_fe_depth_gate
    cvo_fe_depth_gate gate{};
    bool has_gate = false, has_mask = false;
    bool mask_dirty = false;       // h_mask holds bytes the device has not seen yet: the next submit() uploads them
    // with the first gate or mask: the plane the stages in front of the gate write, and the flags
    Dev<uint16_t> ungated;     // rect_plane(np) entries
    Dev<uint8_t> gate_flags;
    // with the first mask: its device plane and its pinned staging image
    Dev<uint8_t> d_mask;
    Pin<uint8_t> h_mask;
    // the caller's stereo settings (cvo_fe_set_stereo); with them a frame is a stereo pair and the matcher of
    // cvo_stereo.hip fills the depth plane
    cvo_fe_stereo stereo{};
    bool has_stereo = false;
    // the path mask (cvo_fe_set_stereo_paths): a setting of the context beside `stereo`, read by stereo frames only
    uint32_t stereo_paths = CVO_FE_PATHS_4;
    // the selector's mode (cvo_fe_set_select_mode): a setting of the context likewise, read by every frame
    int select_mode = CVO_FE_SELECT_IMAGE;
    // the speckle filter (cvo_fe_set_stereo_speckle): a setting of the context likewise; with it a stereo frame passes
    // the kernels of cvo_speckle.hip behind k_fe_stereo_final
    cvo_fe_speckle speckle{};
    bool has_speckle = false;
    // with the filter, and gone with it: parents, sums and sizes (np words each) and the count of removed pixels
    Dev<uint32_t> speckle_words;
    // the median stage (cvo_fe_set_depth_median): a setting of the context likewise, read by every frame; with it
    // whatever fills the depth plane fills `unfiltered`, and k_fe_median of cvo_median.hip writes that plane
    cvo_fe_depth_median median{};
    bool has_median = false;
    // with the filter, and gone with it: A of the median contract (rect_plane(np) entries) and the flags
    Dev<uint16_t> unfiltered;
    Dev<uint8_t> median_flags;
    // the infill stage (cvo_fe_set_depth_infill): a setting of the context likewise, read by every frame; with it
    // whatever fills the depth plane fills `sparse`, and k_fe_infill of cvo_infill.hip writes the plane they filled before
    cvo_fe_depth_infill infill{};
    bool has_infill = false;
    // with the stage, and gone with it: S of the infill contract (rect_plane(np) entries) and the flags
    Dev<uint16_t> sparse;
    Dev<uint8_t> infill_flags;
    // the caller's scan source (cvo_fe_set_lidar); with it a frame is a colour image and a scan, and the kernels of
    // cvo_lidar.hip with k_fe_depth_final between them fill the plane an uploaded depth image fills otherwise
    cvo_fe_lidar lidar{};
    bool has_lidar = false;
    // with a scan source, and gone with it: the scan's staging, pinned and on the device (a header of FE_LIDAR_HEADER
    // bytes whose first word is the frame's number of points, then max_points packed points), the z-buffer above, and,
    // with an occlusion test, P0 (rect_plane(np) entries) and the flags
    Pin<uint8_t> h_scan;
    Dev<uint8_t> d_scan;
    Dev<uint16_t> lidar_p0;
    Dev<uint8_t> lidar_flags;
    // the sweep of the scan source (cvo_fe_set_lidar_sweep), gone with it; the twist of the frames submitted from now
    // on (cvo_fe_set_lidar_motion), which lidar_stage puts into the scan's header; and the bytes of one staged record,
    // which h_scan and d_scan are sized for: 16 under a field mode, else 12
    cvo_fe_lidar_sweep sweep{};
    bool has_sweep = false;
    float lidar_twist[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    size_t scan_record = 12;
    // with the first settings: the right image and its pinned staging image, the planes of the matcher, and the
    // table U(q) with its staging copy; the cost sums follow max_disp
    Dev<uint8_t> right_img, right_gray, stereo_flags;
    Pin<uint8_t> h_right;
    Dev<uint64_t> census;      // 2 planes of np entries: left, right
    Dev<uint16_t> sgm_sum;     // np * stereo.max_disp
    Dev<uint32_t> stereo_win;
    Dev<uint16_t> disparity, depth_table;
    Pin<uint16_t> h_depth_table;
    float table_fx = 0.0f, table_scale = 0.0f;   // the camera the device's table was made for; 0: none yet
    // the caller's stereo rig (cvo_fe_set_stereo_rig); with it a frame is a RAW pair and starts with k_fe_stereo_rectify
    cvo_fe_stereo_rig srig{};
    bool has_srig = false;
    // with a rig, and gone with it: the upload targets of the raw pair, the four map planes (qu, qv of the left camera,
    // qu, qv of the right one; rect_plane(np) entries each) and the validity plane (rect_plane(np) bytes)
    Dev<uint8_t> srig_raw_l, srig_raw_r, srig_valid;
    Dev<int32_t> srig_map;
    // the pixel format of the caller's colour images (cvo_fe_set_pixel_format): a setting of the context, read by every
    // frame; under another than BGR8 the packed bytes are what is staged and uploaded, and k_fe_unpack of cvo_unpack.hip
    // writes where the upload lands otherwise
    int pixfmt = CVO_FE_PIXEL_BGR8;
    size_t pix_row = 0;        // row_bytes and rows of the packed image (cvo_fe_pixel_layout); 0 under BGR8
    int pix_rows = 0;
    // with such a format, and gone with it: the packed image and its pinned staging (they stand in for h_img); under
    // stereo the right image's as well (they stand in for h_right)
    Dev<uint8_t> packed, packed_r;
    Pin<uint8_t> h_packed, h_packed_r;
    // the format of the caller's depth images (cvo_fe_set_depth_format): a setting of the context, read by frames that
    // have a depth image; under a float format the float image is what is staged and uploaded, and k_fe_depth_convert of
    // cvo_depthfmt.hip writes where the uint16 upload lands otherwise
    int depthfmt = CVO_FE_DEPTH_U16;
    float depth_unit = 1.0f;
    // with a float format, and gone with it: the float image (dw * dh values) and its pinned staging (they stand in for
    // h_depth); both follow the depth camera's size
    Dev<uint8_t> fdepth;
    Pin<uint8_t> h_fdepth;
    // the frame being submitted takes its images from the caller's device memory (cvo_fe_submit_device): they are
    // brought to the landing buffers in front of the frame, and the frame's sequence holds no upload of them
    bool dev_in = false;
    // input binning (cvo_fe_set_input_binning): a setting of the context, read by every frame; with it the caller's
    // images are iw x ih = f * (w x h), the upload and the two kernels in front of the bin (k_fe_unpack,
    // k_fe_depth_convert) fill the input-size buffers below, and k_fe_bin of cvo_bin.hip writes where they land otherwise
    cvo_fe_binning bin{};
    bool has_bin = false;
    int iw = 0, ih = 0;        // the size of the colour image a frame takes: f * the context's, or the context's
    // with the setting, and gone with it: the input-size colour image, the right one's (a context that has had stereo
    // set) and the depth image
    Dev<uint8_t> full_img, full_right;
    Dev<uint16_t> full_depth;
    // the photometric stage (cvo_fe_set_photometric): a setting of the context, read by every frame; with it
    // k_fe_photo_apply of cvo_photo.hip corrects img_input / right_input in place behind the unpack and in front of the bin
    cvo_fe_photometric photo{};
    bool has_photo = false;
    // with the setting, and gone with it: the tables (the vignette dense at iw x ih), the header a frame's sequence
    // copies from its pinned twin, and under AUTO the state with the frame's record and the record's pinned landing
    Dev<uint16_t> photo_response, photo_vignette;
    Dev<FePhotoHeader> photo_hdr;
    Pin<FePhotoHeader> h_photo_hdr;
    Dev<FePhotoState> photo_state;
    Pin<cvo_fe_photometric_frame> h_photo_rec;
    uint32_t photo_gain[3] = {4096u, 4096u, 4096u};   // of the frames submitted from now on (cvo_fe_set_photometric_gain)
    bool photo_rearm = false;                          // the next frame opens the lock (cvo_fe_photometric_rearm)
    cvo_fe_photometric_frame photo_frame{};            // the last collected frame's record
    std::string err;
};

// (internal to the library: not among its exported symbols)
namespace cvo_fe __attribute__((visibility("hidden"))) {

inline int fail(cvo_fe_ctx *c, int code, const char *what, hipError_t e = hipSuccess)
{
    if (c) {
        c->err = what;
        if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
    }
    return code;
}

#define FE_HIP(call)                                                            \
    do {                                                                        \
        const hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return fail(ctx, CVO_HIP_ERR_HIP, #call, e_);     \
    } while (0)

template <class T> bool dev_alloc(Dev<T> &b, size_t n)
{
    T *p = nullptr;
    if (hipMalloc((void **)&p, n * sizeof(T)) != hipSuccess) return false;
    b.reset(p);
    return true;
}

template <class T> bool pin_alloc(Pin<T> &b, size_t n)
{
    T *p = nullptr;
    if (hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
    b.reset(p);
    return true;
}

// a setter whose allocation failed: the runtime's error is taken, so that the next frame does not find it
inline int no_memory(cvo_fe_ctx *ctx, const char *what)
{
    (void)hipGetLastError();
    return fail(ctx, CVO_HIP_ERR_NOMEM, what);
}

// The setters replace only when whole: they build what they need in locals, and after the last step that can
// fail the context takes what was built.  A local left empty (the context has that buffer already) changes nothing.
template <class B> void hand_over(B &to, B &built)
{
    if (built) to = std::move(built);
}

// the two planes of the device map lie this many entries apart: k_fe_rectify's 16-byte loads stay aligned
inline size_t rect_plane(int np) { return ((size_t)np + 3) & ~(size_t)3; }

inline bool lidar_stride_ok(size_t stride_bytes) { return stride_bytes >= 12 && stride_bytes % 4 == 0; }

inline bool sweep_field_mode(const cvo_fe_lidar_sweep &sw) { return sw.mode == CVO_FE_SWEEP_TIME_F32 || sw.mode == CVO_FE_SWEEP_TIME_U32; }

// the byte offset of the time word that lidar_stage carries along, -1: none
inline int sweep_time_offset(const cvo_fe_lidar_sweep *sw) { return sw && sweep_field_mode(*sw) ? sw->time_offset : -1; }

// `rows` rows of `row` bytes from an image of any stride into a dense one; in one call when the stride is dense
inline void copy_rows(void *dst, const void *src, size_t stride, size_t row, int rows)
{
    if (stride == row) {
        std::memcpy(dst, src, row * (size_t)rows);
        return;
    }
    for (int y = 0; y < rows; ++y) std::memcpy((uint8_t *)dst + (size_t)y * row, (const uint8_t *)src + (size_t)y * stride, row);
}

inline bool gate_active(const cvo_fe_ctx *ctx) { return ctx->has_gate || ctx->has_mask; }

// the depth plane the stages in front of level 0 write: the gate's input while it runs
inline uint16_t *depth_plane(const cvo_fe_ctx *ctx) { return gate_active(ctx) ? ctx->ungated.get() : ctx->depth.get(); }

// the plane in front of the median stage: its input while it runs, else the depth plane itself.  The infill stage
// writes it; without that stage the producers of depth do
inline uint16_t *filled_plane(const cvo_fe_ctx *ctx) { return ctx->has_median ? ctx->unfiltered.get() : depth_plane(ctx); }

// the plane the producers of depth write (an upload, k_fe_rectify, the depth camera's warp, the stereo matcher and its
// speckle filter, the LiDAR projection and its cull): the infill stage's input while it runs, else the plane above
inline uint16_t *source_plane(const cvo_fe_ctx *ctx) { return ctx->has_infill ? ctx->sparse.get() : filled_plane(ctx); }

// where the uploaded depth image lands: the raw buffer of a depth camera's size, else the raw depth that
// k_fe_rectify resamples, else the plane the producers write (a scan source: no image is uploaded, and the plane the
// projected scan fills stands in its place)
inline uint16_t *depth_upload(const cvo_fe_ctx *ctx)
{
    if (ctx->has_lidar) return source_plane(ctx);
    return ctx->has_rig ? ctx->rig_depth.get() : ctx->rectify ? ctx->raw_depth.get() : source_plane(ctx);
}

// the colour camera in force for a frame: a stereo rig's rectified pinhole, else the caller's model (a distorting
// one: its rectified pinhole), else the table row of dataset_seq (never fails: an index outside the table means row 0)
inline void camera_in_force(const cvo_fe_ctx *ctx, int dataset_seq, float cam[5])
{
    if (ctx->has_srig) {
        const cvo_fe_stereo_rig &r = ctx->srig;
        cam[0] = r.depth_scale; cam[1] = r.fx; cam[2] = r.fy; cam[3] = r.cx; cam[4] = r.cy;
    } else if (ctx->custom) {
        const cvo_fe_camera_model &m = ctx->cam;
        cam[0] = m.depth_scale; cam[1] = m.fx; cam[2] = m.fy; cam[3] = m.cx; cam[4] = m.cy;
    } else cvo_fe_camera(dataset_seq, cam);
}

inline bool unpacks(const cvo_fe_ctx *ctx) { return ctx->pixfmt != CVO_FE_PIXEL_BGR8; }

// the staging a frame's colour image is copied to and uploaded from, its row and its rows: the packed image under a
// pixel format; and the right image's under stereo
inline uint8_t *img_staging(const cvo_fe_ctx *ctx) { return unpacks(ctx) ? ctx->h_packed.get() : ctx->h_img.get(); }
inline uint8_t *right_staging(const cvo_fe_ctx *ctx) { return unpacks(ctx) ? ctx->h_packed_r.get() : ctx->h_right.get(); }
// (under input binning the image is iw x ih, and the packed layout is that size's)
inline size_t img_row(const cvo_fe_ctx *ctx) { return unpacks(ctx) ? ctx->pix_row : (size_t)ctx->iw * 3; }
inline int img_rows(const cvo_fe_ctx *ctx) { return unpacks(ctx) ? ctx->pix_rows : ctx->ih; }

// where the colour image lands on the device (an upload, or k_fe_unpack's output): the stereo rig's raw buffer, else the
// raw image k_fe_rectify resamples, else the image every later stage reads; and the right image of a stereo frame
inline uint8_t *img_landing(const cvo_fe_ctx *ctx)
{
    return ctx->has_srig ? ctx->srig_raw_l.get() : ctx->rectify ? ctx->raw_img.get() : ctx->img.get();
}
inline uint8_t *right_landing(const cvo_fe_ctx *ctx) { return ctx->has_srig ? ctx->srig_raw_r.get() : ctx->right_img.get(); }

// Input binning: the bin's inputs.  A depth image is binned where the frame has one of the context's own size: not
// under a depth camera (its image keeps the rig's size), stereo or a scan source (no depth image).  The buffer an
// upload, a device frame's copy, k_fe_unpack or k_fe_depth_convert fills: the input-size one under binning, else the
// landing buffer itself
inline bool bins_depth(const cvo_fe_ctx *ctx) { return ctx->has_bin && !ctx->has_rig && !ctx->has_stereo && !ctx->has_lidar; }
inline uint8_t *img_input(const cvo_fe_ctx *ctx) { return ctx->has_bin ? ctx->full_img.get() : img_landing(ctx); }
inline uint8_t *right_input(const cvo_fe_ctx *ctx) { return ctx->has_bin ? ctx->full_right.get() : right_landing(ctx); }
inline uint16_t *depth_input(const cvo_fe_ctx *ctx) { return bins_depth(ctx) ? ctx->full_depth.get() : depth_upload(ctx); }

// under a float depth format: the bytes of one value, and the staging a frame's depth image is copied to and uploaded from
inline bool converts(const cvo_fe_ctx *ctx) { return ctx->depthfmt != CVO_FE_DEPTH_U16; }
inline size_t depth_item(const cvo_fe_ctx *ctx) { return fe_depth_item(ctx->depthfmt); }
inline void *depth_staging(const cvo_fe_ctx *ctx) { return converts(ctx) ? (void *)ctx->h_fdepth.get() : (void *)ctx->h_depth.get(); }

// After a change of what a frame's sequence is -- and the only place that destroys a graph.  A graph captured
// before the change holds the old numbers, the old buffers (the map's address too) and the old first node.
// Dropping those graphs here is what keeps them from being launched again -- and what keeps the cache of 8
// from filling with dead entries; the generation in the key is the guard behind it, should a graph ever
// outlive such a change.
inline void drop_graphs(cvo_fe_ctx *ctx)
{
    ctx->cam_gen++;
    for (auto &g : ctx->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    ctx->graphs.clear();
}

}   // namespace cvo_fe

#endif
