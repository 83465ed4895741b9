/* cvo_frontend.h -- C-ABI of the MI355X RGB-D front end: one RGB
 * image + one depth image in, the semi-dense coloured point cloud the
 * registration consumes out.  Part of libcvo_hip.so; status codes are
 * cvo_hip_status (cvo_hip.h).
 *
 * Replaces, behind plain pointers and sizes, what the reference does inside
 * set_pcd() with cv::Mat arguments:
 *   cvo::pcd_generator::load_image          ref cpp/rkhs_registration/src/pcd_generator.cpp:387-398
 *   cvo::pcd_generator::create_pointcloud   ref src/pcd_generator.cpp:400-420
 *     make_pyramid :33-129, select_point :131-176 (dso::PixelSelector::makeMaps,
 *     ref thirdparty/PixelSelector2.cpp:137-236, and the Canny top-up),
 *     get_points_from_pixels :233-327, get_features :329-385
 * as called from cvo::set_pcd (ref src/cvo.cpp:318-341, feature type 1) and
 * acvo::set_pcd (ref src/adaptive_cvo.cpp:440-463, feature type 0).
 *
 * The selector is held to the reference's own code: thirdparty/PixelSelector2.cpp,
 * compiled as it lies, gives the thresholds, the map, the count, the potential and the
 * re-selection of this library bit for bit, for budgets from 1 to 10^6
 * (tests/test_gpu_selector_ref.py).  One read of the reference is undefined and is
 * defined here: a pixel whose threshold cell (x>>5) + (y>>5)*(w/32) lies past the
 * (w/32)*(h/32) cells that exist (any w % 32 > 5 or h % 32 > 3, 1280x720 among them)
 * takes the last cell's threshold; the reference reads memory it never wrote.
 *
 * Every stage runs as HIP kernels on the context's stream.  The images come from
 * host memory (cvo_fe_submit) or lie in device memory already (cvo_fe_submit_device),
 * and the cloud goes to host memory (cvo_fe_collect) or stays in device memory
 * (cvo_fe_collect_device): a frame can go from a device image to a pose without
 * touching host memory.  There is no CPU path: without a gfx950
 * device cvo_fe_create() fails with CVO_HIP_ERR_NODEVICE.
 *
 * Beyond the reference: a caller's own camera (cvo_fe_set_camera) in place of the
 * six-row table, with the lens distortion removed on the device as the first
 * stage of a frame.  The reference treats every camera as an ideal pinhole; its
 * own run script's sequence (TUM fr1) is not one.  The rectification contract is
 * stated at cvo_fe_camera_model below.  And a depth camera of its own
 * (cvo_fe_set_depth_camera): another size, pinhole and lens, mounted beside the
 * colour camera; every frame then registers the depth image into the colour
 * camera's frame on the device.  The registration contract is stated at
 * cvo_fe_depth_camera below.  And a gate on the depth values themselves
 * (cvo_fe_set_depth_gate, cvo_fe_set_mask): pixels out of range, on or beside a depth
 * discontinuity, or under a caller's mask lose their depth before any later stage reads it.
 * The gate contract is stated at cvo_fe_depth_gate below.  And a rectified stereo pair in place
 * of the depth image (cvo_fe_set_stereo, cvo_fe_submit_stereo): a semi-global matcher on the device
 * fills the depth plane.  The stereo contract is stated at cvo_fe_stereo below.  And the rig behind such a pair
 * (cvo_fe_set_stereo_rig): two cameras with lenses of their own that are not parallel; every frame then takes
 * the RAW pair and rectifies both images on the device in front of the matcher.  The rig contract is stated at
 * cvo_fe_stereo_rig below; cvo_fe_stereo_rectify makes a rig from what a calibration tool gives.  And a speckle
 * filter on the matcher's disparities (cvo_fe_set_stereo_speckle; cvo_fe_filter_speckles for any uint16 plane):
 * small connected components lose their disparity.  The speckle contract is stated at cvo_fe_speckle below.  And a
 * mode of the selector in which a pixel without depth does not compete (cvo_fe_set_select_mode), so that the cloud
 * holds the num_want the caller asked for whatever the stages above removed.  The selection contract is stated at
 * cvo_fe_set_select_mode below; a new context selects by the image alone, as the reference does.  And a median
 * filter on the depth plane itself, in front of the gate, for every kind of frame (cvo_fe_set_depth_median;
 * cvo_fe_median_plane for any uint16 plane): a lone outlier takes its neighbourhood's value and, if asked for, a small
 * hole is filled.  The median contract is stated at cvo_fe_depth_median below.  And a LiDAR scan in place of the depth
 * image (cvo_fe_set_lidar, cvo_fe_submit_lidar; cvo_fe_project_points for any scan without a context): the points are
 * projected into the colour camera on the device, nearest surface wins, and what the scanner sees between the points of
 * a nearer object is culled.  The LiDAR contract is stated at cvo_fe_lidar below.  And a stage that bridges the gaps of a
 * sparse depth plane -- between scan lines, in the holes a forward warp leaves, where the stereo tests drop pixels of a
 * smooth surface -- linearly in inverse depth, for every kind of frame (cvo_fe_set_depth_infill; cvo_fe_infill_plane for
 * any uint16 plane).  The infill contract is stated at cvo_fe_depth_infill below.  And motion compensation of a spinning
 * LiDAR scan (cvo_fe_set_lidar_sweep, cvo_fe_set_lidar_motion; cvo_fe_project_points_sweep without a context): every
 * point is moved into the scanner's frame at the instant of the colour image, by its own time or azimuth and the
 * scanner's motion over the sweep, in the pass that projects it.  The sweep contract is stated at cvo_fe_lidar_sweep below.
 * And a format for the depth image (cvo_fe_set_depth_format; cvo_fe_convert_depth for any plane): float32 or float16 in a
 * unit the caller names, converted on the device in front of everything that reads it.  The depth-format contract is stated
 * at CVO_FE_DEPTH_* below.  And frames whose images lie in device memory already (cvo_fe_submit_device,
 * cvo_fe_submit_stereo_device).  The device-input contract is stated at cvo_fe_submit_device below.  And frames in the
 * sensor's own resolution (cvo_fe_set_input_binning; cvo_fe_bin_image and cvo_fe_bin_depth for any image): the caller's
 * images are f times the context's size each way, and the first kernel of the frame bins them down to the working size.
 * The binning contract is stated at cvo_fe_binning below.  And the sensor's photometry (cvo_fe_set_photometric;
 * cvo_fe_photometric_image for any image): a response table, a vignette and a per-frame gain per channel, the caller's
 * or estimated on the device, correct the colour bytes in place in front of the bin.  The photometric contract is
 * stated at cvo_fe_photometric below.
 */
#ifndef CVO_FRONTEND_H
#define CVO_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#include "cvo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cvo_fe_ctx cvo_fe_ctx;

/* feature_type of create_pointcloud (ref include/pcd_generator.hpp:96-99) */
enum { CVO_FE_FEATURES_HSV = 0,   /* H/180 S/255 V/255 dx/255*2 dy/255*2 (acvo) */
       CVO_FE_FEATURES_RGB = 1 }; /* raw channel bytes + raw gradients (cvo) */

/* intermediate images, for parity checks (cvo_fe_read_stage) */
enum { CVO_FE_STAGE_GRAY = 0,     /* w*h uint8 */
       CVO_FE_STAGE_HSV = 1,      /* w*h*3 uint8 */
       CVO_FE_STAGE_MAP = 2,      /* w*h float: 0 / 1 / 2 / 4 as the selector writes them */
       CVO_FE_STAGE_AG0 = 3,      /* squared gradient magnitude, level 0: w*h float */
       CVO_FE_STAGE_AG1 = 4,      /* level 1: (w/2)*(h/2) float */
       CVO_FE_STAGE_AG2 = 5,      /* level 2: (w/4)*(h/4) float */
       CVO_FE_STAGE_THS = 6,      /* smoothed cell thresholds: (w/32)*(h/32) float */
       CVO_FE_STAGE_DX0 = 7, CVO_FE_STAGE_DY0 = 8,   /* level-0 gradients: w*h float */
       CVO_FE_STAGE_EDGES = 9,    /* Canny edges of the last top-up: w*h uint8 (0 / 255) */
       CVO_FE_STAGE_RECT_BGR = 10,    /* the colour image every later stage read: w*h*3 uint8 */
       CVO_FE_STAGE_RECT_DEPTH = 11,  /* ... and the depth image: w*h uint16.  Without a distorting
                                         camera model these two are the input images.  With a depth
                                         camera this one is the registered depth (colour size). */
       CVO_FE_STAGE_RAW_DEPTH = 12,   /* the depth image as uploaded: the depth camera's width*height
                                         uint16, or w*h without a depth camera */
       CVO_FE_STAGE_UNGATED_DEPTH = 13,   /* the depth plane the gate read: w*h uint16.  Without a gate
                                             or mask it equals RECT_DEPTH (which, with one, is the gated
                                             plane: still "the depth image every later stage read") */
       CVO_FE_STAGE_GATE = 14,        /* the gate's flags: w*h uint8, an OR of CVO_FE_GATE_*; all zero
                                         without a gate or mask */
       /* of a stereo frame (cvo_fe_set_stereo; CVO_HIP_ERR_INVALID on a context without stereo).  Under
          stereo RAW_DEPTH and UNGATED_DEPTH are the plane that stereo wrote, RECT_DEPTH that plane after
          the gate, if a gate or mask is set. */
       CVO_FE_STAGE_RIGHT_GRAY = 15,  /* w*h uint8 */
       CVO_FE_STAGE_CENSUS_L = 16, CVO_FE_STAGE_CENSUS_R = 17,   /* w*h uint64 each */
       CVO_FE_STAGE_SGM_SUM = 18,     /* S: w*h*max_disp uint16, index (y*w + x)*max_disp + d */
       CVO_FE_STAGE_DISPARITY = 19,   /* w*h uint16: q in 1/16 pixel, 0 = none */
       CVO_FE_STAGE_STEREO = 20,      /* w*h uint8: an OR of CVO_FE_STEREO_* */
       CVO_FE_STAGE_RIGHT_BGR = 21,   /* the right colour image the matcher read: w*h*3 uint8.  Without a stereo rig
                                         the image as uploaded, with one the rectified one */
       CVO_FE_STAGE_STEREO_VALID = 22,    /* of a frame under a stereo rig (CVO_HIP_ERR_INVALID without one): w*h
                                             uint8, bit 0 = V_L, bit 1 = V_R of the rig contract */
       CVO_FE_STAGE_SPECKLE_SIZE = 23,    /* of a stereo frame under a speckle filter (CVO_HIP_ERR_INVALID without
                                             one): w*h uint32, SIZE of the speckle contract */
       /* of a frame under a median filter (cvo_fe_set_depth_median; CVO_HIP_ERR_INVALID on a context without one).
          With the filter UNGATED_DEPTH, "the plane the gate read", is B of the median contract. */
       CVO_FE_STAGE_UNFILTERED_DEPTH = 24,    /* A of the median contract: w*h uint16 */
       CVO_FE_STAGE_MEDIAN = 25,          /* MEDIAN of the median contract: w*h uint8, CVO_FE_MEDIAN_* */
       /* of a frame under a scan source (cvo_fe_set_lidar; CVO_HIP_ERR_INVALID on a context without one).  With it
          RAW_DEPTH is P of the LiDAR contract. */
       CVO_FE_STAGE_LIDAR_DEPTH = 26,     /* P0 of the LiDAR contract, the plane before culling: w*h uint16 */
       CVO_FE_STAGE_LIDAR = 27,           /* w*h uint8, CVO_FE_LIDAR_* */
       /* of a frame under the infill stage (cvo_fe_set_depth_infill; CVO_HIP_ERR_INVALID on a context without it).
          With it UNFILTERED_DEPTH (under a median filter), else UNGATED_DEPTH, is F of the infill contract. */
       CVO_FE_STAGE_SPARSE_DEPTH = 28,    /* S of the infill contract: w*h uint16 */
       CVO_FE_STAGE_INFILL = 29,          /* INFILL of the infill contract: w*h uint8, CVO_FE_INFILL_* */
       /* of a frame under a pixel format (cvo_fe_set_pixel_format; CVO_HIP_ERR_INVALID on a context in
          CVO_FE_PIXEL_BGR8, and the second on one without stereo as well).  With the photometric stage set
          (cvo_fe_set_photometric) both read what that stage wrote, on a BGR8 context too; under binning
          CVO_FE_STAGE_FULL_BGR / _FULL_RIGHT_BGR below do. */
       CVO_FE_STAGE_INPUT_BGR = 30,       /* the unpacked colour or left image, in front of any rectification: w*h*3 uint8 */
       CVO_FE_STAGE_INPUT_RIGHT_BGR = 31,     /* the unpacked right image: w*h*3 uint8 */
       /* of a frame under input binning (the binning contract at cvo_fe_binning; CVO_HIP_ERR_INVALID without it).  Under
        * binning the two ids above and CVO_FE_STAGE_RAW_DEPTH are what the bin wrote, with or without a pixel format;
        * every id above names a plane of the working size. */
       CVO_FE_STAGE_FULL_BGR = 32,        /* the colour or left image the bin read: fw*fh*3 uint8 */
       CVO_FE_STAGE_FULL_RIGHT_BGR = 33,  /* the right image the bin read: fw*fh*3 uint8; INVALID without stereo */
       CVO_FE_STAGE_FULL_DEPTH = 34 };    /* the depth plane the bin read: fw*fh uint16; INVALID under a depth camera,
                                           * stereo or a scan source */

/* flags of CVO_FE_STAGE_GATE (the gate contract at cvo_fe_depth_gate) */
enum { CVO_FE_GATE_MASKED = 1, CVO_FE_GATE_RANGE = 2, CVO_FE_GATE_JUMP = 4 };
/* flags of CVO_FE_STAGE_STEREO (the stereo contract at cvo_fe_stereo) */
enum { CVO_FE_STEREO_UNIQUE = 1, CVO_FE_STEREO_LR = 2, CVO_FE_STEREO_MIN = 4, CVO_FE_STEREO_DEPTH = 8,
       CVO_FE_STEREO_OUTSIDE = 16,     /* (only under a stereo rig: the rig contract at cvo_fe_stereo_rig) */
       CVO_FE_STEREO_SPECKLE = 32 };   /* (only under a speckle filter: the speckle contract at cvo_fe_speckle) */
/* values of CVO_FE_STAGE_MEDIAN (the median contract at cvo_fe_depth_median) */
enum { CVO_FE_MEDIAN_CHANGED = 1, CVO_FE_MEDIAN_FILLED = 2 };
/* bits of CVO_FE_STAGE_LIDAR (the LiDAR contract at cvo_fe_lidar): HIT where P0 != 0; OCCLUDED beside it where the
   occlusion test dropped the pixel */
enum { CVO_FE_LIDAR_HIT = 1, CVO_FE_LIDAR_OCCLUDED = 2 };
/* values of CVO_FE_STAGE_INFILL (the infill contract at cvo_fe_depth_infill) */
enum { CVO_FE_INFILL_ROW = 1, CVO_FE_INFILL_COL = 2, CVO_FE_INFILL_JUMP = 4 };

/* The pixel format of the colour images a caller hands over (cvo_fe_set_pixel_format), and the unpack contract.
 *
 * Layout.  A packed image of a w x h picture is `rows` rows of `row_bytes` bytes (cvo_fe_pixel_layout):
 *   BGR8, RGB8: 3w.  BGRA8, RGBA8: 4w.  YUY2, UYVY: 2w.  GREY8, NV12 and the four Bayer formats: w.
 *   rows is h, except NV12: h + h/2 (h rows of Y, then h/2 rows of U V pairs).
 * A caller's image has one stride for every row, NV12's chroma rows included, of at least row_bytes.
 * Sizes.  YUY2 and UYVY need an even w, NV12 an even w and an even h, Bayer w >= 2 and h >= 2.
 *
 * The unpacked image is w*h*3 bytes, B G R per pixel, defined by this arithmetic and not by the device -- this
 * library's own definition, not pinned against another library's conversions:
 *   RGB8, BGRA8, RGBA8, GREY8: byte moves; alpha is dropped; GREY8: B = G = R = the byte.
 *   YUY2 (Y0 U Y1 V), UYVY (U Y0 V Y1), NV12: pixels 2k and 2k+1 of a row share the U and V of their pair; NV12 pixel
 *     (x, y) takes the pair at column x >> 1 of chroma row y >> 1; no chroma is interpolated.  BT.601, limited range,
 *     in int32 with an arithmetic shift, Y NOT clamped before the multiply:
 *         c = Y - 16;  d = U - 128;  e = V - 128;
 *         R = sat8((1220945*c + 1673555*e             + 524288) >> 20);
 *         G = sat8((1220945*c -  410793*d - 852458*e  + 524288) >> 20);
 *         B = sat8((1220945*c + 2115221*d             + 524288) >> 20);
 *     The constants are 2^20 times 255/219, 1.402*255/224, 1.772*(0.114/0.587)*255/224, 1.402*(0.299/0.587)*255/224
 *     and 1.772*255/224, rounded to nearest; over all 2^24 triples the largest accumulator is 560 963 210 in
 *     magnitude.  (16, 128, 128) gives 0 0 0, (235, 128, 128) gives 255 255 255, and B = G = R along the grey axis.
 *   Bayer, bilinear.  The four letters of a format are the colours of pixels (0,0) (1,0) / (0,1) (1,1) -- NOT OpenCV's
 *     names.  A pixel keeps the value of its own colour.  Green at a red or blue site is (N + S + E + W + 2) >> 2; the
 *     opposite colour there is the four diagonals, (... + 2) >> 2.  At a green site the colour of its row is
 *     (E + W + 1) >> 1 and the other is (N + S + 1) >> 1.  A neighbour outside the image is MIRRORED about the border
 *     pixel (-1 -> 1, w -> w - 2), which keeps the mosaic's phase.  The mosaic of a flat colour comes back exactly;
 *     that of an integer ramp comes back exactly in the interior, not on the border.
 *
 * Where it sits.  Under a format other than BGR8 one kernel runs in front of everything else in the frame; its output
 * lands where the uploaded image lands otherwise (CVO_FE_STAGE_INPUT_BGR, CVO_FE_STAGE_INPUT_RIGHT_BGR), and no
 * later stage changes: the frame is that of a context in BGR8 fed the unpacked image.  The mask's grid ("the colour
 * image as uploaded") is the same pixel grid. */
enum { CVO_FE_PIXEL_BGR8 = 0,      /* a new context's: the layout cv::imread decodes to */
       CVO_FE_PIXEL_RGB8 = 1, CVO_FE_PIXEL_BGRA8 = 2, CVO_FE_PIXEL_RGBA8 = 3, CVO_FE_PIXEL_GREY8 = 4,
       CVO_FE_PIXEL_YUY2 = 5,      /* Y0 U Y1 V */
       CVO_FE_PIXEL_UYVY = 6,      /* U Y0 V Y1 */
       CVO_FE_PIXEL_NV12 = 7,      /* h rows of Y, then h/2 rows of U V pairs */
       CVO_FE_PIXEL_BAYER_RGGB8 = 8, CVO_FE_PIXEL_BAYER_BGGR8 = 9,
       CVO_FE_PIXEL_BAYER_GRBG8 = 10, CVO_FE_PIXEL_BAYER_GBRG8 = 11 };

/* The format of the depth images a caller hands over (cvo_fe_set_depth_format), and the depth-format contract: depth
 * that comes out of a network or a simulator is a float32 or float16 plane in metres (or another unit), not uint16.
 *
 * THE DEPTH-FORMAT CONTRACT.  Under CVO_FE_DEPTH_F32 or CVO_FE_DEPTH_F16 the depth image of a frame is w x h values of
 * 4 or 2 bytes (the depth camera's size while one is set), and one kernel turns it into the uint16 image that
 * CVO_FE_DEPTH_U16 takes as it is.  The results are defined by the arithmetic below, not by the device; it is this
 * library's own definition.
 * `unit` is metres per input unit: 1 for metres, 0.001 for float millimetres.  `scale` is the depth_scale of whatever
 * reads the uploaded depth image first: the depth camera's (rig.depth_scale) while one is set, otherwise the colour
 * camera's in force for the frame (the cvo_fe_set_camera model, else the table row of dataset_seq).
 * For every input value, in float32, every operation rounded on its own, in this order and no other:
 *     v = the value (a float16 is widened exactly)
 *     no depth (0) unless v is finite and v >= 2^-126     (drops NaN, both infinities, +-0, negatives, subnormals)
 *     t = v * unit;          no depth unless t >= 2^-126
 *     q = rintf(t * scale)   (ties to even)
 *     out = (1 <= q && q <= 65535) ? (uint16)q : 0        (too near and too far are no depth, never clamped)
 * The two subnormal rules make the result independent of whether the device flushes denormals.  The order of the two
 * multiplications is observable and part of the contract: at unit 0.001 and scale 5000 the value 2947.099853515625
 * gives 14736, and v * (unit * scale) would give 14735.  At scale 5000 and unit 1, 0.8 gives 4000 and 0.7998 gives
 * 3999; at scale 1024, 62.5/1024 gives 62, 63.5/1024 gives 64, 0.5/1024 gives 0, 1.5/1024 gives 2, 65534.5/1024 gives
 * 65534 and 65535.5/1024 gives 0.
 *
 * Where it sits.  Under a float format one kernel runs in front of everything else that reads the depth image
 * (rectification, the depth camera's warp, infill, median, gate); it writes where the uint16 upload lands otherwise, and
 * no later stage changes: the frame is that of a context in CVO_FE_DEPTH_U16 fed the converted plane, and
 * CVO_FE_STAGE_RAW_DEPTH is the converted plane.  Stereo and LiDAR frames have no depth image and do not read the
 * format; it may be set beside them and is kept. */
enum { CVO_FE_DEPTH_U16 = 0,       /* a new context's: uint16 in the camera's own depth units */
       CVO_FE_DEPTH_F32 = 1,       /* float32 in `unit` metres */
       CVO_FE_DEPTH_F16 = 2 };     /* float16 (IEEE binary16) in `unit` metres */

typedef struct cvo_fe_info {
    int32_t num_selected;   /* pixels the selector kept (before the depth test), ref pcd_generator.cpp:141; under
                               CVO_FE_SELECT_DEPTH they all have a depth (the selection contract) */
    int32_t pot_used;       /* potential of the selection pass that produced the map */
    int32_t reselected;     /* 1: the first pass missed the density band and a second one ran */
    int32_t canny_used;     /* 1: fewer than num_want/3 were kept, edges were added */
    int32_t num_points;     /* points in the cloud (selected and depth != 0) */
    int32_t pad_;
} cvo_fe_info;

/* A caller's camera: the five numbers of cvo_fe_camera() with the same meaning, and the
 * lens distortion of the Brown-Conrady model in OpenCV's / TUM's order d0..d4.
 *
 * THE RECTIFICATION CONTRACT.  A model whose `dist` is not all zero makes every frame of
 * the context start with a rectification of both images; grey, HSV, pyramid, selector,
 * Canny top-up and back-projection then run on the rectified pair, unchanged.  The
 * results are defined by the arithmetic below, not by the device.  It is this library's
 * own definition -- the constant-camera-matrix convention of cv::undistort (the rectified
 * image keeps fx fy cx cy; no new camera matrix, no cropping) and a fixed-point bilinear
 * tap in the style of cv::remap (5 fractional bits) -- and it is NOT pinned against
 * cv::remap: bytes may differ from OpenCV's in the last place.
 *
 * The map, once per (model, image size), in float64 on the model's floats widened
 * exactly, no operation contracted into an FMA, in this order, for output pixel (u, v):
 *     x = (u - cx) / fx;  y = (v - cy) / fy;  r2 = x*x + y*y;
 *     rad = 1 + r2*(k1 + r2*(k2 + r2*k3));
 *     xd = x*rad + ((2*p1)*x*y + p2*(r2 + (2*x)*x));
 *     yd = y*rad + (p1*(r2 + (2*y)*y) + (2*p2)*x*y);
 *     us = fx*xd + cx;  vs = fy*yd + cy;
 *   us is clamped to [-1, w], vs to [-1, h] (a value that is not a number counts as -1);
 *   qu = rint(32*us), qv = rint(32*vs), ties to even, as int32.
 * Colour, per channel, in integers: x0 = floor(qu/32), ax = qu - 32*x0, likewise y0, ay;
 *   the four taps (x0, x0+1) x (y0, y0+1), each coordinate clamped to the image
 *   (replicated border: no black frame, no gradients made of it);
 *   out = (sum of wx*wy*p + 512) >> 10, wx in {32 - ax, ax}, wy in {32 - ay, ay}.
 * Depth is registered to the colour image and shares its map; it is never interpolated:
 *   xn = floor((qu + 16)/32), yn likewise; out = source(xn, yn), or 0 (no point) when
 *   (xn, yn) lies outside the image.  A zero stays a zero. */
typedef struct cvo_fe_camera_model {
    float depth_scale, fx, fy, cx, cy;   /* as cvo_fe_camera(): depth units per metre, focal lengths, centre */
    float dist[5];                       /* k1 k2 p1 p2 k3; all 0: ideal pinhole, no rectification pass */
} cvo_fe_camera_model;

/* A depth camera of its own: the depth image has its own size, pinhole and lens and is taken
 * from another place than the colour image (7-Scenes, raw NYUv2, ScanNet, Azure Kinect and
 * RealSense recordings).  Without one the library assumes what the reference assumes: depth
 * pixel (u, v) is colour pixel (u, v).
 *
 * THE REGISTRATION CONTRACT.  While a depth camera is set every frame of the context starts
 * with a forward warp of the depth image into the frame of the colour camera in force for that
 * frame -- the cvo_fe_set_camera model if one is set (its rectified pinhole if it distorts),
 * otherwise the table row of dataset_seq -- and every later stage reads the registered image,
 * unchanged.  k_fe_rectify then resamples colour only: the raw depth reaches the rectified
 * frame in one resampling, not two.  The results are defined by the arithmetic below, not by
 * the device.  It is this library's own definition -- the footprint idea of the common SDKs'
 * depth-to-colour alignment, nearest surface wins -- and it is NOT pinned against any of them.
 *
 * The ray table, once per rig, on the host in float64 on the rig's floats widened exactly, no
 * operation contracted, in this order; for the corner (i, j), i = 0..width, j = 0..height, at
 * image position (i - 0.5, j - 0.5):
 *     xd = ((i - 0.5) - cx) / fx;  yd = ((j - 0.5) - cy) / fy;  x = xd;  y = yd;
 *     if dist is not all zero, 20 times:
 *         r2 = x*x + y*y;  rad = 1 + r2*(k1 + r2*(k2 + r2*k3));
 *         dx = (2*p1)*x*y + p2*(r2 + (2*x)*x);  dy = p1*(r2 + (2*y)*y) + (2*p2)*x*y;
 *         x = (xd - dx) / rad;  y = (yd - dy) / rad;
 *       then (x, y) is distorted forward with the formulae of the rectification contract to
 *       (us, vs); unless |us - (i - 0.5)| <= 1/32 and |vs - (j - 0.5)| <= 1/32 (a value that is
 *       not a number fails) the ray is invalid: x = y = NaN.  (A lens the fixed point cannot
 *       invert gives such pixels no depth rather than a wrong one.)
 *     xn[j][i] = (float)x;  yn[j][i] = (float)y.
 * Per depth pixel (u, v) with d = depth[v][u], every frame, in float32, every operation
 * explicit in this order, division correctly rounded, no FMA; c marks the colour camera, w x h
 * its image:
 *     skip if d == 0;  z = (float)d / depth_scale;
 *     skip if (min_range > 0 and z < min_range) or (max_range > 0 and z > max_range);
 *     for the corners a = (u, v) and b = (u+1, v+1) of the table:
 *         X = xn*z;  Y = yn*z;  Q.k = ((R[k][0]*X + R[k][1]*Y) + R[k][2]*z) + T[k],  k = 0, 1, 2;
 *     skip unless Qa.z > 0 and Qb.z > 0 (an invalid ray fails this);
 *     ua = fxc*(Qa.x/Qa.z) + cxc;  va = fyc*(Qa.y/Qa.z) + cyc;  ub, vb likewise;
 *     skip if any of the four is not finite;
 *     q = rintf((0.5f*(Qa.z + Qb.z)) * depth_scale_c);  skip unless 1 <= q <= 65535;
 *     x0 = (int)ceilf(clamp(fminf(ua, ub), -1, w + 1));  x1 = (int)ceilf(clamp(fmaxf(ua, ub), -1, w + 1));
 *     x1 = min(x1, x0 + 8);  y0, y1 likewise with h;
 *     for every colour pixel (x, y), max(x0, 0) <= x < min(x1, w), max(y0, 0) <= y < min(y1, h):
 *         Z[y][x] = min(Z[y][x], q).
 * The registered pixel is Z where something was written and 0 (no point) otherwise.  The
 * footprint is the set of pixel centres inside the projected cell, half-open, capped at 8 x 8 so
 * that a pixel's work is bounded; a rig that is the colour camera itself (same size and pinhole,
 * R = I, T = 0) returns the depth image byte for byte; the result does not depend on the order
 * of the writes.  Holes a forward warp leaves are not filled here; the infill stage (the infill contract at
 * cvo_fe_depth_infill) bridges them by inverse depth and the median stage (the median contract at
 * cvo_fe_depth_median) fills the small ones with a neighbour's depth, each if it is asked to. */
typedef struct cvo_fe_depth_camera {
    int32_t width, height;               /* of the DEPTH image; may differ from the context's (colour) size */
    float depth_scale, fx, fy, cx, cy;   /* units per metre of the depth image's values; the depth camera's pinhole */
    float dist[5];                       /* k1 k2 p1 p2 k3 of the depth camera's lens; all 0: none */
    float R[9], T[3];                    /* p_colour = R p_depth + T, R row-major, T in metres */
    float min_range, max_range;          /* metres along the depth camera's axis; <= 0: no limit on that side */
} cvo_fe_depth_camera;

/* A gate on the depth values: which pixels with a depth keep it.
 *
 * THE GATE CONTRACT.  While a gate or a mask (cvo_fe_set_mask) is set every frame of the context
 * passes its depth plane -- as it stands after the rectification or the registration above, w x h
 * uint16, called U here -- through one more stage before anything else reads it; level 0, the
 * selector, the Canny top-up and the back-projection then run unchanged on the gated plane.  The
 * results are defined by the arithmetic below, not by the device.  It is this library's own
 * definition and is NOT pinned against any SDK's filter.  (Under a median filter U is that stage's
 * output, B of the median contract at cvo_fe_depth_median; under the infill stage without a median
 * filter it is F of the infill contract at cvo_fe_depth_infill.)
 *
 * `scale` is depth_scale of the colour camera in force for the frame (the cvo_fe_set_camera model,
 * else the table row of dataset_seq).  For a pixel p with U(p) != 0:
 *   range (CVO_FE_GATE_RANGE): z = (float)U(p) / scale in float32, correctly rounded; flagged if
 *     (min_range > 0 && z < min_range) || (max_range > 0 && z > max_range) -- the rule and the
 *     arithmetic of the rig's min_range / max_range.  (At scale 5000 and min_range 0.8f a pixel of
 *     4000 is kept and one of 3999 is dropped.)
 *   jump mark J(p): for each of the eight neighbours q inside the image,
 *     U(q) != 0: m = min(U(p), U(q)), D = max(U(p), U(q)) - m; q marks p iff jump_rel > 0 and
 *       (float)D > jump_rel * (float)m  (float32: one multiplication, one comparison; both integers
 *       are exact in float32 and nothing can be contracted);
 *     U(q) == 0: q marks p iff hole_border.
 *     Neighbours outside the image never mark; J(p) = 0 where U(p) == 0.  Both sides of a step are
 *     marked: that is intended.  The threshold is relative because that bounds the slope of a
 *     surface against its ray whatever the range: two neighbouring rays 1/f apart see a depth step
 *     of z tan(theta) / f on a surface inclined by theta, so D/m > jump_rel means
 *     tan(theta) > about f * jump_rel at 1 m as at 4 m; an absolute threshold would not.
 *   near a jump (CVO_FE_GATE_JUMP): flagged if some q inside the image with
 *     max(|dx|, |dy|) <= grow has J(q) = 1.  Marks are computed on U: range and mask do not
 *     change them.
 *   masked (CVO_FE_GATE_MASKED): the mask is height rows of width bytes on the grid of the colour
 *     image as uploaded, non-zero = drop.  Without a distorting model: flagged if mask[p] != 0.
 *     With one the mask goes through the rectification map by the depth rule of the rectification
 *     contract: (xn, yn) = (floor((qu+16)/32), floor((qv+16)/32)); masked if that lies outside the
 *     image, else if mask[yn][xn] != 0.
 * GATE(p) is the OR of the flags, and 0 where U(p) == 0; RECT_DEPTH(p) = GATE(p) ? 0 : U(p).
 * Selection is untouched: a gated pixel is a selected pixel without depth, so num_selected does
 * not move and num_points drops. */
typedef struct cvo_fe_depth_gate {
    float   min_range, max_range;  /* metres along the colour camera's axis; <= 0: no limit on that side */
    float   jump_rel;              /* relative depth jump that marks a discontinuity; 0: no jump test */
    int32_t grow;                  /* 0..3: pixels around a marked pixel that go with it (Chebyshev) */
    int32_t hole_border;           /* 1: a valid pixel beside a pixel without depth is marked too */
    int32_t pad_;                  /* must be 0 */
} cvo_fe_depth_gate;               /* 24 bytes, no padding */

/* A rectified stereo pair in place of a depth image: rows 4 and 5 of cvo_fe_camera() ("kitti 15",
 * "kitti 05") are the left colour camera of a stereo rig with no depth sensor behind it.
 *
 * THE STEREO CONTRACT.  While stereo is set a frame is a left and a right colour image of the
 * context's size (cvo_fe_submit_stereo); the left one is the colour image of every later stage, and a
 * semi-global matcher (census cost, four to eight paths) fills the depth plane that an uploaded depth image
 * fills otherwise -- the input of the gate, if one is set, and of level 0.  The pair must be rectified:
 * a match for left pixel (x, y) is looked for at right pixel (x - d, y) only.  The results are defined by
 * the integer arithmetic below, not by the device.  It is this library's own definition, NOT pinned
 * against OpenCV's or libSGM's.  D is max_disp; p is a pixel (x, y) of the w x h image.
 *   1. Grey.  Both images by the formula of STAGE_GRAY: (c0*4899 + c1*9617 + c2*1868 + 8192) >> 14.
 *   2. Census.  A window 9 wide and 7 high: dy = -3..3 outer, dx = -4..4 inner, the centre skipped, the
 *      neighbour's coordinates clamped to the image; each comparison appends one bit at the low end,
 *      c = (c << 1) | (grey(n) < grey(centre)): 62 bits in a uint64.
 *   3. Cost.  C(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)) for x - d >= 0, and 64 otherwise.
 *   4. Paths.  Eight directions r = (rx, ry), numbered as the bits of a path mask (cvo_fe_set_stereo_paths;
 *      CVO_FE_PATHS_4 = 0x0F, bits 0 to 3, unless the caller chooses another):
 *          bit 0 (+1, 0) left to right      bit 4 (+1, +1) towards lower right
 *          bit 1 (-1, 0) right to left      bit 5 (-1, -1) towards upper left
 *          bit 2 (0, +1) top to bottom      bit 6 (-1, +1) towards lower left
 *          bit 3 (0, -1) bottom to top      bit 7 (+1, -1) towards upper right
 *      A pixel p whose p - r = (x - rx, y - ry) lies outside the image is the first pixel of its path and has
 *      L_r = C; for a diagonal that happens on two borders (x = 0 or y = 0 for bit 4).  After that
 *          L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + p1, L_r(p-r, d+1) + p1, m + p2) - m,
 *          m = min over k of L_r(p-r, k);
 *      terms whose d-1 or d+1 lies outside [0, D) are left out.  S = sum of L_r over the directions whose bit is
 *      set; with n bits set and p2 <= 255 it is at most n * (64 + 255) <= 8 * 319 = 2552, so uint16 holds it, and
 *      being integer it does not depend on the order in which the paths are added.  Under a mask of one bit S is
 *      that direction's L_r.
 *   5. Winner.  d* = argmin over d of S(p, d), the smallest d on ties; S1 = S(p, d*).
 *   6. Uniqueness.  S2 = min of S(p, d) over |d - d*| > 1.  UNIQUE iff such a d exists and
 *      S2 * (100 - uniqueness) < S1 * 100.
 *   7. Left-right.  dR(x, y) = argmin over d with x + d < w of S(x + d, y, d), the smallest d on ties.
 *      LR iff lr_max >= 0 and (x - d* < 0 or |dR(x - d*, y) - d*| > lr_max).
 *   8. Sub-pixel.  Sm = S(p, d* - 1), Sp = S(p, d* + 1).  If 0 < d* < D - 1 and den = Sm + Sp - 2*S1 > 0:
 *      off = floor(((Sm - Sp)*16 + den) / (2*den)) -- floor division of signed integers; off lies in
 *      [-8, 8] -- otherwise off = 0.  q = 16*d* + off.  MIN iff q < 16*min_disp.
 *   9. Depth.  fx and depth_scale are those of the colour camera in force (the cvo_fe_set_camera model,
 *      else the table row of dataset_seq).  A table, once per frame's camera, on the host in float64 on
 *      the floats widened exactly: U(q) = rint((((fx*baseline)*depth_scale)*16) / q), ties to even;
 *      U(q) = 0 for q < 16*min_disp and where the result lies outside [1, 65535].  The device only looks
 *      U(q) up.  DEPTH iff the pixel has no other flag and U(q) == 0.
 *  10. Output.  STEREO(p) is the OR of the flags; DISPARITY(p) = STEREO(p) ? 0 : q; the depth plane gets
 *      STEREO(p) ? 0 : U(q).
 * Diagonal paths are part of it where the path mask names them; hole filling and a median filter are not: they are
 * the infill stage (the infill contract at cvo_fe_depth_infill, linear in inverse depth and so in disparity) and the
 * median stage (the median contract at cvo_fe_depth_median) behind the matcher; what the
 * diagonals are worth in accuracy on real pairs is not measured.  A pair that is not rectified goes in
 * with its rig (cvo_fe_set_stereo_rig, the rig contract below). */
typedef struct cvo_fe_stereo {
    float   baseline;      /* metres between the two cameras; > 0 */
    int32_t max_disp;      /* D: disparities 0 .. D-1 are searched; a multiple of 8 in [8, 128] */
    int32_t min_disp;      /* >= 1: a pixel whose disparity is below it gets no depth */
    int32_t p1, p2;        /* SGM penalties, 1 <= p1 <= p2 <= 255 */
    int32_t uniqueness;    /* 0..99, per cent; 0: no uniqueness test */
    int32_t lr_max;        /* 0..8: largest |dL - dR| kept; -1: no left-right test */
    int32_t pad_;          /* must be 0 */
} cvo_fe_stereo;           /* 32 bytes */

/* A speckle filter on the disparities of a stereo frame: small islands of confident but wrong disparity -- on
 * repetitive texture, sky, occlusion borders and glass they pass the uniqueness and the left-right test -- lose
 * their disparity before they become points that float off every surface.
 *
 * THE SPECKLE CONTRACT.  It is defined by the arithmetic below, not by the device.  It follows the rule of
 * cv::filterSpeckles as its documentation states it, and it is NOT pinned against OpenCV.
 * Let Q be the DISPARITY plane as step 10 of the stereo contract leaves it; under a rig that is with OUTSIDE applied.
 *   Valid pixels: those with Q != 0.
 *   Joined: two valid pixels are joined iff they are 4-neighbours (left, right, up, down; no diagonals) and
 *     |Q(p) - Q(n)| <= max_diff, the difference of signed integers (1 beside 65535 differ by 65534).
 *   Components: the classes of the transitive closure of "joined".  A chain of small steps is one component, however
 *     far its ends are apart.
 *   SIZE(p) is the pixel count of p's component, and 0 where Q(p) == 0 (CVO_FE_STAGE_SPECKLE_SIZE).
 *   SPECKLE is set at p iff Q(p) != 0 and SIZE(p) <= max_size.  Such a pixel has STEREO |= CVO_FE_STEREO_SPECKLE,
 *     DISPARITY = 0 and depth plane 0.  Every other byte of the frame's planes is what it is without the filter.
 * The gate, if one is set, and level 0 read the filtered plane.  The result does not depend on the order in which
 * the device meets the pixels: sizes are integer counts.  Not part of it: hole filling and a median filter, which are
 * the infill stage (the infill contract at cvo_fe_depth_infill) and the median stage (the median contract at
 * cvo_fe_depth_median) behind this one. */
typedef struct cvo_fe_speckle {
    int32_t max_size;   /* components of at most this many pixels lose their disparity; 1 .. 2^26 */
    int32_t max_diff;   /* largest |Q(p) - Q(n)| that joins two neighbours, in units of the plane (1/16 pixel for
                           DISPARITY); 0 .. 65535 */
} cvo_fe_speckle;       /* 8 bytes */

/* A median filter on the depth plane, filling small holes: a single outlier of a sensor or of the matcher, at the
 * strong gradients the selector picks, becomes a point floating off its surface, and a one-pixel hole there loses the
 * pixel that was picked.
 *
 * THE MEDIAN CONTRACT.  While a filter is set every frame of the context, of every kind, passes its depth plane through
 * one more stage directly in front of the gate.  The results are defined by the integer arithmetic below, not by the
 * device.  It is this library's own definition and is NOT pinned against cv::medianBlur or any SDK's filter.
 * Let A be the depth plane as it stands after the rectification, the depth camera's registration, the stereo
 * matcher and its speckle filter, or the LiDAR projection and its cull -- and, where the infill stage is set, after that
 * stage: A is then F of the infill contract at cvo_fe_depth_infill.  It is w x h uint16 with 0 = none -- what the gate
 * contract calls U without this stage.
 * For a pixel p:
 *   W(p) is the set of pixels q inside the image with max(|dx|, |dy|) <= radius.  Pixels outside the image are not in
 *     it: no replicated border.
 *   V(p) is the multiset of A(q) over q in W(p) with A(q) != 0; n = |V(p)|; v_0 <= ... <= v_(n-1) its members in
 *     ascending order.
 *   med(p) = v_((n-1) >> 1): the lower median, always a value some pixel of the window holds, never an average.
 *   B(p) = med(p) if A(p) != 0 (then n >= 1: p counts itself); otherwise med(p) if fill_min > 0 and n >= fill_min;
 *     otherwise 0.
 *   MEDIAN(p) = CVO_FE_MEDIAN_CHANGED where A(p) != 0 and B(p) != A(p); CVO_FE_MEDIAN_FILLED where A(p) == 0 and
 *     B(p) != 0; 0 elsewhere (CVO_FE_STAGE_MEDIAN).
 * Every pixel's result is a function of A alone: it does not depend on the order in which the device meets the pixels,
 * and it is not computed in place.  65535 is a depth like any other.
 * B is the plane the gate reads (the U of the gate contract, CVO_FE_STAGE_UNGATED_DEPTH); without a gate or mask
 * level 0, the selector under CVO_FE_SELECT_DEPTH and the back-projection read it, all unchanged.  Range, jump marks and
 * mask therefore act on B; a caller who wants a region kept free of filled depth masks it.  A is
 * CVO_FE_STAGE_UNFILTERED_DEPTH; CVO_FE_STAGE_RAW_DEPTH keeps its meaning.
 * Under stereo CVO_FE_STAGE_DISPARITY and CVO_FE_STAGE_STEREO stay the matcher's: the stage works on depths only.  A
 * filled pixel has a depth and DISPARITY 0; a changed pixel has its neighbour's depth and its own disparity.  The table
 * U(q) of the stereo contract is monotone (a larger disparity is a smaller depth), so the lower median of the depths is
 * the upper median of the disparities. */
typedef struct cvo_fe_depth_median {
    int32_t radius;     /* 1: 3 x 3, 2: 5 x 5 */
    int32_t fill_min;   /* 0: a pixel without depth stays without; k >= 1: it takes the window's median when at
                           least k pixels of its window have a depth; at most (2*radius+1)^2 - 1 */
    int32_t pad_;       /* must be 0 */
} cvo_fe_depth_median;  /* 12 bytes */

/* A LiDAR scan in place of the depth image: a camera beside a Velodyne, an Ouster or a Livox (KITTI's rig ships a scan
 * per frame and Tr_velo_to_cam in every sequence's calib.txt).  A scan projected into the image is one small launch and
 * is as accurate at 60 m as at 6 m, where a stereo pair's depth error grows with the square of the range.  The plane it
 * leaves has many holes; everything behind it is built for such a plane: CVO_FE_SELECT_DEPTH keeps the cloud at
 * num_want, the median stage with fill_min closes the gaps between scan lines, the gate drops range and jumps.
 *
 * THE LIDAR CONTRACT.  While a scan source is set a frame of the context is one colour image and n points,
 * 0 <= n <= max_points.  The results are defined by the arithmetic below, not by the device.  It is this library's own
 * definition and is NOT pinned against any SDK.
 * The points are the first three floats (x y z) of records stride_bytes apart; stride_bytes is at least 12 and a
 * multiple of 4 (KITTI's .bin: 16; the reflectance is not read).
 * The colour camera in force, c, is the cvo_fe_set_camera model if one is set, otherwise the table row of dataset_seq.
 * If that model distorts, the colour image alone goes through the rectification, as under a depth camera, and c is its
 * rectified pinhole (fxc, fyc, cxc, cyc, depth_scale_c).  The colour image is w x h.
 * Per point, all arithmetic in float32, every operation explicit in this order, division correctly rounded, nothing
 * fused.  "skip" ends the point:
 *   1. Skip unless x, y and z are all finite.
 *   2. Q.k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + T[k], k = 0, 1, 2.
 *   3. Skip unless Q.z > 0.
 *   4. Skip if (min_range > 0 && Q.z < min_range) || (max_range > 0 && Q.z > max_range).
 *   5. u = fxc*(Q.x/Q.z) + cxc;  v = fyc*(Q.y/Q.z) + cyc.
 *   6. Skip unless u and v are both finite.
 *   7. q = rintf(Q.z * depth_scale_c).  Skip unless 1 <= q <= 65535.
 *   8. xi = (int)rintf(clamp(u, -8, w + 8)), ties to even; yi likewise with h.
 *   9. For every pixel (x, y) inside the image with |x - xi| <= splat and |y - yi| <= splat: Z[y][x] = min(Z[y][x], q).
 * The plane before culling, P0, is Z where something was written and 0 elsewhere (CVO_FE_STAGE_LIDAR_DEPTH).  Nearest
 * surface wins; the result does not depend on the order of the points.
 * Occlusion.  The scanner is not at the camera: between the points of a near object it sees background that the camera
 * does not.  For a pixel p with P0(p) != 0:
 *   m(p) is the minimum of P0(q) over q inside the image with |dx| <= occl_rx, |dy| <= occl_ry and P0(q) != 0; p counts
 *     itself.  65535 is a depth like any other.
 *   OCCLUDED(p) holds iff occl_rel > 0 and (float)(P0(p) - m) > occl_rel * (float)m: one float32 multiplication and one
 *     comparison, the shape of the gate's jump test.  At occl_rel 0.25 beside a 4000, a 5000 is kept and a 5001 dropped.
 *   P(p) = OCCLUDED(p) ? 0 : P0(p).  P is a function of P0 alone and is not computed in place.
 * The window has two half-widths because a threshold relative to depth also fires across rows on a ground plane near
 * the horizon: a caller whose scanner sits above the camera wants the window wide and flat (occl_ry 0 or 1).
 * CVO_FE_STAGE_LIDAR holds CVO_FE_LIDAR_HIT where P0 != 0, and CVO_FE_LIDAR_OCCLUDED beside it where OCCLUDED.
 * P is the plane an uploaded depth image fills otherwise: the input of the median stage, the gate and level 0, all
 * unchanged.  It is CVO_FE_STAGE_RAW_DEPTH; without median or gate it is also UNGATED_DEPTH and RECT_DEPTH.
 * Motion compensation of a spinning scan is the sweep contract at cvo_fe_lidar_sweep below: off unless it is set.
 * Not part of it: a lens in the
 * projection (the colour image is rectified instead); reflectance as a feature; densifying beyond splat, which is the
 * infill stage behind this one (the infill contract at cvo_fe_depth_infill: between two scan lines on one surface the
 * depth is interpolated, not copied) and the median stage's fill. */

/* Bridging the gaps of a sparse depth plane.  A LiDAR scan's lines land some pixels apart in the image; on a ground
 * plane near the horizon two neighbouring lines differ by decimetres to metres of depth, and a pixel between them that
 * copies one line's depth (splat, the median stage's fill) becomes a point that floats above or below the road by
 * that much.  In a pinhole image a plane's INVERSE depth is linear in the pixel coordinates, so interpolating the inverse
 * depth between the two lines is exact on planes up to rounding; it is also what interpolating a stereo pair's
 * disparity linearly gives.  What the stage is worth in trajectory accuracy on real scans is not measured.
 *
 * THE INFILL CONTRACT.  While the stage is set every frame of the context, of every kind, passes its depth plane through
 * one more stage directly behind whatever fills it and directly in front of the median stage.  The results are defined
 * by the integer arithmetic below, not by the device.  It is this library's own definition and is NOT pinned against
 * any SDK's hole filling.
 * Let S be the depth plane as it stands after the upload or the rectification, the depth camera's registration, the
 * stereo matcher and its speckle filter, or the LiDAR projection and its cull: w x h uint16 with 0 = none
 * (CVO_FE_STAGE_SPARSE_DEPTH).  The stage's output F is A of the median contract if a median filter is set
 * (CVO_FE_STAGE_UNFILTERED_DEPTH), otherwise U of the gate contract (CVO_FE_STAGE_UNGATED_DEPTH), otherwise the depth
 * plane.  CVO_FE_STAGE_RAW_DEPTH keeps its meaning.
 * One pass along an axis has an input plane X and a limit g.  For a maximal run of L >= 1 consecutive pixels with X = 0
 * along the axis:
 *   The run is bounded iff the pixel in front of it and the pixel behind it both lie inside the image; both then have
 *     a depth, A and B.  A pixel outside the image is never an end: no replicated border.
 *   A bounded run with L <= g is a candidate.
 *   With lo = min(A, B) and hi = max(A, B) a candidate is refused iff
 *     jump_rel > 0 && (float)(hi - lo) > jump_rel * (float)lo
 *     -- one float32 multiplication and one comparison, the shape of the gate's jump test and of the LiDAR cull.  At
 *     jump_rel 0.25 a 5000 beside a 4000 is bridged and a 5001 is not.
 *   A candidate that is not refused is bridged.  Its pixel da >= 1 pixels from the A end and db >= 1 from the B end
 *     (da + db = L + 1) takes
 *       N = A * B * (da + db);  Dn = A * da + B * db;  value = floor((2 * N + Dn) / (2 * Dn))
 *     in exact integers (N reaches 65535^2 * 32: 64 bits).  That is 1 / ((db/A + da/B) / (da + db)), the interpolation
 *     of the inverse depths, rounded half up; it lies in [lo, hi] and is at least 1.
 *   Every other pixel of the pass keeps X.  Every pixel of a pass is a function of the pass's input alone: a pass is not
 *   computed in place.  A pass with g = 0 is the identity.
 * The row pass turns S into H with g = gap_x; the column pass then turns H -- not S -- into F with g = gap_y: a column
 * may be bridged from a pixel the row pass made.
 * INFILL(p) (CVO_FE_STAGE_INFILL) is CVO_FE_INFILL_ROW where the row pass filled p, CVO_FE_INFILL_COL where the column
 * pass did, CVO_FE_INFILL_JUMP where F(p) = 0 and at least one pass refused p's run, and 0 elsewhere.  A pixel with
 * S != 0 is never changed: F = S there.  65535 is a depth like any other.
 * Under stereo CVO_FE_STAGE_DISPARITY and CVO_FE_STAGE_STEREO stay the matcher's: a filled pixel has a depth and
 * DISPARITY 0. */
typedef struct cvo_fe_depth_infill {
    int32_t gap_x;     /* 0..15: the longest run of pixels without depth in a ROW that is bridged; 0: no row pass */
    int32_t gap_y;     /* 0..31: likewise in a COLUMN; 0: no column pass */
    float   jump_rel;  /* 0: no test; > 0: ends that differ by more than this relative step are not bridged */
    int32_t pad_;      /* must be 0 */
} cvo_fe_depth_infill; /* 16 bytes */
typedef struct cvo_fe_lidar {
    int32_t max_points;          /* capacity of a scan, 1 .. 2^21; the staging a frame copies has this size */
    int32_t splat;               /* 0..3: a point writes the (2*splat+1)^2 pixels around its nearest pixel */
    float   R[9], T[3];          /* p_colour = R p_lidar + T, R row-major, T in metres (KITTI: R_rect_00 *
                                    Tr_velo_to_cam, the caller multiplies) */
    float   min_range, max_range;/* metres along the colour camera's axis; <= 0: no limit on that side */
    float   occl_rel;            /* 0: no occlusion test; > 0: see above */
    int32_t occl_rx, occl_ry;    /* 0..7 each: half-widths of the occlusion window */
    int32_t pad_;                /* must be 0 */
} cvo_fe_lidar;                  /* 80 bytes, no padding */

/* Motion compensation of a spinning scan.  A spinning scanner collects a scan over a whole sweep -- 100 ms at 10 Hz --
 * while the colour image is exposed at one instant: at 10 m/s the first and the last point are measured from places a
 * metre apart, and in a turn of 30 degrees/s a point 40 m out lands 2 m beside its surface.  With a sweep set every
 * point is moved into the scanner's frame at the instant of the image before it is projected, by the scanner's motion
 * over the sweep, which the caller hands over per frame (cvo_fe_set_lidar_motion; cvo_fe_lidar_twist makes it from the
 * last registration).  What it is worth in trajectory accuracy on real scans is not measured: none are shipped.
 *
 * THE SWEEP CONTRACT.  While a sweep is set (cvo_fe_set_lidar_sweep) every point of a frame's scan that has passed
 * step 1 of the LiDAR contract goes through the two steps below, and steps 2 to 9 and the cull run on p' in place of
 * (x, y, z), unchanged.  All arithmetic in float32, every operation explicit in the stated order, division correctly
 * rounded, nothing fused, no library transcendental.  It is this library's own definition.
 * Phase s of the point, the fraction of the sweep at which it was measured:
 *   CVO_FE_SWEEP_TIME_F32: t is the float at byte time_offset of the record.  Skip the point unless t is finite.
 *     s = (t - time_origin) * time_scale;  s = fminf(fmaxf(s, 0), 1).
 *   CVO_FE_SWEEP_TIME_U32: t is the uint32 at byte time_offset.  s = (float)t * time_scale (the conversion rounds to
 *     nearest even);  s = fminf(fmaxf(s, 0), 1).
 *   CVO_FE_SWEEP_AZIMUTH (records without a time, KITTI's): a turn fraction q of (x, y), with ax = |x|, ay = |y|:
 *     r = min(ax, ay) / max(ax, ay), and r = 0 if max(ax, ay) is 0;  r2 = r*r;
 *     q = (((((C5*r2 + C4)*r2 + C3)*r2 + C2)*r2 + C1)*r2 + C0) * r   with Ck = CVO_FE_SWEEP_ATAN_Ck below: atan(r)/2pi
 *       within 3e-7 turn on [0, 1];
 *     then, in this order:  if ay > ax: q = 0.25 - q;   if x < 0: q = 0.5 - q;   if y < 0: q = -q.
 *     The tie ax == ay belongs to the octant of the x axis (no first fix-up: q = the polynomial at r = 1); -0 is not < 0.
 *     s = (float)direction * q + phase0;  s = s - floorf(s).  s lies in [0, 1]; 1 itself is reached where s was just
 *     below a whole number.
 *     The seam of this mode is ambiguous by nature: a point on the azimuth where the sweep begins and ends may have been
 *     measured at either end, and is moved as the end its phase names.
 * Move, with the frame's twist (w_twist, v_twist) (cvo_fe_set_lidar_motion):
 *   a = s - s_ref;   w.k = a * w_twist.k;   tau.k = a * v_twist.k   (k = 0, 1, 2);
 *   t2 = (w.0*w.0 + w.1*w.1) + w.2*w.2;
 *   A = ((((A5*t2 + A4)*t2 + A3)*t2 + A2)*t2 + A1)*t2 + A0      sin(t)/t,         Ak = (-1)^k / (2k+1)!
 *   B = ((((B5*t2 + B4)*t2 + B3)*t2 + B2)*t2 + B1)*t2 + B0      (1 - cos t)/t^2,  Bk = (-1)^k / (2k+2)!
 *   C =  (((C4*t2 + C3)*t2 + C2)*t2 + C1)*t2 + C0               (t - sin t)/t^3,  Ck = (-1)^k / (2k+3)!
 *     with the coefficients CVO_FE_SWEEP_A0 .. below, each the float32 nearest to its fraction.  t2 <= 1 by the cap on
 *     the twist; the first term left out is below 2^-26 in every series (B carries one term more than that asks for).
 *   cross(a, b) = (a.1*b.2 - a.2*b.1,  a.2*b.0 - a.0*b.2,  a.0*b.1 - a.1*b.0);
 *   c1 = cross(w, p);  c2 = cross(w, c1);  d1 = cross(w, tau);  d2 = cross(w, d1)      with p = (x, y, z);
 *   p'.k = ((p.k + A*c1.k) + B*c2.k) + ((tau.k + B*d1.k) + C*d2.k).
 * Meaning: p' is the point in the scanner's frame at phase s_ref, for a scanner whose pose over the sweep is
 * T0 * Exp(s * xi), xi = (w_twist, v_twist): p' = Exp((s - s_ref) * xi) p.
 * Identities: with a zero twist, or where s == s_ref, p' = p up to the sign of a zero, and with a zero twist the planes
 * are those of a context without a sweep, byte for byte.
 * p' may overflow for a point beyond 1e37; steps 3, 6 and 7 then skip it. */
enum { CVO_FE_SWEEP_TIME_F32 = 1, CVO_FE_SWEEP_TIME_U32 = 2, CVO_FE_SWEEP_AZIMUTH = 3 };
typedef struct cvo_fe_lidar_sweep {
    int32_t mode;         /* one of the above */
    int32_t time_offset;  /* byte offset of the time word in a record (modes 1, 2): a multiple of 4, >= 12; not read
                             under mode 3 */
    float   time_origin;  /* mode 1: subtracted first; must be 0 otherwise */
    float   time_scale;   /* modes 1, 2: phase per unit of the field (1 / sweep duration); finite, != 0; not read
                             under mode 3 */
    float   phase0;       /* mode 3: phase of azimuth 0, in [0, 1); finite and not read otherwise */
    int32_t direction;    /* mode 3: +1 phase grows with atan2(y, x), -1 it falls; must be 0 otherwise */
    float   s_ref;        /* phase at which the colour image is exposed, in [0, 1] */
    int32_t pad_;         /* must be 0 */
} cvo_fe_lidar_sweep;     /* 32 bytes, no padding */
/* The coefficients of the sweep contract.  ATAN: an odd polynomial of degree 11 for atan(r) / (2 pi) on [0, 1], a
 * least-squares fit at 400 Chebyshev nodes; its largest error in float32 is 3.0e-7 turn, which at the caps on the twist
 * moves a point 120 m out by less than 0.06 mm. */
#define CVO_FE_SWEEP_ATAN_C0 1.591517329e-01f
#define CVO_FE_SWEEP_ATAN_C1 -5.294376612e-02f
#define CVO_FE_SWEEP_ATAN_C2 3.082358837e-02f
#define CVO_FE_SWEEP_ATAN_C3 -1.856560260e-02f
#define CVO_FE_SWEEP_ATAN_C4 8.407119662e-03f
#define CVO_FE_SWEEP_ATAN_C5 -1.873333240e-03f
#define CVO_FE_SWEEP_A0 1.0f
#define CVO_FE_SWEEP_A1 (-1.0f / 6.0f)
#define CVO_FE_SWEEP_A2 (1.0f / 120.0f)
#define CVO_FE_SWEEP_A3 (-1.0f / 5040.0f)
#define CVO_FE_SWEEP_A4 (1.0f / 362880.0f)
#define CVO_FE_SWEEP_A5 (-1.0f / 39916800.0f)
#define CVO_FE_SWEEP_B0 (1.0f / 2.0f)
#define CVO_FE_SWEEP_B1 (-1.0f / 24.0f)
#define CVO_FE_SWEEP_B2 (1.0f / 720.0f)
#define CVO_FE_SWEEP_B3 (-1.0f / 40320.0f)
#define CVO_FE_SWEEP_B4 (1.0f / 3628800.0f)
#define CVO_FE_SWEEP_B5 (-1.0f / 479001600.0f)
#define CVO_FE_SWEEP_C0 (1.0f / 6.0f)
#define CVO_FE_SWEEP_C1 (-1.0f / 120.0f)
#define CVO_FE_SWEEP_C2 (1.0f / 5040.0f)
#define CVO_FE_SWEEP_C3 (-1.0f / 362880.0f)
#define CVO_FE_SWEEP_C4 (1.0f / 39916800.0f)
/* the caps on a frame's twist: |w| in radians per sweep (573 degrees/s at 10 Hz), |v| in metres per sweep */
#define CVO_FE_SWEEP_MAX_ROTATION 1.0f
#define CVO_FE_SWEEP_MAX_TRANSLATION 64.0f

/* One camera of a stereo rig: its pinhole and its lens (k1 k2 p1 p2 k3, as cvo_fe_camera_model's dist). */
typedef struct cvo_fe_lens {
    float fx, fy, cx, cy;
    float dist[5];
} cvo_fe_lens;                 /* 36 bytes, no padding */

/* What a stereo calibration tool gives: the two cameras and where the right one sits. */
typedef struct cvo_fe_stereo_calib {
    cvo_fe_lens left, right;
    float R[9], T[3];          /* p_right = R p_left + T, R row-major, T in metres */
} cvo_fe_stereo_calib;         /* 120 bytes, no padding */

/* A raw stereo pair, rectified on the device by its rig: two cameras with lenses of their own whose axes are not
 * parallel (KITTI raw, EuRoC, a ZED or RealSense IR pair, any rig bolted together).  A caller with published
 * rectification data fills the struct directly (KITTI raw: R_left / R_right = R_rect_0x, fx fy cx cy from
 * P_rect_0x, baseline = -P_rect(0,3) / fx of the right camera); everybody else gets it from
 * cvo_fe_stereo_rectify.
 *
 * THE RIG CONTRACT.  While a rig is set cvo_fe_submit_stereo / cvo_fe_create_pointcloud_stereo take the RAW pair,
 * and every frame starts with the resampling of both images through the rig's two maps; the rectified left image
 * is the colour image of every later stage (CVO_FE_STAGE_RECT_BGR), the matcher of the stereo contract reads the
 * rectified pair (CVO_FE_STAGE_RIGHT_BGR is the right one), and its steps 1 to 10 are unchanged.  The results
 * are defined by the arithmetic below, not by the device.
 *
 * The helper cvo_fe_stereo_rectify(calib, width, height, out, depth_scale), host only, float64 on the floats
 * widened exactly.  It is this library's own definition, in the manner of Bouguet's method, and is NOT pinned
 * against cv::stereoRectify.  In this order:
 *   1. om = the axis-angle of R: c = (((R00 + R11) + R22) - 1) / 2, v = (R21 - R12, R02 - R20, R10 - R01),
 *      n = |v|, angle = atan2(n / 2, c), axis k = v / n (angle 0 and no axis if n == 0).  Refused: an angle
 *      above 0.5 rad.
 *   2. Rl0 = exp(om / 2), Rr0 = exp(-om / 2) by Rodrigues' formula I + sin(a) K + (1 - cos(a)) K K with
 *      a = +-angle / 2 and K the cross-product matrix of k: R = Rr0^T Rl0, each camera turns half the way.
 *   3. t = Rr0 T, b = |t|, e1 = -t / b: the direction from the left centre to the right one.  Refused unless
 *      b > 0, e1.x > 0, e1.x >= |e1.y| and e1.x >= |e1.z|: the rig must be horizontal, the right camera on
 *      the right.
 *   4. e2 = normalise((0, 0, 1) x e1), e3 = e1 x e2; W has the rows e1, e2, e3; R_left = W Rl0,
 *      R_right = W Rr0.
 *   5. f = (left.fy + right.fy) / 2; fx = fy = f.
 *   6. a_k = R_k (0, 0, 1), the third column of R_k: camera k's optical axis lands at
 *      (f a_k.x / a_k.z, f a_k.y / a_k.z); m = the mean of the two landing points;
 *      cx = (width - 1) / 2 - m.x, cy = (height - 1) / 2 - m.y.  Both cameras get ONE cx: a point at infinity
 *      has disparity 0.
 *   7. baseline = b; every member is rounded to float32; the two cameras are copied through.
 *
 * The maps, one per camera, once per (rig, image size), on the host in float64 on the rig's floats widened
 * exactly, no operation contracted, in this order, for output pixel (u, v) of camera k (R_k = R_left or
 * R_right, R_k[i][j] = R_k[3*i + j]):
 *     xr = (u - cx) / fx;  yr = (v - cy) / fy;                       (the rectified pinhole)
 *     X = (R_k[0][0]*xr + R_k[1][0]*yr) + R_k[2][0];                 (R_k^T applied to (xr, yr, 1):
 *     Y = (R_k[0][1]*xr + R_k[1][1]*yr) + R_k[2][1];                  p_rect = R_k p_k)
 *     Z = (R_k[0][2]*xr + R_k[1][2]*yr) + R_k[2][2];
 *     unless Z > 0: us = vs = -1;  else x = X / Z, y = Y / Z and (us, vs) is (x, y) distorted forward and
 *     projected with camera k's own fx fy cx cy and dist by the formulae of the rectification contract (rad, xd,
 *     yd, us, vs at cvo_fe_camera_model);
 *   then that contract's clamp to [-1, w] x [-1, h] (a value that is not a number counts as -1) and
 *   qu = rint(32*us), qv = rint(32*vs), ties to even.  cvo_fe_stereo_rig_map returns the map.
 * Colour of both images: the integer bilinear tap of the rectification contract (5 fractional bits, replicated
 * border, + 512 >> 10).
 * Validity: V_k(p) = 1 iff the nearest sample (floor((qu + 16) / 32), floor((qv + 16) / 32)) of camera k's map
 * at p lies inside the raw image -- the depth rule of the rectification contract.  CVO_FE_STAGE_STEREO_VALID
 * holds V_L in bit 0 and V_R in bit 1.
 * One more flag, CVO_FE_STEREO_OUTSIDE: set at p = (x, y) iff !V_L(x, y), or x - d* >= 0 && !V_R(x - d*, y),
 * d* the winner of step 5.  The flags of steps 6 to 9 are computed exactly as without a rig (OUTSIDE is not
 * "another flag" for DEPTH) and OUTSIDE is ORed in afterwards; a pixel with any flag gets no disparity and no
 * depth, as in step 10.
 * The camera in force for the frame is (depth_scale, fx, fy, cx, cy) of the rig: back-projection, the gate's
 * `scale` and the depth table; dataset_seq is ignored.  The table of step 9 is made from the rig's fx, baseline
 * and depth_scale; cvo_fe_stereo.baseline is not read while a rig is set.
 * A mask (cvo_fe_set_mask) lies on the grid of the raw LEFT image and goes through the left map by the gate
 * contract's rule for a distorting model.
 * Not part of it: hole filling, keeping the smeared border (the replicated taps outside the raw images) out of
 * the path costs -- OUTSIDE drops such pixels, their costs still reach their neighbours -- and vertical rigs. */
typedef struct cvo_fe_stereo_rig {
    cvo_fe_lens left, right;             /* the two cameras as they are */
    float R_left[9], R_right[9];         /* the rectifying rotations, row-major: p_rect = R_k p_k */
    float fx, fy, cx, cy;                /* the rectified pinhole, common to both */
    float baseline;                      /* metres between the rectified cameras; > 0 */
    float depth_scale;                   /* units per metre of the depth plane; > 0 */
} cvo_fe_stereo_rig;                     /* 168 bytes, no padding */

/* One context per image size, device and stream.  `stream` as in cvo_hip_create
 * (NULL: a stream of its own).  Images must be at least 64 x 64. */
int cvo_fe_create(int device, void *stream, int width, int height, cvo_fe_ctx **out);
int cvo_fe_destroy(cvo_fe_ctx *ctx);
const char *cvo_fe_last_error(const cvo_fe_ctx *ctx);

/* num_want of pcd_generator (ref src/pcd_generator.cpp:22; default 3000) */
int cvo_fe_set_num_want(cvo_fe_ctx *ctx, int num_want);

/* load_image + create_pointcloud.
 *   img:   height rows of width*3 bytes, `img_stride` bytes apart, channel order as
 *          decoded from the file by cv::imread (B, G, R) -- the reference hands that
 *          to its RGB conversions unchanged, and so does this.
 *   depth: height rows of width uint16, `depth_stride` BYTES apart; while a depth camera is
 *          set (cvo_fe_set_depth_camera): rig.height rows of rig.width uint16, and
 *          depth_stride >= rig.width * 2.
 *   dataset_seq: camera table index (ref src/pcd_generator.cpp:241-295); 1 = TUM fr1.
 *          Ignored while the context has a camera model of its own (cvo_fe_set_camera).
 *   positions: capacity*3 floats (x y z per point); features: capacity*5 floats,
 *   ROW-major (CVO_HIP_FEAT_ROWMAJOR).  Points are in image scan order.
 *   *num_points: points found; if it exceeds `capacity` only the first `capacity`
 *   are stored and CVO_HIP_ERR_INVALID is returned. */
int cvo_fe_create_pointcloud(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const uint16_t *depth,
                             size_t depth_stride, int dataset_seq, int feature_type, float *positions,
                             float *features, int capacity, int *num_points);

/* The context's own pinned staging images (width*3 bytes per colour row -- under a pixel format
 * the packed image, rows * row_bytes bytes of cvo_fe_pixel_layout, and the pointer is valid until
 * the next cvo_fe_set_pixel_format() -- width uint16 per
 * depth row, no padding): a decoder that writes straight into them -- e.g. a cv::Mat header
 * over the pointer handed to cv::imdecode -- saves the copy that submit() / create_pointcloud()
 * otherwise make; pass these same pointers (and the dense strides) to them.  They may be
 * refilled once the frame has been collected.  While a depth camera is set the depth image is
 * of its size; the depth pointer is valid until the next cvo_fe_set_depth_camera().  Under a float
 * depth format (cvo_fe_set_depth_format) *depth points at the float staging image instead. */
int cvo_fe_host_buffers(cvo_fe_ctx *ctx, uint8_t **img, uint16_t **depth);

/* The same in two halves, for callers that have other work while the GPU is busy (the
 * drivers register frame k while frame k+1 is in the front end): submit() stages the
 * images, enqueues every kernel and the copies back and returns; collect() waits, runs the
 * rare edge top-up if the frame needs it, and delivers the cloud.  One frame in flight per
 * context; the image buffers may be re-used as soon as submit() returns. */
int cvo_fe_submit(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const uint16_t *depth,
                  size_t depth_stride, int dataset_seq, int feature_type);
int cvo_fe_collect(cvo_fe_ctx *ctx, float *positions, float *features, int capacity, int *num_points);

/* collect() without the copy to the host: the cloud stays in device memory (positions
 * n x 3, features n x 5 row-major, floats) for cvo_hip_set_fixed_device / _set_moving_device.
 * The pointers are valid until the next submit() / create_pointcloud() on this context. */
int cvo_fe_collect_device(cvo_fe_ctx *ctx, const float **d_positions, const float **d_features, int *num_points);

/* 1: the following frames are collected with cvo_fe_collect_device(): submit() then does not
 * start the (optimistic) copy of the cloud to the host.  cvo_fe_collect() still works. */
int cvo_fe_set_device_output(cvo_fe_ctx *ctx, int on);

/* While a model is set every frame of the context uses it and the `dataset_seq` argument of
 * create_pointcloud() / submit() is ignored; model == NULL: back to the table (the state of a
 * new context).  CVO_HIP_ERR_INVALID for a non-finite member, for fx, fy or depth_scale <= 0,
 * and while a frame is submitted and not collected; the context keeps what it had.  The raw
 * images and the map of the contract above take device memory only once a model with a
 * non-zero `dist` has been set. */
int cvo_fe_set_camera(cvo_fe_ctx *ctx, const cvo_fe_camera_model *model);
/* *custom = 1 and the model set, or *custom = 0 and the table row of the last frame's
 * dataset_seq with zero distortion.  `custom` may be NULL. */
int cvo_fe_get_camera(const cvo_fe_ctx *ctx, cvo_fe_camera_model *out, int *custom);

/* While a rig is set the depth image of every frame is the depth camera's (see the
 * registration contract at cvo_fe_depth_camera); rig == NULL: depth is registered again (the
 * state of a new context).  CVO_HIP_ERR_INVALID, the context keeping what it had: a null
 * context; a frame submitted and not collected; width or height outside [8, 8192]; a
 * non-finite member; fx, fy or depth_scale <= 0; max_range > 0 && max_range <= min_range; R
 * further than 1e-3 (largest absolute entry of R R^T - I) from orthonormal or with a
 * non-positive determinant.  The raw depth, the ray table and the z-buffer take device memory
 * only once a rig has been set. */
int cvo_fe_set_depth_camera(cvo_fe_ctx *ctx, const cvo_fe_depth_camera *rig);
/* *set = 1 and the rig, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_depth_camera(const cvo_fe_ctx *ctx, cvo_fe_depth_camera *out, int *set);

/* While a gate is set every frame passes its depth through the gate contract at cvo_fe_depth_gate;
 * gate == NULL: no gate (the state of a new context).  CVO_HIP_ERR_INVALID, the context keeping
 * what it had: a null context; a frame submitted and not collected; whatever
 * cvo_fe_check_depth_gate refuses.  A gate whose tests are all off (min_range <= 0, max_range <= 0,
 * jump_rel == 0, hole_border == 0) is accepted and gates nothing.  The ungated plane and the flags
 * take device memory only once a gate or a mask has been set. */
int cvo_fe_set_depth_gate(cvo_fe_ctx *ctx, const cvo_fe_depth_gate *gate);
/* *set = 1 and the gate, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_depth_gate(const cvo_fe_ctx *ctx, cvo_fe_depth_gate *out, int *set);
/* A mask for every following frame: height rows of width bytes, `stride` bytes apart, non-zero =
 * this pixel gives no point; mask == NULL: no mask (the state of a new context).  The bytes are
 * copied into a pinned image of the context before the call returns; the next submit() uploads
 * them in front of its frame.  The mask stays until it is replaced or cleared: a caller with a mask
 * per frame calls this before every submit().  Mask and gate are independent: either alone makes
 * the gate stage run.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a
 * frame submitted and not collected; stride < width.  The device and the pinned mask take memory
 * only once a mask has been set.
 * UNDER INPUT BINNING (cvo_fe_set_input_binning) THE MASK IS width x height OF THE CONTEXT, ON THE WORKING GRID, not
 * the size of the images a frame takes: working pixel (x, y) is block (x, y) of the input image. */
int cvo_fe_set_mask(cvo_fe_ctx *ctx, const uint8_t *mask, size_t stride);

/* While stereo is set a frame is a rectified stereo pair (the stereo contract at cvo_fe_stereo) and goes
 * in through cvo_fe_submit_stereo / cvo_fe_create_pointcloud_stereo; st == NULL: back to depth images (the
 * state of a new context).  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame
 * submitted and not collected; whatever cvo_fe_check_stereo refuses; a depth camera is set; a camera model
 * with a non-zero `dist` is set (a pair that is not rectified goes in with its rig: cvo_fe_set_stereo_rig); st == NULL
 * while a stereo rig is set ("clear the rig first").  While stereo is set
 * cvo_fe_set_depth_camera refuses a rig, cvo_fe_set_camera refuses a model with a non-zero `dist`, and
 * cvo_fe_submit / cvo_fe_create_pointcloud refuse.  The right image, the census planes, the cost sums and
 * the disparity maps take device and pinned memory only once stereo has been set. */
int cvo_fe_set_stereo(cvo_fe_ctx *ctx, const cvo_fe_stereo *st);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_stereo(const cvo_fe_ctx *ctx, cvo_fe_stereo *out, int *set);
/* The path mask of step 4 of the stereo contract: bit b set, direction b is summed into S.  Any non-empty subset
 * of the eight bits is accepted: a caller pays one launch per path and may want a subset, and under a mask of one
 * bit CVO_FE_STAGE_SGM_SUM is that direction's L_r alone. */
enum { CVO_FE_PATHS_4 = 0x0F, CVO_FE_PATHS_8 = 0xFF };
/* The mask is a setting of the context, like num_want: a new context has CVO_FE_PATHS_4; it may be set with or
 * without stereo set, survives cvo_fe_set_stereo (settings or NULL) and changes of the rig, is read by stereo frames
 * only and takes no memory.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame
 * submitted and not collected; a mask cvo_fe_check_stereo_paths refuses. */
int cvo_fe_set_stereo_paths(cvo_fe_ctx *ctx, uint32_t mask);
int cvo_fe_get_stereo_paths(const cvo_fe_ctx *ctx, uint32_t *mask);
/* The speckle filter of the stereo matcher (the speckle contract at cvo_fe_speckle); sp == NULL: no filter (the state
 * of a new context).  A setting of the context, like the path mask: it may be set with or without stereo set, survives
 * cvo_fe_set_stereo (settings or NULL) and changes of the rig, and is read by stereo frames only.  Without it a frame
 * launches no kernel of the filter.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame
 * submitted and not collected; settings cvo_fe_check_speckle refuses.  The filter's planes (parents, sums, sizes)
 * take device memory only once it has been set and are given back when it is cleared. */
int cvo_fe_set_stereo_speckle(cvo_fe_ctx *ctx, const cvo_fe_speckle *sp);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_stereo_speckle(const cvo_fe_ctx *ctx, cvo_fe_speckle *out, int *set);
/* The median stage (the median contract at cvo_fe_depth_median); m == NULL: no filter (the state of a new context).  A
 * setting of the context, like the path mask: every kind of frame reads it and it survives every other setter.  Without
 * it a frame launches no kernel of the stage and every stage writes where it writes without.  CVO_HIP_ERR_INVALID, the
 * context keeping what it had: a null context; a frame submitted and not collected; settings cvo_fe_check_depth_median
 * refuses.  The stage's two planes (A and the flags) take device memory only once it has been set and are given back
 * when it is cleared. */
int cvo_fe_set_depth_median(cvo_fe_ctx *ctx, const cvo_fe_depth_median *m);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_depth_median(const cvo_fe_ctx *ctx, cvo_fe_depth_median *out, int *set);
/* The infill stage (the infill contract at cvo_fe_depth_infill); f == NULL: no stage (the state of a new context).  A
 * setting of the context, like the median filter: every kind of frame reads it and it survives every other setter.
 * Without it a frame launches no kernel of the stage, a captured graph has no node of it, and every stage writes where
 * it writes without.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame submitted and not
 * collected; settings cvo_fe_check_depth_infill refuses.  The stage's two planes (S and the flags) take device memory
 * only once it has been set and are given back when it is cleared. */
int cvo_fe_set_depth_infill(cvo_fe_ctx *ctx, const cvo_fe_depth_infill *f);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_depth_infill(const cvo_fe_ctx *ctx, cvo_fe_depth_infill *out, int *set);
/* A scan source (the LiDAR contract at cvo_fe_lidar); l == NULL: depth images again (the state of a new context).
 * While it is set a frame goes in through cvo_fe_submit_lidar / cvo_fe_create_pointcloud_lidar; cvo_fe_submit and
 * cvo_fe_create_pointcloud refuse, and cvo_fe_set_stereo and cvo_fe_set_depth_camera refuse settings and rigs.
 * CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame submitted and not collected; settings
 * cvo_fe_check_lidar refuses; stereo set; a depth camera set.  The staging of a scan (pinned and device memory of
 * max_points points), the z-buffer and the planes of the stage take memory only once it has been set and are given back
 * when it is cleared. */
int cvo_fe_set_lidar(cvo_fe_ctx *ctx, const cvo_fe_lidar *l);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_lidar(const cvo_fe_ctx *ctx, cvo_fe_lidar *out, int *set);
/* A sweep for the scan source (the sweep contract at cvo_fe_lidar_sweep); sw == NULL: none (the state of a new context
 * and of a new scan source).  It needs a scan source and goes when the scan source goes (cvo_fe_set_lidar(ctx, NULL));
 * other settings of the scan source leave it.  The frame's twist is zero after every call that sets a sweep.  Under a
 * field mode a frame's staging and its copy hold 16 bytes per point instead of 12.  CVO_HIP_ERR_INVALID, the context
 * keeping what it had: a null context; a frame submitted and not collected; no scan source; settings
 * cvo_fe_check_lidar_sweep refuses.  Without a sweep a frame launches the kernel it launched before there was one. */
int cvo_fe_set_lidar_sweep(cvo_fe_ctx *ctx, const cvo_fe_lidar_sweep *sw);
/* *set = 1 and the settings, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_lidar_sweep(const cvo_fe_ctx *ctx, cvo_fe_lidar_sweep *out, int *set);
/* The twist of the scanner's own motion over one full sweep, in its own frame: w (radians per sweep) then v (metres
 * per sweep), so that the scanner's pose at phase s is T0 * Exp(s * twist).  It holds for the frames submitted after
 * the call (a frame submitted and not collected keeps the one it was submitted with) and travels with the frame's
 * points, so that a captured frame is replayed with a twist that changes.  Zero in a new context and after a sweep is
 * set.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null argument; no sweep set; a member that is not
 * finite; |w| > CVO_FE_SWEEP_MAX_ROTATION or |v| > CVO_FE_SWEEP_MAX_TRANSLATION (norms in float64). */
int cvo_fe_set_lidar_motion(cvo_fe_ctx *ctx, const float twist[6]);
/* The twist in force, zero without a sweep. */
int cvo_fe_get_lidar_motion(const cvo_fe_ctx *ctx, float twist[6]);
/* cvo_fe_submit / cvo_fe_create_pointcloud for a colour image and a scan: `img` as there; `points` are num_points
 * records `stride_bytes` apart whose first three floats are x, y, z.  The points are copied to the context's pinned
 * staging before the call returns.  CVO_HIP_ERR_INVALID without a scan source, for num_points outside
 * [0, max_points], a stride below 12 or not a multiple of 4, under a sweep with a field mode a stride below
 * time_offset + 4, and null points with num_points > 0.  collect,
 * collect_device, get_info, set_device_output, set_num_want, the mask, the gate, the median and the select mode work on
 * such a frame as on any other. */
int cvo_fe_submit_lidar(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const void *points, size_t stride_bytes,
                        int num_points, int dataset_seq, int feature_type);
int cvo_fe_create_pointcloud_lidar(cvo_fe_ctx *ctx, const uint8_t *img, size_t img_stride, const void *points,
                                   size_t stride_bytes, int num_points, int dataset_seq, int feature_type,
                                   float *positions, float *features, int capacity, int *num_points_out);
/* cvo_fe_submit / cvo_fe_create_pointcloud for a stereo pair: `left` and `right` are height rows of
 * width*3 bytes each, as `img` there (a caller whose right image is grey replicates it); the left image
 * is the colour image of the frame.  CVO_HIP_ERR_INVALID without stereo set.  collect, collect_device,
 * get_info, set_device_output and set_num_want work on a stereo frame as on any other. */
int cvo_fe_submit_stereo(cvo_fe_ctx *ctx, const uint8_t *left, size_t left_stride, const uint8_t *right,
                         size_t right_stride, int dataset_seq, int feature_type);
int cvo_fe_create_pointcloud_stereo(cvo_fe_ctx *ctx, const uint8_t *left, size_t left_stride, const uint8_t *right,
                                    size_t right_stride, int dataset_seq, int feature_type, float *positions,
                                    float *features, int capacity, int *num_points);

/* While a rig is set a frame is a RAW stereo pair (the rig contract at cvo_fe_stereo_rig); rig == NULL: back to
 * rectified pairs (the state after cvo_fe_set_stereo).  CVO_HIP_ERR_INVALID, the context keeping what it had: a
 * null context; a frame submitted and not collected; stereo not set; a cvo_fe_set_camera model set (of any
 * kind: the rig is the camera); whatever cvo_fe_check_stereo_rig refuses.  While a rig is set
 * cvo_fe_set_camera(model) and cvo_fe_set_stereo(NULL) refuse ("clear the rig first"); other stereo settings are
 * welcome; cvo_fe_get_camera returns the rectified pinhole with zero `dist` and *custom = 1.  The raw images,
 * the four map planes and the validity plane take device memory only once a rig has been set and are given back
 * when it is cleared. */
int cvo_fe_set_stereo_rig(cvo_fe_ctx *ctx, const cvo_fe_stereo_rig *rig);
/* *set = 1 and the rig, or *set = 0 and *out zeroed.  `set` may be NULL. */
int cvo_fe_get_stereo_rig(const cvo_fe_ctx *ctx, cvo_fe_stereo_rig *out, int *set);

/* THE SELECTION CONTRACT (this library's own definition, in arithmetic; not pinned against anything).
 *
 * CVO_FE_SELECT_IMAGE is the reference's selector, held to thirdparty/PixelSelector2.cpp bit for bit (the opening
 * comment): about num_want pixels by the image's gradients alone; back-projection then drops every pick whose depth
 * is 0, so num_points is an unknown fraction of num_selected.  Under CVO_FE_SELECT_DEPTH a pixel without depth does
 * not compete.  Let Z be CVO_FE_STAGE_RECT_DEPTH: the plane the cloud is made from, behind rectification, the depth
 * camera's registration, the stereo matcher, the speckle filter and the gate; valid(x, y) := Z(x, y) != 0.
 *
 *   1. Thresholds.  makeHists is unchanged and reads every pixel, valid or not: CVO_FE_STAGE_THS is the plane of
 *      CVO_FE_SELECT_IMAGE.  The thresholds describe the image's texture; a hole in the depth image must not move,
 *      through the 3x3 smoothing, the threshold of a cell three cells away.
 *   2. select.  A pixel (xf, yf) with !valid(xf, yf) is skipped exactly where, and exactly as, a pixel outside the
 *      margin is: the test is  xf < 4 || xf >= w-5 || yf < 4 || yf > h-4 || Z(xf, yf) == 0.  Such a pixel is a
 *      candidate at no level, sets no "-2" mark, and its map value is 0.  Validity is always that of the level-0
 *      pixel (xf, yf), also for the level-1 and level-2 tests, which look up ag1 at (xf/2, yf/2) and ag2 at
 *      (xf/4, yf/4) FOR that pixel.  Blocks, visiting order, "first largest" and the precedence of the levels are
 *      otherwise unchanged; in closed form, over the pixels inside the margin that are valid:
 *        every B2 (pot x pot) holding a pixel with ag0 > th0 keeps the first largest ag0 among them (map 1);
 *        every B3 (2pot x 2pot) without such a pixel that holds one with ag1 > th1 keeps the first largest ag1 (map 2);
 *        every B4 (4pot x 4pot) without either that holds one with ag2 > th2 keeps the first largest ag2 (map 4).
 *      "A B3 without a level-0 hit" thus means: without one among pixels with depth.
 *   3. makeMaps is unchanged, on the counts select now gives: numHave, the one re-selection and its ideal potential
 *      (numHave == 0: the float divisions by zero as IEEE does them -- quotia = +inf, the ideal potential 1, a second
 *      pass at potential 1 that finds nothing, no sub-sampling), charTH, and the running index rn into the random
 *      bytes over the chosen pixels in scan order.
 *   4. The Canny top-up.  The trigger is unchanged, num_selected < num_want / 3, and num_selected now counts pixels
 *      with depth.  Canny itself is unchanged and reads the image only.  Per 8x8 block the top-up takes the first
 *      pixel in row order that is an edge, is free in the map and is valid.
 *
 * Consequences: every non-zero pixel of CVO_FE_STAGE_MAP is valid; num_points == num_selected where no top-up ran
 * and num_points == num_selected + (pixels topped up) where one ran; on a frame that is valid everywhere every plane
 * and every point is that of CVO_FE_SELECT_IMAGE.  num_selected is "pixels the selector kept" in both modes. */
enum { CVO_FE_SELECT_IMAGE = 0,    /* the reference: by the image alone (a new context) */
       CVO_FE_SELECT_DEPTH = 1 };  /* among the pixels that have a depth */
/* The mode is a setting of the context, like the path mask: it survives every other setter, is read by every frame
 * (depth, stereo, under a rig, a gate, a mask) and takes no memory; both modes issue the same launches in the same
 * order.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame submitted and not collected;
 * a mode cvo_fe_check_select_mode refuses. */
int cvo_fe_set_select_mode(cvo_fe_ctx *ctx, int mode);
int cvo_fe_get_select_mode(const cvo_fe_ctx *ctx, int *mode);
/* CVO_HIP_OK for a mode cvo_fe_set_select_mode() would accept on an idle context: one of the two above.  The one
 * statement of what is accepted.  Host only. */
int cvo_fe_check_select_mode(int mode);

/* what the last create_pointcloud / collect did */
int cvo_fe_get_info(const cvo_fe_ctx *ctx, cvo_fe_info *out);
/* copy an intermediate image of the last create_pointcloud to host memory */
int cvo_fe_read_stage(cvo_fe_ctx *ctx, int stage, void *out, size_t bytes);

/* The selector's random bytes (ref thirdparty/PixelSelector2.cpp:35-37:
 * srand(3141592); rand() & 0xFF) from a restatement of the C library's additive
 * feedback generator: host only, no device needed. */
int cvo_fe_random_pattern(int n, uint8_t *out);
/* The camera table: {depth scale, fx, fy, cx, cy}.  Host only. */
int cvo_fe_camera(int dataset_seq, float cam[5]);
/* The map of the rectification contract (see cvo_fe_camera_model) for a width x height image:
 * qu and qv, width*height int32 each, row-major.  Host only.  CVO_HIP_ERR_INVALID for a null
 * pointer, width or height < 1 and a model cvo_fe_set_camera() would refuse. */
int cvo_fe_rectify_map(const cvo_fe_camera_model *model, int width, int height, int32_t *qu, int32_t *qv);

/* The ray table of the registration contract (see cvo_fe_depth_camera): xn and yn,
 * (height+1) x (width+1) floats each, row-major.  Host only.  CVO_HIP_ERR_INVALID for a null
 * pointer and a rig cvo_fe_set_depth_camera() would refuse. */
int cvo_fe_depth_rays(const cvo_fe_depth_camera *rig, float *xn, float *yn);
/* CVO_HIP_OK for a rig cvo_fe_set_depth_camera() would accept on an idle context, CVO_HIP_ERR_INVALID
 * otherwise (and for NULL): the one statement of what a rig must satisfy.  Host only. */
int cvo_fe_check_depth_camera(const cvo_fe_depth_camera *rig);
/* CVO_HIP_OK for a gate cvo_fe_set_depth_gate() would accept on an idle context, CVO_HIP_ERR_INVALID
 * otherwise: NULL; a non-finite float; jump_rel < 0; max_range > 0 && max_range <= min_range; grow
 * outside [0, 3]; hole_border not 0 or 1; pad_ != 0.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_depth_gate(const cvo_fe_depth_gate *gate);
/* CVO_HIP_OK for settings cvo_fe_set_stereo() would accept on an idle context without a depth camera and
 * a distorting model, CVO_HIP_ERR_INVALID otherwise: NULL; baseline not finite or <= 0; max_disp no multiple
 * of 8 in [8, 128]; min_disp < 1; not 1 <= p1 <= p2 <= 255; uniqueness outside [0, 99]; lr_max outside
 * [-1, 8]; pad_ != 0.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_stereo(const cvo_fe_stereo *st);
/* CVO_HIP_OK for a path mask cvo_fe_set_stereo_paths() would accept on an idle context: 1 <= mask <= 0xFF.  Host only. */
int cvo_fe_check_stereo_paths(uint32_t mask);
/* U(q) of the stereo contract for q = 0 .. 16*max_disp - 1.  Host only.  CVO_HIP_ERR_INVALID for a null
 * pointer, settings cvo_fe_check_stereo refuses, and fx or depth_scale not finite or <= 0. */
int cvo_fe_stereo_depth_table(const cvo_fe_stereo *st, float fx, float depth_scale, uint16_t *out);
/* CVO_HIP_OK for a rig cvo_fe_set_stereo_rig() would accept on an idle context with stereo set and no camera model,
 * CVO_HIP_ERR_INVALID otherwise: NULL; a member that is not finite; fx or fy of either camera or of the rectified
 * pinhole, depth_scale or baseline <= 0; R_left or R_right further than 1e-3 (largest absolute entry of
 * R R^T - I) from orthonormal or with a non-positive determinant (the depth camera's rule).  The one statement of
 * what is accepted.  Host only. */
int cvo_fe_check_stereo_rig(const cvo_fe_stereo_rig *rig);
/* The rig of a calibration for width x height images (the helper of the rig contract).  Host only.
 * CVO_HIP_ERR_INVALID, *out untouched: a null pointer; width or height < 1; a member of calib or depth_scale not
 * finite; fx or fy of either camera or depth_scale <= 0; R no rotation (the rule above); what steps 1 and 3 refuse. */
int cvo_fe_stereo_rectify(const cvo_fe_stereo_calib *calib, int width, int height, cvo_fe_stereo_rig *out,
                          float depth_scale);
/* The map of the rig contract for camera `which` (0 left, 1 right) and a width x height image: qu and qv,
 * width*height int32 each, row-major.  Host only.  CVO_HIP_ERR_INVALID for a null pointer, width or height < 1,
 * `which` not 0 or 1 and a rig cvo_fe_check_stereo_rig refuses. */
int cvo_fe_stereo_rig_map(const cvo_fe_stereo_rig *rig, int which, int width, int height, int32_t *qu, int32_t *qv);

/* CVO_HIP_OK for settings cvo_fe_set_stereo_speckle() would accept on an idle context, CVO_HIP_ERR_INVALID otherwise:
 * NULL; max_size outside [1, 2^26]; max_diff outside [0, 65535].  The one statement of what is accepted.  Host only. */
int cvo_fe_check_speckle(const cvo_fe_speckle *sp);
/* The filter of the speckle contract on any uint16 plane with 0 = none -- a disparity map of another matcher, a depth
 * image -- by the kernels a stereo frame runs, without a context: host arrays in and out.  `plane` is height rows of
 * width uint16, `stride_bytes` BYTES apart, and is filtered in place; `sizes`, if not NULL, receives SIZE (width*height
 * uint32, dense); *removed the number of pixels zeroed.  CVO_HIP_ERR_INVALID for a null plane or `removed`, width or
 * height outside [1, 8192], stride_bytes < width*2 and settings cvo_fe_check_speckle refuses; CVO_HIP_ERR_NODEVICE
 * without such a device. */
int cvo_fe_filter_speckles(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                           const cvo_fe_speckle *sp, uint32_t *sizes, int *removed);

/* CVO_HIP_OK for settings cvo_fe_set_depth_median() would accept on an idle context, CVO_HIP_ERR_INVALID otherwise:
 * NULL; a radius that is not 1 or 2; fill_min outside [0, (2*radius+1)^2 - 1]; pad_ != 0.  The one statement of what is
 * accepted.  Host only. */
int cvo_fe_check_depth_median(const cvo_fe_depth_median *m);
/* The stage of the median contract on any uint16 plane with 0 = none -- a depth image of another pipeline, a disparity
 * map -- by the kernel a frame runs, without a context: host arrays in and out.  `plane` is height rows of width uint16,
 * `stride_bytes` BYTES apart; it is A on entry and B on return (the bytes between the rows stay); `flags`, if not NULL,
 * receives MEDIAN (width*height uint8, dense); *changed and *filled the numbers of pixels with either value.
 * CVO_HIP_ERR_INVALID for a null plane, `changed` or `filled`, width or height outside [1, 8192],
 * stride_bytes < width*2 and settings cvo_fe_check_depth_median refuses; CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_median_plane(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                        const cvo_fe_depth_median *m, uint8_t *flags, int *changed, int *filled);

/* CVO_HIP_OK for settings cvo_fe_set_depth_infill() would accept on an idle context, CVO_HIP_ERR_INVALID otherwise:
 * NULL; gap_x outside [0, 15]; gap_y outside [0, 31]; a jump_rel that is not finite or is below 0; pad_ != 0.  Both
 * gaps 0 is accepted and fills nothing.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_depth_infill(const cvo_fe_depth_infill *f);
/* The stage of the infill contract on any uint16 plane with 0 = none -- a depth image of another pipeline, a disparity
 * map -- by the kernel a frame runs, without a context: host arrays in and out.  `plane` is height rows of width uint16,
 * `stride_bytes` BYTES apart; it is S on entry and F on return (the bytes between the rows stay; "in place" is the
 * host array only, the kernel writes another plane than it reads); `flags`, if not NULL, receives INFILL (width*height
 * uint8, dense); *row_filled and *col_filled the numbers of pixels with CVO_FE_INFILL_ROW and CVO_FE_INFILL_COL.
 * CVO_HIP_ERR_INVALID for a null plane, `row_filled` or `col_filled`, width or height outside [1, 8192],
 * stride_bytes < width*2 and settings cvo_fe_check_depth_infill refuses; CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_infill_plane(int device, uint16_t *plane, size_t stride_bytes, int width, int height,
                        const cvo_fe_depth_infill *f, uint8_t *flags, int *row_filled, int *col_filled);

/* CVO_HIP_OK for a format of the list above that fits a width x height picture (the sizes of the unpack contract;
 * width and height at least 1), CVO_HIP_ERR_INVALID otherwise.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_pixel_format(int format, int width, int height);
/* The layout table of the unpack contract: *row_bytes and *rows of a packed width x height image.
 * CVO_HIP_ERR_INVALID for a null pointer and for what cvo_fe_check_pixel_format refuses.  Host only. */
int cvo_fe_pixel_layout(int format, int width, int height, size_t *row_bytes, int *rows);
/* The format of EVERY colour image of every following frame: the image of cvo_fe_submit / cvo_fe_create_pointcloud
 * and of cvo_fe_submit_lidar, and both images of cvo_fe_submit_stereo (one format for the pair, with or without a
 * stereo rig).  Their strides are then at least row_bytes, and their rows are `rows`.  A setting of its own: it
 * survives every other setter.  CVO_FE_PIXEL_BGR8: a new context's state; the buffers of the setting are freed and a
 * frame launches what it launched before.  CVO_HIP_ERR_INVALID while a frame is pending and for a format
 * cvo_fe_check_pixel_format refuses at the context's size; cvo_fe_last_error() says which. */
int cvo_fe_set_pixel_format(cvo_fe_ctx *ctx, int format);
int cvo_fe_get_pixel_format(const cvo_fe_ctx *ctx, int *format);
/* The unpack contract on any packed image by the kernel a frame runs, without a context: host arrays in and out.
 * `src` is `rows` rows of row_bytes bytes, `stride_bytes` apart, and is not written; `bgr` receives width*height*3
 * bytes, dense.  Under CVO_FE_PIXEL_BGR8 it is a copy.  CVO_HIP_ERR_INVALID for a null pointer, width or height
 * outside [1, 8192], a format cvo_fe_check_pixel_format refuses at that size and stride_bytes < row_bytes;
 * CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_unpack_image(int device, const uint8_t *src, size_t stride_bytes, int width, int height, int format,
                        uint8_t *bgr);

/* CVO_HIP_OK for what cvo_fe_set_depth_format() would accept on an idle context, CVO_HIP_ERR_INVALID otherwise: a format
 * that is none of CVO_FE_DEPTH_*; a unit that is not finite or lies outside [2^-20, 2^20]; under CVO_FE_DEPTH_U16 a unit
 * other than 1.  The one statement of what is accepted.  Host only; it asks for no device. */
int cvo_fe_check_depth_format(int format, float unit);
/* The format of the depth image of every following frame that has one (cvo_fe_submit / cvo_fe_create_pointcloud and
 * cvo_fe_submit_device): those take the image through their `depth` pointer, cast; depth_stride is in bytes, at least
 * the depth image's width times the bytes of a value, and a multiple of the bytes of a value.  A setting of its own: it
 * survives every other setter, cvo_fe_set_depth_camera in either order included (the float staging follows the rig's
 * size).  CVO_FE_DEPTH_U16 with unit 1: a new context's state; the buffers of the setting are freed and a frame launches
 * what it launched before.  Under a float format cvo_fe_host_buffers' *depth points at the float staging image (dw*dh
 * values of 4 or 2 bytes, valid until the next cvo_fe_set_depth_format / cvo_fe_set_depth_camera).
 * CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame submitted and not collected; what
 * cvo_fe_check_depth_format refuses. */
int cvo_fe_set_depth_format(cvo_fe_ctx *ctx, int format, float unit);
int cvo_fe_get_depth_format(const cvo_fe_ctx *ctx, int *format, float *unit);
/* The depth-format contract on any plane by the kernel a frame runs, without a context: host arrays in and out.  `src`
 * is height rows of width values, `stride_bytes` apart, and is not written; `out` receives width*height uint16, dense.
 * `scale` is the contract's.  Under CVO_FE_DEPTH_U16 it is a copy on the host and no device is asked for.
 * CVO_HIP_ERR_INVALID, before a device is asked for: a null pointer; width or height outside [1, 8192]; what
 * cvo_fe_check_depth_format refuses; a scale that is not finite and positive; stride_bytes below the row or not a
 * multiple of the bytes of a value.  CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_convert_depth(int device, const void *src, size_t stride_bytes, int width, int height, int format, float unit,
                         float scale, uint16_t *out);

/* FRAMES WHOSE IMAGES ARE IN DEVICE MEMORY: a decoder or a camera pipeline that delivers into device memory, a depth
 * network in the same process.  cvo_fe_submit_device / cvo_fe_submit_stereo_device are cvo_fe_submit /
 * cvo_fe_submit_stereo for such images and are followed by cvo_fe_collect or cvo_fe_collect_device like them.  The
 * images have the layout of the host forms: the pixel format in force (packed rows at one pitch, NV12's chroma rows
 * included), the depth format in force, the depth camera's size while one is set.  Host and device submits may
 * alternate on one context, frame by frame.
 *
 * THE DEVICE-INPUT CONTRACT.
 * What is accepted.  A pointer is accepted only if hipPointerGetAttributes reports device memory (hipMemoryTypeDevice)
 *   of the context's device.  Pinned host memory, managed memory, another device's memory and pointers the runtime
 *   does not know are refused with CVO_HIP_ERR_INVALID and a message (cvo_fe_last_error).
 * Checks before anything is enqueued.  A stride below the row, and a depth stride or a depth pointer that is not a
 *   multiple of the bytes of a depth value, are refused (nothing more is asked of a pointer's alignment).  If hipMemGetAddressRange answers for a pointer, an image whose last byte -- at
 *   (rows - 1) * stride + row_bytes from its first -- lies past the end of the allocation is refused too.  The runtime's
 *   range is the ALLOCATION's, which may be larger than the caller's array (an allocator that cuts arrays out of larger
 *   blocks): the check catches an image that leaves the block, not one that leaves the array.
 * Ordering.  The images are read by work enqueued on the context's stream during the call.  What wrote them must have
 *   completed, or have been enqueued on that same stream, before the call; they must stay valid and unwritten until the
 *   frame's collect has returned.  The library never writes them.
 * Results.  The cloud, cvo_fe_info and every cvo_fe_read_stage plane of a device frame are, by bits, those of the same
 *   images submitted from the host.
 * A captured frame graph holds no pointer of the caller's: the images are brought to the buffers an upload lands in by one
 *   pitched device-to-device copy each, in front of the frame and outside its graph (a float depth image is not copied:
 *   the conversion kernel reads it in place), and the frame's graph is a variant without the uploads.
 * LiDAR frames are out of scope: a scan's header and time words are packed by host code, and a device-side packer is a
 *   piece of work of its own; cvo_fe_submit_device refuses on a context with a scan source. */
int cvo_fe_submit_device(cvo_fe_ctx *ctx, const void *d_img, size_t img_stride, const void *d_depth,
                         size_t depth_stride, int dataset_seq, int feature_type);
int cvo_fe_submit_stereo_device(cvo_fe_ctx *ctx, const void *d_left, size_t left_stride, const void *d_right,
                                size_t right_stride, int dataset_seq, int feature_type);

/*
 * THE BINNING CONTRACT.  The results are defined by the integer arithmetic below, not by the device; it is this
 * library's own definition and is NOT pinned against cv::resize(INTER_AREA) or any SDK.  While binning is set the
 * context's width x height (w x h) is the WORKING SIZE, and every image that is uploaded or read from the caller's
 * device memory is fw x fh.  Block (x, y) of an input plane is the f x f input pixels (fx + i, fy + j), 0 <= i, j < f;
 * n = f*f.
 *   Colour (the unpacked B G R image, and both images of a stereo pair).  Per channel, S = the sum of the n bytes of
 *     the block, out = (S + (n >> 1)) / n, floor division.  For f = 2 and f = 4 that is round half up; for f = 3 a half
 *     cannot occur.  A flat block comes back exactly.
 *   Depth (the uint16 depth image of a frame that has one and no depth camera).  k = the number of non-zero values of
 *     the block, v_0 <= ... <= v_(k-1) those values in ascending order.  out = v_((k-1) >> 1) if k >= depth_min, else
 *     0: the lower median of the median contract, always a value some pixel of the block holds and never an average
 *     across an occlusion edge.  65535 is a depth like any other.  With depth_min = n a block with any hole has no depth.
 *   Every output pixel is a function of its own block alone.
 * Where it sits.  One launch, behind k_fe_unpack (which under a pixel format runs at the input size; the format must
 * pass cvo_fe_check_pixel_format at fw x fh) and behind k_fe_depth_convert (which under a float depth format runs at
 * the input size), and in front of everything else: rectification of either kind, the depth camera's warp, the LiDAR
 * projection, infill, median, gate and level 0.  It writes the buffers an upload or those two kernels fill without
 * binning; they fill input-size buffers instead.  No later stage changes or learns of it: by bits, the frame is that
 * of a context of the working size, without binning, fed the binned images.
 *   a depth camera set: only the colour image is binned; the depth image keeps the rig's own size
 *   a scan source:      only the colour image
 *   stereo:             both colour images, in the same launch
 * EVERY CAMERA OF THE CONTEXT DESCRIBES THE WORKING IMAGE: the model of cvo_fe_set_camera, a stereo rig's two lenses
 * and its rectified pinhole, the colour side of a depth camera's registration and of the LiDAR projection, the table
 * rows of dataset_seq.  The mask of cvo_fe_set_mask is w x h, on the working grid.  A caller who bins and keeps the
 * input image's pinhole gets a cloud f times too large: cvo_fe_bin_camera / cvo_fe_bin_stereo_rig make the working
 * camera.  Pixel centres lie at integer coordinates, so working pixel X is centred at input f X + (f - 1) / 2 and the
 * binned principal point is (cx - (f - 1) / 2) / f, not cx / f.
 * Everything that names "the size of the caller's image" speaks of fw x fh (for depth: unless a depth camera is set):
 * cvo_fe_host_buffers, the stride checks of the submits, the pointer and extent checks of the device submits.
 * Stage ids.  No existing id changes its meaning; each names a working-size plane.  CVO_FE_STAGE_RAW_DEPTH and, under
 * a pixel format or binning, CVO_FE_STAGE_INPUT_BGR / _INPUT_RIGHT_BGR are what the bin wrote.  CVO_FE_STAGE_FULL_*
 * are what it read.
 * Not part of it: factors above 4, and different factors in x and y; binning the Bayer mosaic before the demosaic;
 * binning a depth camera's image or a LiDAR plane; any filter other than the box; cropping an input that is no
 * multiple of f (the caller's pointer and stride do that); fusing the bin into k_fe_unpack or level 0.
 */
typedef struct cvo_fe_binning {
    int32_t factor;      /* f: 2, 3 or 4 */
    int32_t depth_min;   /* 1 .. f*f: a working pixel gets a depth when at least this many pixels of its block have one */
    int32_t pad_;        /* must be 0 */
} cvo_fe_binning;        /* 12 bytes */

/* CVO_HIP_OK for what cvo_fe_set_input_binning() would accept on an idle BGR8 context of the working size
 * width x height, CVO_HIP_ERR_INVALID otherwise: NULL; a factor outside {2, 3, 4}; depth_min outside [1, f*f];
 * pad_ != 0; width or height below 1; f*width or f*height above 8192.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_binning(const cvo_fe_binning *b, int width, int height);
/* Input binning for every following frame.  THE CAMERAS AND THE MASK OF THE CONTEXT DESCRIBE THE WORKING IMAGE (the
 * binning contract above): bin the input image's camera with cvo_fe_bin_camera / cvo_fe_bin_stereo_rig.  A setting of
 * its own: it survives every other setter, in either order with cvo_fe_set_pixel_format, cvo_fe_set_depth_format,
 * cvo_fe_set_depth_camera, cvo_fe_set_stereo, cvo_fe_set_stereo_rig, cvo_fe_set_lidar and cvo_fe_set_camera; the packed
 * staging, the float staging and the right image's staging follow the input size.  Pointers of cvo_fe_host_buffers
 * are valid until the next call.  NULL: off, a new context's state; the buffers of the setting are freed and a frame
 * launches what it launched before.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame
 * submitted and not collected; what cvo_fe_check_binning refuses at the context's size; a pixel format in force that
 * cvo_fe_check_pixel_format refuses at fw x fh.  (In turn cvo_fe_set_pixel_format checks at the input size.) */
int cvo_fe_set_input_binning(cvo_fe_ctx *ctx, const cvo_fe_binning *b);
int cvo_fe_get_input_binning(const cvo_fe_ctx *ctx, cvo_fe_binning *out, int *set);
/* The working camera of an input image's camera.  In float32, each operation rounded on its own:
 *   c = 0.5f * (float)(f - 1)   (exact: 0.5, 1, 1.5)
 *   fx' = fx / (float)f;  fy' = fy / (float)f;  cx' = (cx - c) / (float)f;  cy' = (cy - c) / (float)f
 * depth_scale and dist[5] are unchanged (the distortion acts on normalised coordinates).  `out` may be `in`.
 * CVO_HIP_ERR_INVALID for a null pointer, a factor outside {2, 3, 4} and a model cvo_fe_set_camera refuses.  Host only. */
int cvo_fe_bin_camera(const cvo_fe_camera_model *in, int factor, cvo_fe_camera_model *out);
/* The same rule on `left`, `right` and the rectified fx fy cx cy of a rig; the rotations, the baseline and depth_scale
 * are unchanged.  CVO_HIP_ERR_INVALID for a null pointer, such a factor and a rig cvo_fe_check_stereo_rig refuses. */
int cvo_fe_bin_stereo_rig(const cvo_fe_stereo_rig *in, int factor, cvo_fe_stereo_rig *out);
/* The binning contract on any image / plane by the kernel a frame runs, without a context: host arrays in and out.
 * width x height is the OUTPUT size; the source is factor*width x factor*height, `stride_bytes` apart, and is not
 * written; `out` is dense.  *valid: the number of output pixels with a depth.  CVO_HIP_ERR_INVALID for a null pointer,
 * width or height below 1, what cvo_fe_check_binning refuses (cvo_fe_bin_image reads the factor only) and a stride
 * below the source's row; CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_bin_image(int device, const uint8_t *bgr, size_t stride_bytes, int width, int height, int factor, uint8_t *out);
int cvo_fe_bin_depth(int device, const uint16_t *plane, size_t stride_bytes, int width, int height,
                     const cvo_fe_binning *b, uint16_t *out, int *valid);

/* CVO_HIP_OK for settings cvo_fe_set_lidar() would accept on an idle context without stereo and depth camera,
 * CVO_HIP_ERR_INVALID otherwise: NULL; max_points outside [1, 2^21]; splat outside [0, 3]; a float that is not finite;
 * occl_rel < 0; occl_rx or occl_ry outside [0, 7]; max_range > 0 && max_range <= min_range; R failing the depth
 * camera's rotation rule (within 1e-3 of orthonormal, positive determinant); pad_ != 0.  The one statement of what is
 * accepted.  Host only. */
int cvo_fe_check_lidar(const cvo_fe_lidar *l);
/* The stage of the LiDAR contract on any scan by the kernels a frame runs, without a context: host arrays in and out.
 * `points` are n records `stride_bytes` apart (x, y, z first); `cam` is the colour camera as cvo_fe_camera gives it
 * (depth scale, fx, fy, cx, cy).  `plane` receives P (width*height uint16, dense), `unculled`, if not NULL, P0, and
 * `flags`, if not NULL, the bytes of CVO_FE_STAGE_LIDAR; *hits the number of pixels with P0 != 0 and *occluded the
 * number of those the occlusion test dropped.  max_points is not read beyond n <= 2^21.  CVO_HIP_ERR_INVALID for a
 * null `plane`, `cam`, `hits` or `occluded`, null points with n > 0, n outside [0, 2^21], a stride below 12 or not a
 * multiple of 4, width or height outside [1, 8192], a camera that is not finite and positive in scale and focal lengths,
 * and settings cvo_fe_check_lidar refuses; CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_project_points(int device, const void *points, size_t stride_bytes, int n, const cvo_fe_lidar *l,
                          const float cam[5], int width, int height, uint16_t *plane, uint16_t *unculled, uint8_t *flags,
                          int *hits, int *occluded);
/* CVO_HIP_OK for a sweep cvo_fe_set_lidar_sweep() would accept on an idle context with a scan source,
 * CVO_HIP_ERR_INVALID otherwise: NULL; a mode that is none of CVO_FE_SWEEP_*; a float that is not finite; under a field
 * mode time_offset below 12 or not a multiple of 4, time_scale 0, direction != 0; time_origin != 0 outside
 * CVO_FE_SWEEP_TIME_F32; under CVO_FE_SWEEP_AZIMUTH a direction that is neither +1 nor -1, phase0 outside [0, 1);
 * s_ref outside [0, 1]; pad_ != 0.  The one statement of what is accepted.  Host only. */
int cvo_fe_check_lidar_sweep(const cvo_fe_lidar_sweep *sw);
/* The twist for cvo_fe_set_lidar_motion of a caller who assumes the velocity of the last frame interval to hold.  Host
 * only, float64.  `T_cam` is the relative camera pose of the last registration as the registration objects return it
 * in `transform` (row-major 4 x 4): the moving cloud, the LATER frame's, is aligned to the fixed one, the earlier
 * frame's, by y = R^T (z - T), so [R | T] takes coordinates in the earlier camera's frame to coordinates in the later
 * one's, and the later camera's pose in the earlier one's frame -- the camera's motion over the frame interval -- is
 * its inverse M.  With X = [l->R | l->T], the scanner's pose in the camera's frame, the scanner's own motion is
 * X^-1 M X; the twist is its SE(3) logarithm times `sweep_fraction`, the sweep duration over the frame interval
 * (1 for a scanner that spins once per image).  CVO_HIP_ERR_INVALID: a null argument; a member of T_cam or a
 * sweep_fraction that is not finite; sweep_fraction <= 0; a rotation part that fails the depth camera's rotation rule;
 * settings cvo_fe_check_lidar refuses (max_points is not read); a rotation of more than 3 radians over the frame
 * interval; a twist over the caps of cvo_fe_set_lidar_motion. */
int cvo_fe_lidar_twist(const float T_cam[16], const cvo_fe_lidar *l, float sweep_fraction, float twist[6]);
/* cvo_fe_project_points under the sweep contract: its arguments, then the sweep and the scan's twist (what
 * cvo_fe_set_lidar_sweep and cvo_fe_set_lidar_motion accept; under a field mode time_offset + 4 <= stride_bytes).
 * `phase`, if not NULL, receives s of each of the n points and `moved`, if not NULL, p' (3n floats); a point that
 * step 1 or a time that is not finite skipped has NaN in all four.  sw == NULL: cvo_fe_project_points itself (`twist`
 * is not read; phase and moved must be NULL). */
int cvo_fe_project_points_sweep(int device, const void *points, size_t stride_bytes, int n, const cvo_fe_lidar *l,
                                const float cam[5], int width, int height, uint16_t *plane, uint16_t *unculled,
                                uint8_t *flags, int *hits, int *occluded, const cvo_fe_lidar_sweep *sw,
                                const float twist[6], float *phase, float *moved);

/*
 * The photometric contract (cvo_fe_set_photometric; off by default).  The pair weight compares colour bytes of two
 * frames and the selector reads grey gradients of the same bytes, so a surface should give one value in both.  A
 * sensor's response curve, its lens's vignette and an exposure that changes between frames stand against that.  This
 * stage corrects the B G R bytes of every colour image by a per-channel response table, a per-pixel vignette gain and
 * a per-frame gain per channel.  It is this library's own definition, in unsigned integers; tests/fe_photometric_ref.py
 * restates it.
 *   Per pixel p (row-major index at the input size iw x ih) and channel c (0, 1, 2 = B, G, R as the image's bytes)
 *   with input byte b:
 *       L   = response ? response[c][b] : b << 8           (Q8 value, at most 65535)
 *       V   = vignette ? vignette[p]    : 4096              (Q12 gain, 4096 = 1)
 *       A   = L * V                                          (fits 32 bits)
 *       out = min(255, ((uint64)A * G_c + 2^31) >> 32)       (G_c: Q12, at most 65535)
 *   Without tables and with G_c = 4096 the stage is the identity by bytes.
 *   G_c by the flags:
 *     neither CVO_FE_PHOTO_GAIN nor CVO_FE_PHOTO_AUTO: 4096.
 *     CVO_FE_PHOTO_GAIN: the gains of cvo_fe_set_photometric_gain, G = (uint32)(gain * 4096.0f + 0.5f) with each
 *       operation in float32, clamped to [gain_min, gain_max]; 4096 until the first call.  They travel in a header
 *       that the frame's sequence copies to the device, so a captured frame replays under gains that change.
 *     CVO_FE_PHOTO_AUTO: estimated on the device from the image itself (the LEFT image of a stereo pair).
 *       Pixel p counts iff all three of its INPUT bytes lie in [lo, hi] (saturation is the sensor's, so the window
 *       tests what the sensor gave).  k = the number of such pixels, M_c = the sum over them of A_c(p) >> 12, in 64
 *       bits.  T_c is the target: settings.target where that is not all zero, else the lock's.
 *         k < min_count:            G = 4096 on all channels, CVO_FE_PHOTO_FALLBACK; the lock is left as it is.
 *         target all zero and the lock open (k >= min_count): T_c = (M_c + (k >> 1)) / k, G = 4096, the lock
 *                                   closes, CVO_FE_PHOTO_LOCKED.
 *         else, per_channel:        G_c = clamp((T_c * k * 4096 + (M_c >> 1)) / M_c, gain_min, gain_max)
 *         else:                     one G for all channels from T_0 + T_1 + T_2 and M_0 + M_1 + M_2 in the same way.
 *         A divisor of zero (any of the three under per_channel): G = 4096 on all channels, CVO_FE_PHOTO_FALLBACK.
 *       The setter opens the lock; cvo_fe_photometric_rearm opens it again.  With a closed lock T holds.
 *   A stereo pair: both images go through the same tables and the same G.
 * Where it sits.  In place on the image the upload, the copy of a device frame or k_fe_unpack left, at the input size
 * iw x ih: behind the unpack, in front of k_fe_bin (a box mean then averages linearised values) and of everything else.
 * No later stage changes or learns of it: by bits, the frame is that of a context without the stage fed the corrected
 * image.  With the stage on CVO_FE_STAGE_INPUT_BGR / _INPUT_RIGHT_BGR (under binning CVO_FE_STAGE_FULL_BGR /
 * _FULL_RIGHT_BGR) read what the stage wrote, and CVO_FE_STAGE_INPUT_BGR is readable on a BGR8 context too.
 * Not part of it: tables or gains of its own for the right camera; estimating response or vignette; smoothing AUTO
 * gains over time; more than 8 bits per channel behind the stage.
 */
enum { CVO_FE_PHOTO_RESPONSE = 1, CVO_FE_PHOTO_VIGNETTE = 2, CVO_FE_PHOTO_GAIN = 4, CVO_FE_PHOTO_AUTO = 8 };
/* flags of cvo_fe_photometric_frame */
enum { CVO_FE_PHOTO_FALLBACK = 1, CVO_FE_PHOTO_LOCKED = 2 };
typedef struct cvo_fe_photometric {
    uint32_t flags;        /* OR of CVO_FE_PHOTO_RESPONSE, _VIGNETTE, _GAIN, _AUTO; _GAIN and _AUTO exclude each other */
    int32_t lo, hi;        /* 0 <= lo <= hi <= 255: the window of AUTO on the input bytes, both ends inside */
    int32_t min_count;     /* >= 1: AUTO falls back to G = 4096 with fewer counted pixels */
    int32_t per_channel;   /* 0: one gain for all channels; 1: one per channel */
    uint32_t target[3];    /* T_c in Q8 times the vignette's gain, B G R, each <= 65535; all zero: the lock */
    int32_t gain_min, gain_max;   /* Q12: 1 <= gain_min <= gain_max <= 65535 */
    int32_t pad_;          /* must be 0 */
} cvo_fe_photometric;      /* 44 bytes, no padding */
typedef struct cvo_fe_photometric_frame {
    uint32_t gain[3];      /* G_c the frame was corrected with, Q12 */
    uint32_t flags;        /* CVO_FE_PHOTO_FALLBACK, CVO_FE_PHOTO_LOCKED */
    uint64_t count;        /* k (0 without AUTO) */
    uint64_t sum[3];       /* M_c (0 without AUTO) */
    uint32_t target[3];    /* T_c in force behind the frame (0 without AUTO, and while the lock is open) */
    uint32_t pad_;
} cvo_fe_photometric_frame;   /* 64 bytes, no padding */

/* CVO_HIP_OK for settings and tables cvo_fe_set_photometric() would accept, CVO_HIP_ERR_INVALID otherwise: NULL; a flag
 * outside the four; _GAIN together with _AUTO; lo, hi outside 0 <= lo <= hi <= 255; min_count < 1; per_channel outside
 * {0, 1}; a target above 65535; gain_min, gain_max outside 1 <= gain_min <= gain_max <= 65535; pad_ != 0;
 * have_response != (flags & _RESPONSE != 0); have_vignette != (flags & _VIGNETTE != 0); flags == 0 (that, with no
 * tables, is how the setter is told "off", and is no setting).  The one statement of what is accepted.  Host only. */
int cvo_fe_check_photometric(const cvo_fe_photometric *p, int have_response, int have_vignette);
/* The stage for every following frame of any kind.  `response`: 3 x 256 uint16, B G R; `vignette`: iw x ih uint16 in rows
 * `vignette_stride` bytes apart, iw x ih the size of the images a frame takes (under input binning factor times the
 * context's).  Both are copied before the call returns.  p == NULL, or flags == 0 with both tables NULL: off, a new
 * context's state; the stage's memory is given back and a frame launches what it launched before.  A setting of its
 * own: it survives every other setter in either order.  Every call opens the lock of AUTO and puts the caller's gains
 * back to 1.  CVO_HIP_ERR_INVALID, the context keeping what it had: a null context; a frame in flight; what
 * cvo_fe_check_photometric refuses; a vignette stride below iw * 2 or odd.  With a vignette set,
 * cvo_fe_set_input_binning refuses a change of the input size: set the stage off first, then the binning, then the
 * stage with a vignette of the new size. */
int cvo_fe_set_photometric(cvo_fe_ctx *ctx, const cvo_fe_photometric *p, const uint16_t *response, const uint16_t *vignette,
                           size_t vignette_stride);
/* The settings in force (zeroes and *set = 0 without); the tables are not handed back. */
int cvo_fe_get_photometric(const cvo_fe_ctx *ctx, cvo_fe_photometric *out, int *set);
/* The gains (B, G, R) of the frames submitted from now on, under CVO_FE_PHOTO_GAIN; they hold until changed.  May be
 * called between any two frames; no graph is dropped.  CVO_HIP_ERR_INVALID: a null argument; the stage not set with
 * CVO_FE_PHOTO_GAIN; a gain that is not finite or outside [1/16, 15.99]. */
int cvo_fe_set_photometric_gain(cvo_fe_ctx *ctx, const float gain[3]);
/* Opens the lock of AUTO: the next frame with k >= min_count sets T.  CVO_HIP_ERR_INVALID without CVO_FE_PHOTO_AUTO. */
int cvo_fe_photometric_rearm(cvo_fe_ctx *ctx);
/* The record of the last collected frame.  CVO_HIP_ERR_INVALID: a null argument; the stage not set. */
int cvo_fe_get_photometric_frame(const cvo_fe_ctx *ctx, cvo_fe_photometric_frame *out);
/* The contract on any image by the kernels a frame runs, without a context: host arrays in and out.  `bgr` is width x
 * height x 3 in rows `stride` bytes apart and is not written; `out` is dense.  `vignette` is width x height in rows
 * `vignette_stride` bytes apart.  `gains_q12` (B, G, R; NULL: 4096) is read under CVO_FE_PHOTO_GAIN and clamped as the
 * contract says.  Under CVO_FE_PHOTO_AUTO the image is a first frame: with a target of all zero it closes the lock.
 * `frame_out` may be NULL.  CVO_HIP_ERR_INVALID: a null image; width or height outside [1, 8192]; a stride below the
 * row; what cvo_fe_check_photometric refuses; CVO_HIP_ERR_NODEVICE without such a device. */
int cvo_fe_photometric_image(int device, const uint8_t *bgr, int width, int height, size_t stride,
                             const cvo_fe_photometric *settings, const uint16_t *response, const uint16_t *vignette,
                             size_t vignette_stride, const uint32_t gains_q12[3], uint8_t *out,
                             cvo_fe_photometric_frame *frame_out);
/* A row of the response table from the inverse response of one channel (a row of DSO's pcalib.txt: the irradiance, in
 * [0, 255], of each of the 256 pixel values): out = min(65535, (uint32)(v * 256.0f + 0.5f)), each operation in float32.
 * CVO_HIP_ERR_INVALID: a null pointer; a value that is not finite or outside [0, 255].  Host only. */
int cvo_fe_response_table(const float inv[256], uint16_t out[256]);
/* The vignette's gains from its attenuations (the plane of DSO's vignette.png as 16-bit values, 65535 = none):
 * out = a ? min(65535, (4096 * 65535 + a / 2) / a) : 65535.  `out` may be `atten`.  CVO_HIP_ERR_INVALID: a null pointer
 * with n > 0.  Host only. */
int cvo_fe_vignette_gains(const uint16_t *atten, size_t n, uint16_t *out);
#ifdef __cplusplus
}
#endif
#endif
