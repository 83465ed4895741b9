"""RGB-D front end: Python mirror of the reference's
`cvo::pcd_generator` (ref cpp/rkhs_registration/include/pcd_generator.hpp:30-108)
over the C-ABI of include/cvo_frontend.h.  All image work runs as HIP kernels in
libcvo_hip.so; there is no CPU path (creating a generator without a gfx950
device raises).

    gen = PcdGenerator(width=640, height=480)
    xyz, feat = gen.create_pointcloud(bgr, depth, dataset_seq=1, feature_type=FEATURES_RGB)

A median filter on the depth plane in front of every later stage, filling small holes (the median contract of
include/cvo_frontend.h; frames of either kind):

    gen.set_depth_median(DepthMedian(radius=1, fill_min=5))

The gaps of a sparse depth plane -- between scan lines, in a warp's holes -- bridged linearly in inverse depth, directly
behind whatever fills the plane (the infill contract of include/cvo_frontend.h; frames of every kind):

    gen.set_depth_infill(DepthInfill(gap_x=2, gap_y=8, jump_rel=0.25))

Colour images in the sensor's own pixel format -- a Bayer mosaic, YUY2 / UYVY / NV12, grey, RGB, BGRA / RGBA -- unpacked
on the device in front of everything else (the unpack contract of include/cvo_frontend.h; frames of every kind):

    gen.set_pixel_format(PIXEL_BAYER_RGGB8)     # the images are then h x w bytes of mosaic

Depth as float32 / float16 in metres, as a network or a simulator produces it (the depth-format contract of
include/cvo_frontend.h), and frames whose images lie in device memory already (the device-input contract; any object with
`__cuda_array_interface__`, a torch tensor on ROCm among them -- the producer synchronised, or the generator on its stream):

    gen.set_depth_format(DEPTH_F32, unit=1.0)
    gen.submit_device(bgr_on_device, metres_on_device, dataset_seq=1)
    d_xyz, d_feat, n = gen.collect_device()     # from a tensor to the registration without touching host memory

A LiDAR scan in place of the depth image, projected into the colour camera on the device (the LiDAR contract of
include/cvo_frontend.h; KITTI: R, T from R_rect_00 * Tr_velo_to_cam):

    gen.set_lidar(Lidar(max_points=130000, R=R, T=T, splat=1, occl_rel=0.25, occl_rx=7, occl_ry=1))
    xyz, feat = gen.create_pointcloud_lidar(bgr, scan, dataset_seq=4)   # scan: n x 4 float32, x y z reflectance

A rectified stereo pair in place of the depth image (the stereo contract of include/cvo_frontend.h):

    gen = PcdGenerator(width=1241, height=376)
    gen.set_stereo(Stereo(baseline=0.54, max_disp=128))
    gen.set_stereo_paths(PATHS_8)       # optional: the four diagonal paths beside rows and columns (PATHS_4 otherwise)
    gen.set_stereo_speckle(Speckle(max_size=100, max_diff=16))   # optional: small islands of disparity give no point
    xyz, feat = gen.create_pointcloud_stereo(left, right, dataset_seq=4)

A RAW pair with its rig (the rig contract of include/cvo_frontend.h): both images are rectified on the device

    rig = stereo_rectify(StereoCalib(left=Lens(...), right=Lens(...), R=R, T=T), 752, 480, depth_scale=1000.0)
    gen.set_stereo(Stereo(max_disp=64))
    gen.set_stereo_rig(rig)
    xyz, feat = gen.create_pointcloud_stereo(raw_left, raw_right)

`bgr` is the h x w x 3 uint8 array an image decoder returns in OpenCV's channel
order (cv::imread: B, G, R) -- the reference passes exactly that to its "RGB"
conversions (ref src/pcd_generator.cpp:389-390), so channel 0 plays the role of R
there and here.  `depth` is h x w uint16 (TUM: 5000 units per metre).

Also here: the file side of the reference's drivers -- the association list and the
image pair of a frame (ref src/cvo_main.cpp:69-106).
"""
import ctypes as C
import os

import numpy as np

from . import capi

FEATURES_HSV, FEATURES_RGB = 0, 1
(STAGE_GRAY, STAGE_HSV, STAGE_MAP, STAGE_AG0, STAGE_AG1, STAGE_AG2, STAGE_THS, STAGE_DX0, STAGE_DY0,
 STAGE_EDGES, STAGE_RECT_BGR, STAGE_RECT_DEPTH, STAGE_RAW_DEPTH, STAGE_UNGATED_DEPTH, STAGE_GATE, STAGE_RIGHT_GRAY,
 STAGE_CENSUS_L, STAGE_CENSUS_R, STAGE_SGM_SUM, STAGE_DISPARITY, STAGE_STEREO, STAGE_RIGHT_BGR,
 STAGE_STEREO_VALID, STAGE_SPECKLE_SIZE, STAGE_UNFILTERED_DEPTH, STAGE_MEDIAN, STAGE_LIDAR_DEPTH,
 STAGE_LIDAR, STAGE_SPARSE_DEPTH, STAGE_INFILL, STAGE_INPUT_BGR, STAGE_INPUT_RIGHT_BGR) = range(32)
# of a frame under input binning (set_input_binning): the input-size images the bin read
STAGE_FULL_BGR, STAGE_FULL_RIGHT_BGR, STAGE_FULL_DEPTH = 32, 33, 34
GATE_MASKED, GATE_RANGE, GATE_JUMP = 1, 2, 4   # the flags of STAGE_GATE
STEREO_UNIQUE, STEREO_LR, STEREO_MIN, STEREO_DEPTH, STEREO_OUTSIDE, STEREO_SPECKLE = 1, 2, 4, 8, 16, 32   # the flags of STAGE_STEREO
MEDIAN_CHANGED, MEDIAN_FILLED = 1, 2   # the values of STAGE_MEDIAN
LIDAR_HIT, LIDAR_OCCLUDED = 1, 2       # the bits of STAGE_LIDAR
SWEEP_TIME_F32, SWEEP_TIME_U32, SWEEP_AZIMUTH = 1, 2, 3   # the modes of a LidarSweep
INFILL_ROW, INFILL_COL, INFILL_JUMP = 1, 2, 4   # the values of STAGE_INFILL
# pixel formats of the colour images (set_pixel_format; the unpack contract of include/cvo_frontend.h).  Bayer: the four
# letters are the colours of pixels (0,0) (1,0) / (0,1) (1,1) -- not OpenCV's names
(PIXEL_BGR8, PIXEL_RGB8, PIXEL_BGRA8, PIXEL_RGBA8, PIXEL_GREY8, PIXEL_YUY2, PIXEL_UYVY, PIXEL_NV12, PIXEL_BAYER_RGGB8,
 PIXEL_BAYER_BGGR8, PIXEL_BAYER_GRBG8, PIXEL_BAYER_GBRG8) = range(12)
# formats of the depth images (set_depth_format; the depth-format contract of include/cvo_frontend.h): uint16 in the
# camera's own units (a new object's), or float32 / float16 in `unit` metres
DEPTH_U16, DEPTH_F32, DEPTH_F16 = 0, 1, 2
_DEPTH_DTYPES = {DEPTH_U16: np.uint16, DEPTH_F32: np.float32, DEPTH_F16: np.float16}
# path masks of the stereo matcher (set_stereo_paths): bits 0-3 rows and columns, bits 4-7 the diagonals
PATHS_4, PATHS_8 = 0x0F, 0xFF
# modes of the selector (set_select_mode): by the image alone (the reference; a new object's), or among the pixels
# that have a depth (the selection contract of include/cvo_frontend.h)
SELECT_IMAGE, SELECT_DEPTH = 0, 1

SYMBOLS = ("cvo_fe_create", "cvo_fe_destroy", "cvo_fe_last_error", "cvo_fe_set_num_want",
           "cvo_fe_create_pointcloud", "cvo_fe_submit", "cvo_fe_collect", "cvo_fe_collect_device", "cvo_fe_set_device_output", "cvo_fe_host_buffers", "cvo_fe_get_info", "cvo_fe_read_stage", "cvo_fe_random_pattern",
           "cvo_fe_camera", "cvo_fe_set_camera", "cvo_fe_get_camera", "cvo_fe_rectify_map",
           "cvo_fe_set_depth_camera", "cvo_fe_get_depth_camera", "cvo_fe_depth_rays",
           "cvo_fe_check_depth_camera", "cvo_fe_set_depth_gate", "cvo_fe_get_depth_gate", "cvo_fe_check_depth_gate",
           "cvo_fe_set_mask", "cvo_fe_check_stereo", "cvo_fe_set_stereo", "cvo_fe_get_stereo", "cvo_fe_submit_stereo",
           "cvo_fe_create_pointcloud_stereo", "cvo_fe_stereo_depth_table", "cvo_fe_set_stereo_rig", "cvo_fe_get_stereo_rig",
           "cvo_fe_check_stereo_rig", "cvo_fe_stereo_rectify", "cvo_fe_stereo_rig_map", "cvo_fe_check_stereo_paths",
           "cvo_fe_set_stereo_paths", "cvo_fe_get_stereo_paths", "cvo_fe_check_speckle", "cvo_fe_set_stereo_speckle",
           "cvo_fe_get_stereo_speckle", "cvo_fe_filter_speckles", "cvo_fe_check_select_mode", "cvo_fe_set_select_mode",
           "cvo_fe_get_select_mode", "cvo_fe_check_depth_median", "cvo_fe_set_depth_median", "cvo_fe_get_depth_median",
           "cvo_fe_median_plane", "cvo_fe_check_depth_infill", "cvo_fe_set_depth_infill", "cvo_fe_get_depth_infill",
           "cvo_fe_infill_plane", "cvo_fe_check_lidar", "cvo_fe_set_lidar", "cvo_fe_get_lidar", "cvo_fe_submit_lidar",
           "cvo_fe_create_pointcloud_lidar", "cvo_fe_project_points", "cvo_fe_check_pixel_format", "cvo_fe_pixel_layout",
           "cvo_fe_set_pixel_format", "cvo_fe_get_pixel_format", "cvo_fe_unpack_image", "cvo_fe_check_lidar_sweep",
           "cvo_fe_set_lidar_sweep", "cvo_fe_get_lidar_sweep", "cvo_fe_set_lidar_motion", "cvo_fe_get_lidar_motion",
           "cvo_fe_lidar_twist", "cvo_fe_project_points_sweep", "cvo_fe_check_depth_format", "cvo_fe_set_depth_format",
           "cvo_fe_get_depth_format", "cvo_fe_convert_depth", "cvo_fe_submit_device", "cvo_fe_submit_stereo_device",
           "cvo_fe_check_binning", "cvo_fe_set_input_binning", "cvo_fe_get_input_binning", "cvo_fe_bin_camera",
           "cvo_fe_bin_stereo_rig", "cvo_fe_bin_image", "cvo_fe_bin_depth",
           "cvo_fe_check_photometric", "cvo_fe_set_photometric", "cvo_fe_get_photometric", "cvo_fe_set_photometric_gain",
           "cvo_fe_photometric_rearm", "cvo_fe_get_photometric_frame", "cvo_fe_photometric_image",
           "cvo_fe_response_table", "cvo_fe_vignette_gains")
# the flags of Photometric, and of PhotometricFrame
PHOTO_RESPONSE, PHOTO_VIGNETTE, PHOTO_GAIN, PHOTO_AUTO = 1, 2, 4, 8
PHOTO_FALLBACK, PHOTO_LOCKED = 1, 2


class Info(C.Structure):
    _fields_ = [("num_selected", C.c_int32), ("pot_used", C.c_int32), ("reselected", C.c_int32),
                ("canny_used", C.c_int32), ("num_points", C.c_int32), ("pad_", C.c_int32)]


class _Settings(C.Structure):
    """What the structures a caller hands to a setter share, derived from `_fields_`; a `pad_` is shown nowhere."""

    def astuple(self):
        vals = (getattr(self, name) for name, _ in self._fields_ if name != "pad_")
        return tuple(tuple(v) if isinstance(v, C.Array) else v for v in vals)

    def __eq__(self, other):
        return isinstance(other, type(self)) and bytes(self) == bytes(other)

    __hash__ = None

    def __repr__(self):
        names = (name for name, _ in self._fields_ if name != "pad_")
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % nv for nv in zip(names, self.astuple())))


class CameraModel(_Settings):
    """cvo_fe_camera_model: a caller's camera in place of the table row of `dataset_seq`.
    `dist` is (k1, k2, p1, p2, k3) in OpenCV's / TUM's order; all zero: an ideal pinhole."""
    _fields_ = [("depth_scale", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("dist", C.c_float * 5)]

    def __init__(self, depth_scale=1000.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
        if len(dist) != 5:
            raise ValueError("dist holds k1, k2, p1, p2, k3")
        super().__init__(depth_scale, fx, fy, cx, cy, (C.c_float * 5)(*dist))


class DepthCamera(_Settings):
    """cvo_fe_depth_camera: a depth camera of its own -- the size of its image, its pinhole and lens,
    and where it sits: p_colour = R p_depth + T (R row-major, T in metres).  `min_range` / `max_range`
    in metres along its axis; <= 0: no limit on that side."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth_scale", C.c_float), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("dist", C.c_float * 5),
                ("R", C.c_float * 9), ("T", C.c_float * 3), ("min_range", C.c_float), ("max_range", C.c_float)]

    def __init__(self, width=0, height=0, depth_scale=1000.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0,
                 dist=(0.0, 0.0, 0.0, 0.0, 0.0), R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), T=(0.0, 0.0, 0.0),
                 min_range=0.0, max_range=0.0):
        R = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
        if len(dist) != 5 or len(R) != 9 or len(T) != 3:
            raise ValueError("dist holds k1, k2, p1, p2, k3; R is 3 x 3; T holds 3 numbers")
        super().__init__(int(width), int(height), depth_scale, fx, fy, cx, cy, (C.c_float * 5)(*dist),
                         (C.c_float * 9)(*R), (C.c_float * 3)(*T), min_range, max_range)


class DepthGate(_Settings):
    """cvo_fe_depth_gate: which pixels with a depth keep it (the gate contract of include/cvo_frontend.h).
    `min_range` / `max_range` in metres along the colour camera's axis, <= 0: no limit on that side;
    `jump_rel`: the relative depth jump between neighbours that marks a discontinuity, 0: no jump test;
    `grow` 0..3: the pixels around a marked one that go with it; `hole_border` 1: a pixel beside one
    without depth is marked too."""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("jump_rel", C.c_float), ("grow", C.c_int32),
                ("hole_border", C.c_int32), ("pad_", C.c_int32)]

    def __init__(self, min_range=0.0, max_range=0.0, jump_rel=0.0, grow=0, hole_border=0, pad_=0):
        super().__init__(min_range, max_range, jump_rel, int(grow), int(hole_border), int(pad_))


class Stereo(_Settings):
    """cvo_fe_stereo: a rectified stereo pair in place of the depth image (the stereo contract of
    include/cvo_frontend.h).  `baseline` in metres; disparities 0 .. `max_disp` - 1 are searched (a multiple of 8
    in [8, 128]); a pixel whose disparity is below `min_disp` gets no depth; `p1` <= `p2` <= 255: the penalties of
    the semi-global paths; `uniqueness` 0..99 per cent, 0: no uniqueness test; `lr_max` 0..8: the largest
    left-right difference kept, -1: no left-right test."""
    _fields_ = [("baseline", C.c_float), ("max_disp", C.c_int32), ("min_disp", C.c_int32), ("p1", C.c_int32),
                ("p2", C.c_int32), ("uniqueness", C.c_int32), ("lr_max", C.c_int32), ("pad_", C.c_int32)]

    def __init__(self, baseline=0.54, max_disp=64, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1, pad_=0):
        super().__init__(baseline, int(max_disp), int(min_disp), int(p1), int(p2), int(uniqueness), int(lr_max), int(pad_))


class Speckle(_Settings):
    """cvo_fe_speckle: the speckle filter on the matcher's disparities (the speckle contract of include/cvo_frontend.h).
    Components of 4-neighbours whose values differ by `max_diff` at the most (units of the plane: 1/16 pixel of a
    disparity) and that hold `max_size` pixels at the most lose their disparity."""
    _fields_ = [("max_size", C.c_int32), ("max_diff", C.c_int32)]

    def __init__(self, max_size=100, max_diff=16):
        super().__init__(int(max_size), int(max_diff))


class DepthMedian(_Settings):
    """cvo_fe_depth_median: the median stage on the depth plane, in front of the gate (the median contract of
    include/cvo_frontend.h).  `radius` 1: a 3 x 3 window, 2: 5 x 5; a pixel with a depth takes the lower median of its
    window's depths.  `fill_min` 0: a pixel without depth stays without; k >= 1: it takes that median when at least k
    pixels of its window have a depth."""
    _fields_ = [("radius", C.c_int32), ("fill_min", C.c_int32), ("pad_", C.c_int32)]

    def __init__(self, radius=1, fill_min=0, pad_=0):
        super().__init__(int(radius), int(fill_min), int(pad_))


class Binning(_Settings):
    """cvo_fe_binning: input binning (the binning contract of include/cvo_frontend.h).  The images a frame takes are
    `factor` (2, 3 or 4) times the generator's size each way and are binned to it on the device in front of everything
    else: box means of the colour bytes, and the lower median of a block's depths where at least `depth_min` (1 ..
    factor^2) of its pixels have one.  EVERY CAMERA OF THE GENERATOR THEN DESCRIBES THE BINNED IMAGE: bin_camera(),
    bin_stereo_rig()."""
    _fields_ = [("factor", C.c_int32), ("depth_min", C.c_int32), ("pad_", C.c_int32)]

    def __init__(self, factor=2, depth_min=1, pad_=0):
        super().__init__(int(factor), int(depth_min), int(pad_))


class Photometric(_Settings):
    """cvo_fe_photometric: the photometric stage (the photometric contract of include/cvo_frontend.h).  `flags`: an OR
    of PHOTO_RESPONSE, PHOTO_VIGNETTE (a table of that kind is handed over beside the settings), PHOTO_GAIN (the
    caller's gain per frame and channel: set_photometric_gain) and PHOTO_AUTO (the gain estimated on the device from
    the pixels whose three input bytes lie in [lo, hi], at least `min_count` of them; `target` B G R in Q8, all zero:
    the first such frame's own statistic; `per_channel` 0: one gain for all channels).  `gain_min`, `gain_max`: Q12."""
    _fields_ = [("flags", C.c_uint32), ("lo", C.c_int32), ("hi", C.c_int32), ("min_count", C.c_int32),
                ("per_channel", C.c_int32), ("target", C.c_uint32 * 3), ("gain_min", C.c_int32), ("gain_max", C.c_int32),
                ("pad_", C.c_int32)]

    def __init__(self, flags=PHOTO_GAIN, lo=8, hi=247, min_count=1, per_channel=0, target=(0, 0, 0), gain_min=256,
                 gain_max=65535, pad_=0):
        super().__init__(int(flags), int(lo), int(hi), int(min_count), int(per_channel),
                         (C.c_uint32 * 3)(*(int(t) for t in target)), int(gain_min), int(gain_max), int(pad_))


class PhotometricFrame(_Settings):
    """cvo_fe_photometric_frame: what the stage did to a frame: the gains (Q12) it was corrected with, PHOTO_FALLBACK /
    PHOTO_LOCKED, and under PHOTO_AUTO the count k, the sums M and the target T in force behind the frame."""
    _fields_ = [("gain", C.c_uint32 * 3), ("flags", C.c_uint32), ("count", C.c_uint64), ("sum", C.c_uint64 * 3),
                ("target", C.c_uint32 * 3), ("pad_", C.c_uint32)]


class DepthInfill(_Settings):
    """cvo_fe_depth_infill: the infill stage on the depth plane, directly behind whatever fills it and in front of the
    median stage (the infill contract of include/cvo_frontend.h).  A run of at most `gap_x` (0..15) pixels without depth
    in a row, then of at most `gap_y` (0..31) in a column, that has a depth at both ends inside the image takes the
    values linear in INVERSE depth between them; 0: no pass along that axis.  `jump_rel` 0: every such run is bridged;
    > 0: not one whose ends differ by more than this relative step."""
    _fields_ = [("gap_x", C.c_int32), ("gap_y", C.c_int32), ("jump_rel", C.c_float), ("pad_", C.c_int32)]

    def __init__(self, gap_x=0, gap_y=0, jump_rel=0.0, pad_=0):
        super().__init__(int(gap_x), int(gap_y), float(jump_rel), int(pad_))


class Lidar(_Settings):
    """cvo_fe_lidar: a LiDAR scan in place of the depth image (the LiDAR contract of include/cvo_frontend.h).
    `max_points`: the capacity of a scan, 1 .. 2^21 (a frame copies a staging of this size); `splat` 0..3: a point writes
    the (2*splat+1)^2 pixels around its nearest pixel; p_colour = R p_lidar + T (R row-major, T in metres);
    `min_range` / `max_range` in metres along the colour camera's axis, <= 0: no limit on that side; `occl_rel` 0: no
    occlusion test, > 0: a pixel farther than (1 + occl_rel) times the nearest depth of its window of half-widths
    (`occl_rx`, `occl_ry`), 0..7 each, is dropped."""
    _fields_ = [("max_points", C.c_int32), ("splat", C.c_int32), ("R", C.c_float * 9), ("T", C.c_float * 3),
                ("min_range", C.c_float), ("max_range", C.c_float), ("occl_rel", C.c_float), ("occl_rx", C.c_int32),
                ("occl_ry", C.c_int32), ("pad_", C.c_int32)]

    def __init__(self, max_points=131072, splat=0, R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), T=(0.0, 0.0, 0.0),
                 min_range=0.0, max_range=0.0, occl_rel=0.0, occl_rx=0, occl_ry=0, pad_=0):
        R = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
        if len(R) != 9 or len(T) != 3:
            raise ValueError("R is 3 x 3; T holds 3 numbers")
        super().__init__(int(max_points), int(splat), (C.c_float * 9)(*R), (C.c_float * 3)(*T), min_range, max_range,
                         occl_rel, int(occl_rx), int(occl_ry), int(pad_))


class LidarSweep(_Settings):
    """cvo_fe_lidar_sweep: motion compensation of a spinning scan (the sweep contract of include/cvo_frontend.h).
    `mode`: where a point's phase, the fraction of the sweep at which it was measured, comes from -- SWEEP_TIME_F32 /
    SWEEP_TIME_U32: the float32 / uint32 at byte `time_offset` of its record (a multiple of 4, >= 12), as
    (t - `time_origin`) * `time_scale` (`time_origin` under SWEEP_TIME_F32 only), clamped to [0, 1]; SWEEP_AZIMUTH: its
    azimuth, `direction` (+1 or -1) * atan2(y, x) / 2 pi + `phase0` (in [0, 1)), wrapped.  `s_ref` in [0, 1]: the phase
    at which the colour image is exposed."""
    _fields_ = [("mode", C.c_int32), ("time_offset", C.c_int32), ("time_origin", C.c_float), ("time_scale", C.c_float),
                ("phase0", C.c_float), ("direction", C.c_int32), ("s_ref", C.c_float), ("pad_", C.c_int32)]

    def __init__(self, mode=SWEEP_AZIMUTH, time_offset=0, time_origin=0.0, time_scale=0.0, phase0=0.0, direction=0,
                 s_ref=0.0, pad_=0):
        super().__init__(int(mode), int(time_offset), time_origin, time_scale, phase0, int(direction), s_ref, int(pad_))


class Lens(_Settings):
    """cvo_fe_lens: one camera of a stereo rig, its pinhole and its lens (k1, k2, p1, p2, k3)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("dist", C.c_float * 5)]

    def __init__(self, fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
        if len(dist) != 5:
            raise ValueError("dist holds k1, k2, p1, p2, k3")
        super().__init__(fx, fy, cx, cy, (C.c_float * 5)(*dist))

    def astuple(self):
        return (self.fx, self.fy, self.cx, self.cy, tuple(self.dist))


def _lens(v):
    return v if isinstance(v, Lens) else Lens(*v)


def _floats(v, n, what):
    v = [float(x) for x in np.asarray(v, np.float64).reshape(-1)]
    if len(v) != n:
        raise ValueError(what)
    return (C.c_float * n)(*v)


_EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class StereoCalib(_Settings):
    """cvo_fe_stereo_calib: what a stereo calibration tool gives -- the two cameras (Lens, or its tuple) and where
    the right one sits: p_right = R p_left + T (R 3 x 3 row-major, T in metres).  stereo_rectify() makes the rig."""
    _fields_ = [("left", Lens), ("right", Lens), ("R", C.c_float * 9), ("T", C.c_float * 3)]

    def __init__(self, left=(), right=(), R=_EYE, T=(-0.1, 0.0, 0.0)):
        super().__init__(_lens(left), _lens(right), _floats(R, 9, "R is 3 x 3"), _floats(T, 3, "T holds 3 numbers"))

    def astuple(self):
        return (self.left.astuple(), self.right.astuple(), tuple(self.R), tuple(self.T))


class StereoRig(_Settings):
    """cvo_fe_stereo_rig: a raw stereo pair's rig (the rig contract of include/cvo_frontend.h) -- the two cameras,
    the rectifying rotations (p_rect = R_k p_k, row-major), the common rectified pinhole, the `baseline` in metres
    and `depth_scale`, the units per metre of the depth plane.  From stereo_rectify(), or filled from published
    rectification data (KITTI raw: R_rect_0x, P_rect_0x)."""
    _fields_ = [("left", Lens), ("right", Lens), ("R_left", C.c_float * 9), ("R_right", C.c_float * 9), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("baseline", C.c_float), ("depth_scale", C.c_float)]

    def __init__(self, left=(), right=(), R_left=_EYE, R_right=_EYE, fx=1.0, fy=1.0, cx=0.0, cy=0.0, baseline=0.1,
                 depth_scale=1000.0):
        super().__init__(_lens(left), _lens(right), _floats(R_left, 9, "R_left is 3 x 3"),
                         _floats(R_right, 9, "R_right is 3 x 3"), fx, fy, cx, cy, baseline, depth_scale)

    def astuple(self):
        return (self.left.astuple(), self.right.astuple(), tuple(self.R_left), tuple(self.R_right), self.fx, self.fy,
                self.cx, self.cy, self.baseline, self.depth_scale)


# The published calibrations of the TUM RGB-D sequences (fx fy cx cy, d0..d4; depth 5000 per metre).
# The reference's table (camera(1..3)) holds the same intrinsics without the distortion.  The entries are
# shared by every user of the module: read them, hand them to set_camera() (which copies), and make a model of
# your own -- CameraModel(*TUM_CAMERAS["fr1"].astuple()) -- before changing a member.
TUM_CAMERAS = {
    "fr1": CameraModel(5000.0, 517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)),
    "fr2": CameraModel(5000.0, 520.9, 521.0, 325.1, 249.7, (0.2312, -0.7849, -0.0033, -0.0001, 0.9172)),
    "fr3": CameraModel(5000.0, 535.4, 539.2, 320.1, 247.6),
}


_BOUND = False


def lib():
    """libcvo_hip.so with the cvo_fe_* prototypes set (raises if it is not built)."""
    global _BOUND
    L = capi.lib()
    if not _BOUND:
        vp, u8p, u16p, fp = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_float)
        L.cvo_fe_create.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.cvo_fe_destroy.argtypes = [vp]
        L.cvo_fe_last_error.argtypes = [vp]
        L.cvo_fe_last_error.restype = C.c_char_p
        L.cvo_fe_set_num_want.argtypes = [vp, C.c_int]
        L.cvo_fe_create_pointcloud.argtypes = [vp, u8p, C.c_size_t, u16p, C.c_size_t, C.c_int, C.c_int, fp, fp,
                                               C.c_int, C.POINTER(C.c_int)]
        L.cvo_fe_submit.argtypes = [vp, u8p, C.c_size_t, u16p, C.c_size_t, C.c_int, C.c_int]
        L.cvo_fe_collect.argtypes = [vp, fp, fp, C.c_int, C.POINTER(C.c_int)]
        L.cvo_fe_collect_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
        L.cvo_fe_set_device_output.argtypes = [vp, C.c_int]
        L.cvo_fe_host_buffers.argtypes = [vp, C.POINTER(u8p), C.POINTER(u16p)]
        L.cvo_fe_get_info.argtypes = [vp, C.POINTER(Info)]
        L.cvo_fe_read_stage.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.cvo_fe_random_pattern.argtypes = [C.c_int, u8p]
        L.cvo_fe_camera.argtypes = [C.c_int, fp]
        # the settings that are structures: cvo_fe_set_<name>, cvo_fe_get_<name> and, but for the camera, cvo_fe_check_<check>
        for name, cls, check in (("camera", CameraModel, None), ("depth_camera", DepthCamera, "depth_camera"),
                                 ("depth_gate", DepthGate, "depth_gate"), ("stereo", Stereo, "stereo"),
                                 ("stereo_speckle", Speckle, "speckle"), ("depth_median", DepthMedian, "depth_median"),
                                 ("depth_infill", DepthInfill, "depth_infill"), ("lidar", Lidar, "lidar"),
                                 ("lidar_sweep", LidarSweep, "lidar_sweep"), ("stereo_rig", StereoRig, "stereo_rig")):
            getattr(L, "cvo_fe_set_" + name).argtypes = [vp, C.POINTER(cls)]
            getattr(L, "cvo_fe_get_" + name).argtypes = [vp, C.POINTER(cls), C.POINTER(C.c_int)]
            if check:
                getattr(L, "cvo_fe_check_" + check).argtypes = [C.POINTER(cls)]
        L.cvo_fe_rectify_map.argtypes = [C.POINTER(CameraModel), C.c_int, C.c_int, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32)]
        L.cvo_fe_depth_rays.argtypes = [C.POINTER(DepthCamera), fp, fp]
        L.cvo_fe_set_mask.argtypes = [vp, u8p, C.c_size_t]
        L.cvo_fe_submit_stereo.argtypes = [vp, u8p, C.c_size_t, u8p, C.c_size_t, C.c_int, C.c_int]
        L.cvo_fe_create_pointcloud_stereo.argtypes = [vp, u8p, C.c_size_t, u8p, C.c_size_t, C.c_int, C.c_int, fp, fp,
                                                      C.c_int, C.POINTER(C.c_int)]
        L.cvo_fe_check_stereo_paths.argtypes = [C.c_uint32]
        L.cvo_fe_set_stereo_paths.argtypes = [vp, C.c_uint32]
        L.cvo_fe_get_stereo_paths.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.cvo_fe_check_select_mode.argtypes = [C.c_int]
        L.cvo_fe_set_select_mode.argtypes = [vp, C.c_int]
        L.cvo_fe_get_select_mode.argtypes = [vp, C.POINTER(C.c_int)]
        L.cvo_fe_filter_speckles.argtypes = [C.c_int, u16p, C.c_size_t, C.c_int, C.c_int, C.POINTER(Speckle),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.cvo_fe_infill_plane.argtypes = [C.c_int, u16p, C.c_size_t, C.c_int, C.c_int, C.POINTER(DepthInfill), u8p,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cvo_fe_median_plane.argtypes = [C.c_int, u16p, C.c_size_t, C.c_int, C.c_int, C.POINTER(DepthMedian), u8p,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cvo_fe_check_pixel_format.argtypes = [C.c_int, C.c_int, C.c_int]
        L.cvo_fe_pixel_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.cvo_fe_set_pixel_format.argtypes = [vp, C.c_int]
        L.cvo_fe_get_pixel_format.argtypes = [vp, C.POINTER(C.c_int)]
        L.cvo_fe_unpack_image.argtypes = [C.c_int, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, u8p]
        L.cvo_fe_submit_lidar.argtypes = [vp, u8p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
        L.cvo_fe_create_pointcloud_lidar.argtypes = [vp, u8p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                                     fp, fp, C.c_int, C.POINTER(C.c_int)]
        L.cvo_fe_project_points.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Lidar), fp, C.c_int, C.c_int,
                                            u16p, u16p, u8p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cvo_fe_set_lidar_motion.argtypes = [vp, fp]
        L.cvo_fe_get_lidar_motion.argtypes = [vp, fp]
        L.cvo_fe_lidar_twist.argtypes = [fp, C.POINTER(Lidar), C.c_float, fp]
        L.cvo_fe_project_points_sweep.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Lidar), fp, C.c_int,
                                                  C.c_int, u16p, u16p, u8p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                  C.POINTER(LidarSweep), fp, fp, fp]
        L.cvo_fe_stereo_depth_table.argtypes = [C.POINTER(Stereo), C.c_float, C.c_float, u16p]
        L.cvo_fe_stereo_rectify.argtypes = [C.POINTER(StereoCalib), C.c_int, C.c_int, C.POINTER(StereoRig), C.c_float]
        L.cvo_fe_stereo_rig_map.argtypes = [C.POINTER(StereoRig), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32)]
        L.cvo_fe_check_depth_format.argtypes = [C.c_int, C.c_float]
        L.cvo_fe_set_depth_format.argtypes = [vp, C.c_int, C.c_float]
        L.cvo_fe_get_depth_format.argtypes = [vp, C.POINTER(C.c_int), fp]
        L.cvo_fe_convert_depth.argtypes = [C.c_int, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, u16p]
        L.cvo_fe_submit_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int]
        L.cvo_fe_submit_stereo_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int]
        L.cvo_fe_check_binning.argtypes = [C.POINTER(Binning), C.c_int, C.c_int]
        L.cvo_fe_set_input_binning.argtypes = [vp, C.POINTER(Binning)]
        L.cvo_fe_get_input_binning.argtypes = [vp, C.POINTER(Binning), C.POINTER(C.c_int)]
        L.cvo_fe_bin_camera.argtypes = [C.POINTER(CameraModel), C.c_int, C.POINTER(CameraModel)]
        L.cvo_fe_bin_stereo_rig.argtypes = [C.POINTER(StereoRig), C.c_int, C.POINTER(StereoRig)]
        L.cvo_fe_bin_image.argtypes = [C.c_int, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, u8p]
        L.cvo_fe_bin_depth.argtypes = [C.c_int, u16p, C.c_size_t, C.c_int, C.c_int, C.POINTER(Binning), u16p,
                                       C.POINTER(C.c_int)]
        pp, fp = C.POINTER(Photometric), C.POINTER(C.c_float)
        L.cvo_fe_check_photometric.argtypes = [pp, C.c_int, C.c_int]
        L.cvo_fe_set_photometric.argtypes = [vp, pp, u16p, u16p, C.c_size_t]
        L.cvo_fe_get_photometric.argtypes = [vp, pp, C.POINTER(C.c_int)]
        L.cvo_fe_set_photometric_gain.argtypes = [vp, fp]
        L.cvo_fe_photometric_rearm.argtypes = [vp]
        L.cvo_fe_get_photometric_frame.argtypes = [vp, C.POINTER(PhotometricFrame)]
        L.cvo_fe_photometric_image.argtypes = [C.c_int, u8p, C.c_int, C.c_int, C.c_size_t, pp, u16p, u16p, C.c_size_t,
                                               C.POINTER(C.c_uint32), u8p, C.POINTER(PhotometricFrame)]
        L.cvo_fe_response_table.argtypes = [fp, u16p]
        L.cvo_fe_vignette_gains.argtypes = [u16p, C.c_size_t, u16p]
        for name in SYMBOLS:
            if name != "cvo_fe_last_error":
                getattr(L, name).restype = C.c_int
        _BOUND = True
    return L


def random_pattern(n):
    """The selector's random bytes (ref thirdparty/PixelSelector2.cpp:35-37)."""
    out = np.empty(n, np.uint8)
    capi.check(lib().cvo_fe_random_pattern(n, out.ctypes.data_as(C.POINTER(C.c_uint8))), what="random_pattern")
    return out


def camera(dataset_seq):
    """{scaling_factor, fx, fy, cx, cy} of the reference's camera table
    (ref src/pcd_generator.cpp:241-295)."""
    cam = np.zeros(5, np.float32)
    capi.check(lib().cvo_fe_camera(int(dataset_seq), cam.ctypes.data_as(C.POINTER(C.c_float))), what="camera")
    return dict(zip(("scaling_factor", "fx", "fy", "cx", "cy"), (float(v) for v in cam)))


_table_row = camera   # (run_frames has an argument of that name)


def rectify_map(model, width, height):
    """The map of the rectification contract (include/cvo_frontend.h) for a width x height image:
    (qu, qv), int32 height x width, where each output pixel looks in the input, in 1/32 pixel.
    Host only."""
    qu = np.empty((int(height), int(width)), np.int32)
    qv = np.empty_like(qu)
    i32p = C.POINTER(C.c_int32)
    capi.check(lib().cvo_fe_rectify_map(C.byref(model), int(width), int(height), qu.ctypes.data_as(i32p),
                                        qv.ctypes.data_as(i32p)), what="rectify_map")
    return qu, qv


def depth_rays(rig):
    """The ray table of the registration contract (include/cvo_frontend.h) for a DepthCamera:
    (xn, yn), float32 (height+1) x (width+1), the rays through the corners of the depth pixels; NaN where
    the lens cannot be inverted.  Host only."""
    xn = np.empty((int(rig.height) + 1, int(rig.width) + 1), np.float32)
    yn = np.empty_like(xn)
    fp = C.POINTER(C.c_float)
    capi.check(lib().cvo_fe_depth_rays(C.byref(rig), xn.ctypes.data_as(fp), yn.ctypes.data_as(fp)), what="depth_rays")
    return xn, yn


def check_depth_camera(rig):
    """True for a DepthCamera set_depth_camera() accepts (cvo_fe_check_depth_camera).  Host only."""
    return lib().cvo_fe_check_depth_camera(C.byref(rig)) == 0


def check_depth_gate(gate):
    """True for a DepthGate set_depth_gate() accepts (cvo_fe_check_depth_gate).  Host only."""
    return lib().cvo_fe_check_depth_gate(C.byref(gate)) == 0


def check_stereo(stereo):
    """True for a Stereo set_stereo() accepts (cvo_fe_check_stereo).  Host only."""
    return lib().cvo_fe_check_stereo(C.byref(stereo)) == 0


def check_stereo_paths(mask):
    """True for a path mask set_stereo_paths() accepts (cvo_fe_check_stereo_paths): 1 <= mask <= 0xFF.  Host only."""
    mask = int(mask)
    return 0 <= mask <= 0xFFFFFFFF and lib().cvo_fe_check_stereo_paths(mask) == 0


def check_select_mode(mode):
    """True for a mode set_select_mode() accepts (cvo_fe_check_select_mode): SELECT_IMAGE or SELECT_DEPTH.  Host only."""
    mode = int(mode)
    return -2 ** 31 <= mode < 2 ** 31 and lib().cvo_fe_check_select_mode(mode) == 0


def check_speckle(speckle):
    """True for a Speckle set_stereo_speckle() accepts (cvo_fe_check_speckle): max_size in [1, 2^26], max_diff in
    [0, 65535]; None is refused.  Host only."""
    if speckle is None:
        return lib().cvo_fe_check_speckle(None) == 0
    ok = all(-2 ** 31 <= int(v) < 2 ** 31 for v in (speckle.max_size, speckle.max_diff))
    return ok and lib().cvo_fe_check_speckle(C.byref(speckle)) == 0


def filter_speckles(plane, speckle, device=0):
    """The speckle filter on any h x w uint16 plane with 0 = none (cvo_fe_filter_speckles: the kernels a stereo frame
    runs, without a generator).  Returns (the filtered plane, SIZE as h x w uint32, the number of pixels zeroed); the
    argument is left as it is."""
    plane = np.array(plane, np.uint16, order="C")
    if plane.ndim != 2:
        raise ValueError("expected an h x w uint16 plane")
    h, w = plane.shape
    sizes = np.empty((h, w), np.uint32)
    removed = C.c_int(0)
    capi.check(lib().cvo_fe_filter_speckles(int(device), plane.ctypes.data_as(C.POINTER(C.c_uint16)), w * 2, w, h,
                                            None if speckle is None else C.byref(speckle),
                                            sizes.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(removed)),
               what="filter_speckles")
    return plane, sizes, removed.value


def check_depth_median(median):
    """True for a DepthMedian set_depth_median() accepts (cvo_fe_check_depth_median): radius 1 or 2, fill_min in
    [0, (2*radius+1)^2 - 1], pad_ 0; None is refused.  Host only."""
    if median is None:
        return lib().cvo_fe_check_depth_median(None) == 0
    return lib().cvo_fe_check_depth_median(C.byref(median)) == 0


def median_plane(plane, median, device=0):
    """The median stage on any h x w uint16 plane with 0 = none (cvo_fe_median_plane: the kernel a frame runs, without
    a generator).  Returns (the filtered plane, the flags as h x w uint8 of MEDIAN_CHANGED / MEDIAN_FILLED, the number
    of pixels changed, the number filled); the argument is left as it is."""
    plane = np.array(plane, np.uint16, order="C")
    if plane.ndim != 2:
        raise ValueError("expected an h x w uint16 plane")
    h, w = plane.shape
    flags = np.empty((h, w), np.uint8)
    changed, filled = C.c_int(0), C.c_int(0)
    capi.check(lib().cvo_fe_median_plane(int(device), plane.ctypes.data_as(C.POINTER(C.c_uint16)), w * 2, w, h,
                                         None if median is None else C.byref(median),
                                         flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(changed), C.byref(filled)),
               what="median_plane")
    return plane, flags, changed.value, filled.value


def check_depth_infill(infill):
    """True for a DepthInfill set_depth_infill() accepts (cvo_fe_check_depth_infill): gap_x in [0, 15], gap_y in [0, 31],
    jump_rel finite and >= 0, pad_ 0; None is refused.  Host only."""
    if infill is None:
        return lib().cvo_fe_check_depth_infill(None) == 0
    return lib().cvo_fe_check_depth_infill(C.byref(infill)) == 0


def infill_plane(plane, infill, device=0, stride=None):
    """The infill stage on any h x w uint16 plane with 0 = none (cvo_fe_infill_plane: the kernel a frame runs, without
    a generator).  Returns (F, the flags as h x w uint8 of INFILL_ROW / INFILL_COL / INFILL_JUMP, the number of pixels
    the row pass filled, the number the column pass filled); the argument is left as it is.  `stride`: the plane is
    handed over in rows that many uint16 apart (at least w), the cells between them holding 65535; they come back as
    they went."""
    src = np.asarray(plane, np.uint16)
    if src.ndim != 2:
        raise ValueError("expected an h x w uint16 plane")
    h, w = src.shape
    pitch = w if stride is None else int(stride)
    if pitch < w:
        raise ValueError("stride below the plane's width")
    buf = np.full((h, pitch), 65535, np.uint16)
    buf[:, :w] = src
    flags = np.empty((h, w), np.uint8)
    rows, cols = C.c_int(0), C.c_int(0)
    capi.check(lib().cvo_fe_infill_plane(int(device), buf.ctypes.data_as(C.POINTER(C.c_uint16)), pitch * 2, w, h,
                                         None if infill is None else C.byref(infill),
                                         flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rows), C.byref(cols)),
               what="infill_plane")
    if not (buf[:, w:] == 65535).all():
        raise RuntimeError("infill_plane: the cells between the rows were written")
    return np.ascontiguousarray(buf[:, :w]), flags, rows.value, cols.value


def _c_int(v, what):
    v = int(v)
    if not -2 ** 31 <= v < 2 ** 31:
        raise capi.CvoHipError("%s: outside the range of a C int" % what)
    return v


def check_pixel_format(fmt, width, height):
    """True for a PIXEL_* format that fits a width x height picture (cvo_fe_check_pixel_format): YUY2 and UYVY need an
    even width, NV12 an even width and height, Bayer at least 2 x 2.  Host only."""
    return lib().cvo_fe_check_pixel_format(_c_int(fmt, "check_pixel_format"), _c_int(width, "check_pixel_format"),
                                           _c_int(height, "check_pixel_format")) == 0


def pixel_layout(fmt, width, height):
    """(rows, row_bytes) of a packed width x height image of format `fmt` (cvo_fe_pixel_layout).  Host only."""
    row, rows = C.c_size_t(0), C.c_int(0)
    capi.check(lib().cvo_fe_pixel_layout(_c_int(fmt, "pixel_layout"), _c_int(width, "pixel_layout"),
                                         _c_int(height, "pixel_layout"), C.byref(row), C.byref(rows)), what="pixel_layout")
    return rows.value, row.value


def unpack_image(src, fmt, width, height, device=0, stride=None):
    """The unpack contract on any packed image (cvo_fe_unpack_image: the kernel a frame runs, without a generator): `src`
    is any uint8 array whose C-order bytes are the rows of pixel_layout(fmt, width, height), `stride` bytes apart (dense
    without one).  Returns the height x width x 3 uint8 image, B G R; the argument is left as it is."""
    rows, row = pixel_layout(fmt, width, height)
    pitch = row if stride is None else int(stride)
    src = np.ascontiguousarray(src, np.uint8)
    if pitch < row or src.size != rows * pitch:
        raise ValueError("expected %d rows of %d bytes, %d apart" % (rows, row, pitch))
    out = np.empty((int(height), int(width), 3), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    capi.check(lib().cvo_fe_unpack_image(int(device), src.ctypes.data_as(u8p), pitch, int(width), int(height), int(fmt),
                                         out.ctypes.data_as(u8p)), what="unpack_image")
    return out


def check_binning(binning, width, height):
    """True for a Binning set_input_binning() accepts on a generator of width x height (cvo_fe_check_binning): factor 2,
    3 or 4, depth_min in [1, factor^2], pad_ 0, factor times the size at most 8192 each way; None is refused.  Host only."""
    return lib().cvo_fe_check_binning(None if binning is None else C.byref(binning), _c_int(width, "check_binning"),
                                      _c_int(height, "check_binning")) == 0


def bin_camera(model, factor):
    """The CameraModel of the binned image from the input image's (cvo_fe_bin_camera): fx / f, fy / f,
    (cx - (f - 1) / 2) / f, (cy - (f - 1) / 2) / f in float32; depth_scale and dist unchanged.  Host only."""
    out = CameraModel()
    capi.check(lib().cvo_fe_bin_camera(C.byref(model), _c_int(factor, "bin_camera"), C.byref(out)), what="bin_camera")
    return out


def bin_stereo_rig(rig, factor):
    """bin_camera()'s rule on the two lenses and the rectified pinhole of a StereoRig (cvo_fe_bin_stereo_rig); the
    rotations, the baseline and depth_scale unchanged.  Host only."""
    out = StereoRig()
    capi.check(lib().cvo_fe_bin_stereo_rig(C.byref(rig), _c_int(factor, "bin_stereo_rig"), C.byref(out)),
               what="bin_stereo_rig")
    return out


def _strided(src, row_items, stride, fill):
    """`src` (rows x row_items ...) in rows `stride` items apart, the cells between them holding `fill`."""
    pitch = row_items if stride is None else int(stride)
    if pitch < row_items:
        raise ValueError("stride below the row")
    buf = np.full((src.shape[0], pitch), fill, src.dtype)
    buf[:, :row_items] = src.reshape(src.shape[0], row_items)
    return buf, pitch


def bin_image(bgr, factor, device=0, stride=None):
    """The binning contract on any fh x fw x 3 uint8 image (cvo_fe_bin_image: the kernel a frame runs, without a
    generator).  Returns the h x w x 3 image; the argument is left as it is.  `stride`: the image is handed over in rows
    that many bytes apart (at least fw * 3)."""
    f = _c_int(factor, "bin_image")
    src = np.ascontiguousarray(bgr, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3 or f < 1 or src.shape[0] % f or src.shape[1] % f:
        raise ValueError("expected an fh x fw x 3 uint8 image, fh and fw multiples of the factor")
    h, w = src.shape[0] // f, src.shape[1] // f
    buf, pitch = _strided(src, src.shape[1] * 3, stride, 0xA5)
    keep = buf.copy()
    out = np.empty((h, w, 3), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    capi.check(lib().cvo_fe_bin_image(int(device), buf.ctypes.data_as(u8p), pitch, w, h, f, out.ctypes.data_as(u8p)),
               what="bin_image")
    if not (buf == keep).all():
        raise RuntimeError("bin_image: the source was written")
    return out


def bin_depth(plane, binning, device=0, stride=None):
    """The binning contract on any fh x fw uint16 plane with 0 = none (cvo_fe_bin_depth).  Returns (the h x w plane, the
    number of its pixels with a depth); the argument is left as it is.  `stride`: rows that many uint16 apart."""
    f = int(binning.factor) if binning is not None else 0
    src = np.ascontiguousarray(plane, np.uint16)
    if src.ndim != 2 or f < 1 or src.shape[0] % f or src.shape[1] % f:
        raise ValueError("expected an fh x fw uint16 plane, fh and fw multiples of the factor")
    h, w = src.shape[0] // f, src.shape[1] // f
    buf, pitch = _strided(src, src.shape[1], stride, 0xA5A5)
    keep = buf.copy()
    out = np.empty((h, w), np.uint16)
    valid = C.c_int(0)
    u16p = C.POINTER(C.c_uint16)
    capi.check(lib().cvo_fe_bin_depth(int(device), buf.ctypes.data_as(u16p), pitch * 2, w, h, C.byref(binning),
                                      out.ctypes.data_as(u16p), C.byref(valid)), what="bin_depth")
    if not (buf == keep).all():
        raise RuntimeError("bin_depth: the source was written")
    return out, valid.value


def _photo_tables(response, vignette, width, height, what):
    """The two tables as the library takes them: (response 3 x 256 uint16 or None, vignette h x w uint16 or None)."""
    if response is not None:
        response = np.ascontiguousarray(response, np.uint16)
        if response.shape != (3, 256):
            raise ValueError("%s: expected a 3 x 256 uint16 response table (B, G, R)" % what)
    if vignette is not None:
        vignette = np.ascontiguousarray(vignette, np.uint16)
        if vignette.shape != (height, width):
            raise ValueError("%s: expected a %d x %d uint16 vignette, the size of the images a frame takes" % (what, height, width))
    return response, vignette


def _u16p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint16))


def check_photometric(photometric, response=False, vignette=False):
    """True for a Photometric set_photometric() accepts beside a response table / a vignette (`response`, `vignette`:
    whether one is handed over; cvo_fe_check_photometric); None is refused.  Host only."""
    return lib().cvo_fe_check_photometric(None if photometric is None else C.byref(photometric),
                                          1 if response is not None and response is not False else 0,
                                          1 if vignette is not None and vignette is not False else 0) == 0


def response_table(inv):
    """A row of the response table from a channel's inverse response, 256 floats in [0, 255] -- a row of DSO's
    pcalib.txt (cvo_fe_response_table): min(65535, uint32(v * 256 + 0.5)) in float32.  Host only."""
    src = np.ascontiguousarray(inv, np.float32)
    if src.shape != (256,):
        raise ValueError("response_table: expected 256 values")
    out = np.empty(256, np.uint16)
    capi.check(lib().cvo_fe_response_table(src.ctypes.data_as(C.POINTER(C.c_float)), _u16p(out)), what="response_table")
    return out


def vignette_gains(atten):
    """The vignette's Q12 gains from its attenuations as uint16, 65535 = none -- the plane of DSO's vignette.png
    (cvo_fe_vignette_gains): a ? min(65535, (4096 * 65535 + a // 2) // a) : 65535, in the argument's shape.  Host only."""
    src = np.ascontiguousarray(atten, np.uint16)
    out = np.empty(src.shape, np.uint16)
    capi.check(lib().cvo_fe_vignette_gains(_u16p(src), src.size, _u16p(out)), what="vignette_gains")
    return out


def photometric_image(bgr, photometric, response=None, vignette=None, gains_q12=None, device=0, stride=None,
                      vignette_stride=None):
    """The photometric contract on any h x w x 3 uint8 image (cvo_fe_photometric_image: the kernels a frame runs,
    without a generator; under PHOTO_AUTO the image is a first frame).  Returns (the corrected image, its
    PhotometricFrame); the argument is left as it is.  `stride`: the image is handed over in rows that many bytes apart;
    `vignette_stride`: the vignette in rows that many uint16 apart."""
    src = np.ascontiguousarray(bgr, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("expected an h x w x 3 uint8 image")
    h, w = src.shape[:2]
    response, vignette = _photo_tables(response, vignette, w, h, "photometric_image")
    buf, pitch = _strided(src, w * 3, stride, 0xA5)
    keep = buf.copy()
    vbuf, vpitch = (None, 0) if vignette is None else _strided(vignette, w, vignette_stride, 0xA5A5)
    g = None if gains_q12 is None else (C.c_uint32 * 3)(*(int(v) for v in gains_q12))
    out, rec = np.empty((h, w, 3), np.uint8), PhotometricFrame()
    u8p = C.POINTER(C.c_uint8)
    capi.check(lib().cvo_fe_photometric_image(int(device), buf.ctypes.data_as(u8p), w, h, pitch,
                                              None if photometric is None else C.byref(photometric), _u16p(response),
                                              _u16p(vbuf), vpitch * 2, g, out.ctypes.data_as(u8p), C.byref(rec)),
               what="photometric_image")
    if not (buf == keep).all():
        raise RuntimeError("photometric_image: the source was written")
    return out, rec


def check_depth_format(fmt, unit=1.0):
    """True for what set_depth_format() accepts (cvo_fe_check_depth_format): a DEPTH_* format, a finite unit in
    [2^-20, 2^20], and a unit of 1 under DEPTH_U16.  Host only."""
    return lib().cvo_fe_check_depth_format(_c_int(fmt, "check_depth_format"), float(unit)) == 0


def convert_depth(src, fmt, width, height, unit=1.0, scale=1000.0, device=0, stride=None):
    """The depth-format contract on any plane (cvo_fe_convert_depth: the kernel a frame runs, without a generator): `src`
    is any array whose C-order bytes are `height` rows of `width` values of the format (uint16, float32, float16),
    `stride` bytes apart (dense without one; the last row may end with its last value).  `scale` is the depth_scale of
    what reads the plane.  Returns the height x width uint16 plane; the argument is left as it is."""
    fmt, w, h = _c_int(fmt, "convert_depth"), _c_int(width, "convert_depth"), _c_int(height, "convert_depth")
    if fmt not in _DEPTH_DTYPES:
        raise capi.CvoHipError("convert_depth: an unknown depth format")
    item = np.dtype(_DEPTH_DTYPES[fmt]).itemsize
    pitch = w * item if stride is None else int(stride)
    src = np.ascontiguousarray(src)
    if h < 1 or w < 1 or pitch < w * item or src.nbytes < (h - 1) * pitch + w * item:
        raise ValueError("expected %d rows of %d values of %d bytes, %d bytes apart" % (h, w, item, pitch))
    out = np.empty((h, w), np.uint16)
    capi.check(lib().cvo_fe_convert_depth(int(device), src.ctypes.data, pitch, w, h, fmt, float(unit), float(scale),
                                          out.ctypes.data_as(C.POINTER(C.c_uint16))), what="convert_depth")
    return out


_DEVICE_TYPES = {1: ("u1",), 2: ("u2", "f2"), 4: ("f4",)}


def device_image(obj, rows, row_bytes, itemsize, what):
    """(pointer, pitch in bytes) of an image in device memory: `obj` is any object with `__cuda_array_interface__` (a
    torch tensor on ROCm, a cupy array) that holds `rows` rows of `row_bytes` bytes in items of `itemsize` bytes -- shape
    (rows, ...) with the dimensions behind the first dense, as a slice of a wider array is.  ValueError for another dtype
    or shape, a last dimension that is not dense, a row stride below the row or not a multiple of the item size, and
    negative strides.  It needs no device: nothing is read through the pointer."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise ValueError("%s: an object with __cuda_array_interface__ is expected (a device array)" % what)
    typestr, shape, strides = str(cai["typestr"]), tuple(int(v) for v in cai["shape"]), cai.get("strides")
    if typestr[:1] not in "<|" or typestr[1:] not in _DEVICE_TYPES.get(int(itemsize), ()):
        raise ValueError("%s: dtype %s, and items of %d bytes are expected" % (what, typestr, itemsize))
    inner = 1
    for v in shape[1:]:
        inner *= v
    if len(shape) < 2 or shape[0] != rows or inner * itemsize != row_bytes:
        raise ValueError("%s: shape %s, and %d rows of %d bytes are expected" % (what, shape, rows, row_bytes))
    pitch = row_bytes
    if strides is not None:
        strides = tuple(int(v) for v in strides)
        if len(strides) != len(shape) or any(v < 0 for v in strides):
            raise ValueError("%s: strides %s (negative strides are not taken)" % (what, strides))
        dense = itemsize
        for k in range(len(shape) - 1, 0, -1):
            if strides[k] != dense:
                raise ValueError("%s: strides %s: every dimension behind the first must be dense" % (what, strides))
            dense *= shape[k]
        if rows > 1:
            pitch = strides[0]
        if pitch < row_bytes or pitch % itemsize != 0:
            raise ValueError("%s: a row stride of %d bytes, below the row of %d or no multiple of the item size %d"
                             % (what, pitch, row_bytes, itemsize))
    ptr = cai["data"][0]
    if not ptr:
        raise ValueError("%s: a null device pointer" % what)
    return int(ptr), int(pitch)


def check_lidar(lidar):
    """True for a Lidar set_lidar() accepts on a generator without stereo and depth camera (cvo_fe_check_lidar); None is
    refused.  Host only."""
    if lidar is None:
        return lib().cvo_fe_check_lidar(None) == 0
    return lib().cvo_fe_check_lidar(C.byref(lidar)) == 0


def _scan(points):
    """A scan as the C side takes it: (a float32 array that owns the records, its address, the stride in bytes, n).
    `points` is n x k float32 with k >= 3, x y z first (KITTI: n x 4); any row stride that is a multiple of 4."""
    pts = np.asarray(points)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] < 3:
        pts = np.asarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError("expected an n x k float32 array of points, k >= 3, x y z first")
    n = pts.shape[0]
    if n and (pts.strides[1] != 4 or pts.strides[0] < 12 or pts.strides[0] % 4):
        pts = np.ascontiguousarray(pts)
    stride = pts.strides[0] if n else max(12, 4 * pts.shape[1])
    return pts, (pts.ctypes.data if n else None), stride, n


def project_points(points, lidar, cam, width, height, device=0):
    """The stage of the LiDAR contract on any scan (cvo_fe_project_points: the kernels a frame runs, without a
    generator).  `points`: n x k float32, x y z first; `cam`: the colour camera (depth scale, fx, fy, cx, cy), e.g.
    tuple(camera(4).values()).  Returns (P as h x w uint16, P0 likewise, the flags as h x w uint8 of LIDAR_HIT /
    LIDAR_OCCLUDED, the number of pixels hit, the number of those dropped as occluded)."""
    pts, addr, stride, n = _scan(points)
    cam = np.ascontiguousarray(cam, np.float32)
    if cam.shape != (5,):
        raise ValueError("cam holds depth scale, fx, fy, cx, cy")
    w, h = int(width), int(height)
    if not (1 <= w <= 8192 and 1 <= h <= 8192):
        raise capi.CvoHipError("project_points: width and height in [1, 8192]")
    plane, p0, flags = np.empty((h, w), np.uint16), np.empty((h, w), np.uint16), np.empty((h, w), np.uint8)
    hits, occluded = C.c_int(0), C.c_int(0)
    u16p = C.POINTER(C.c_uint16)
    capi.check(lib().cvo_fe_project_points(int(device), addr, stride, n, None if lidar is None else C.byref(lidar),
                                           cam.ctypes.data_as(C.POINTER(C.c_float)), w, h, plane.ctypes.data_as(u16p),
                                           p0.ctypes.data_as(u16p), flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           C.byref(hits), C.byref(occluded)), what="project_points")
    return plane, p0, flags, hits.value, occluded.value


def check_lidar_sweep(sweep):
    """True for a LidarSweep set_lidar_sweep() accepts on a generator with a scan source (cvo_fe_check_lidar_sweep);
    None is refused.  Host only."""
    return lib().cvo_fe_check_lidar_sweep(None if sweep is None else C.byref(sweep)) == 0


def _twist(twist, what):
    tw = np.ascontiguousarray(twist, np.float32)
    if tw.shape != (6,):
        raise ValueError("%s: a twist holds w (radians per sweep) then v (metres per sweep), six numbers" % what)
    return tw


def lidar_twist(transform, lidar, sweep_fraction=1.0):
    """The twist for set_lidar_motion() of a caller who assumes the velocity of the last frame interval to hold
    (cvo_fe_lidar_twist; host only, float64): `transform` is the registration's last relative transform, 4 x 4 as
    `registration.transform` holds it -- coordinates in the earlier camera's frame to coordinates in the later one's, so
    the camera's motion is its inverse --, `lidar` the Lidar whose R, T mount the scanner, `sweep_fraction` the sweep
    duration over the frame interval.  Raises for a motion over the caps of set_lidar_motion()."""
    T = np.ascontiguousarray(transform, np.float32)
    if T.shape != (4, 4):
        raise ValueError("expected a 4 x 4 transform")
    out = np.zeros(6, np.float32)
    fp = C.POINTER(C.c_float)
    capi.check(lib().cvo_fe_lidar_twist(T.ctypes.data_as(fp), None if lidar is None else C.byref(lidar),
                                        float(sweep_fraction), out.ctypes.data_as(fp)), what="lidar_twist")
    return out


def project_points_sweep(points, lidar, cam, width, height, sweep, twist, device=0):
    """project_points() under the sweep contract (cvo_fe_project_points_sweep): `points` n x k float32 whose records
    hold the time word of a field mode at `sweep.time_offset` (a uint32 time: view the array as float32); `twist`: w
    then v of the scan.  Returns project_points()'s five and (the phase of every point, p' of every point as n x 3):
    NaN for a point skipped before it has a phase."""
    pts, addr, stride, n = _scan(points)
    cam = np.ascontiguousarray(cam, np.float32)
    if cam.shape != (5,):
        raise ValueError("cam holds depth scale, fx, fy, cx, cy")
    w, h = int(width), int(height)
    if not (1 <= w <= 8192 and 1 <= h <= 8192):
        raise capi.CvoHipError("project_points_sweep: width and height in [1, 8192]")
    tw = _twist(twist, "project_points_sweep")
    plane, p0, flags = np.empty((h, w), np.uint16), np.empty((h, w), np.uint16), np.empty((h, w), np.uint8)
    phase, moved = np.empty(n, np.float32), np.empty((n, 3), np.float32)
    hits, occluded = C.c_int(0), C.c_int(0)
    u16p, fp = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    capi.check(lib().cvo_fe_project_points_sweep(
        int(device), addr, stride, n, None if lidar is None else C.byref(lidar), cam.ctypes.data_as(fp), w, h,
        plane.ctypes.data_as(u16p), p0.ctypes.data_as(u16p), flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(hits),
        C.byref(occluded), None if sweep is None else C.byref(sweep), tw.ctypes.data_as(fp), phase.ctypes.data_as(fp),
        moved.ctypes.data_as(fp)), what="project_points_sweep")
    return plane, p0, flags, hits.value, occluded.value, phase, moved


def stereo_depth_table(stereo, fx, depth_scale):
    """U(q) of the stereo contract (include/cvo_frontend.h) for q = 0 .. 16 * max_disp - 1: the depth value of a
    disparity of q / 16 pixel under a camera of focal length `fx` and `depth_scale` units per metre; uint16.  Host only."""
    out = np.empty(16 * int(stereo.max_disp), np.uint16)
    capi.check(lib().cvo_fe_stereo_depth_table(C.byref(stereo), fx, depth_scale, out.ctypes.data_as(C.POINTER(C.c_uint16))),
               what="stereo_depth_table")
    return out


def check_stereo_rig(rig):
    """True for a StereoRig set_stereo_rig() accepts (cvo_fe_check_stereo_rig).  Host only."""
    return lib().cvo_fe_check_stereo_rig(C.byref(rig)) == 0


def stereo_rectify(calib, width, height, depth_scale=1000.0):
    """The StereoRig of a StereoCalib for width x height images (cvo_fe_stereo_rectify, the helper of the rig contract
    of include/cvo_frontend.h); `depth_scale`: the units per metre the depth plane shall have.  Raises for a calibration
    the helper refuses: cameras turned more than 0.5 rad against each other, a rig that is not horizontal with the
    right camera on the right.  Host only."""
    out = StereoRig()
    capi.check(lib().cvo_fe_stereo_rectify(C.byref(calib), int(width), int(height), C.byref(out), depth_scale),
               what="stereo_rectify")
    return out


def stereo_rig_map(rig, which, width, height):
    """The map of the rig contract for camera `which` (0 left, 1 right): (qu, qv), int32 height x width, where each
    pixel of the rectified image looks in the raw one, in 1/32 pixel.  Host only."""
    qu = np.empty((int(height), int(width)), np.int32)
    qv = np.empty_like(qu)
    i32p = C.POINTER(C.c_int32)
    capi.check(lib().cvo_fe_stereo_rig_map(C.byref(rig), int(which), int(width), int(height), qu.ctypes.data_as(i32p),
                                           qv.ctypes.data_as(i32p)), what="stereo_rig_map")
    return qu, qv


class PcdGenerator:
    """ref include/pcd_generator.hpp:30-108; one object per image size."""

    def __init__(self, width=640, height=480, device=0, stream=None, num_want=3000):
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        st = lib().cvo_fe_create(device, stream, self.width, self.height, C.byref(self._h))
        if st != 0:
            self._h = C.c_void_p()
            capi.check(st, what="cvo_fe_create (the front end needs a gfx950 device: no CPU path)")
        self.num_want = int(num_want)
        self._chk(lib().cvo_fe_set_num_want(self._h, self.num_want), "set_num_want")
        self.capacity = self.width * self.height   # (upper bound of any selection)
        self._iw, self._ih = self.width, self.height   # of the colour images a frame takes: f times the size under set_input_binning
        self._dshape = (self.height, self.width)   # of the depth image: the depth camera's, if one is set
        self._has_rig = False
        self._max_disp = 0                         # of the stereo settings, if some are set
        self._pix = PIXEL_BGR8                     # the pixel format of the colour images (set_pixel_format)
        self._ishape = (self.height, self.width * 3)   # rows x row_bytes of a colour image in that format
        self._dfmt = DEPTH_U16                     # the format of the depth images (set_depth_format)
        self._held = None                          # the device images of a frame in flight (submit_device)
        self._pos = np.empty((self.capacity, 3), np.float32)
        self._feat = np.empty((self.capacity, 5), np.float32)

    def _chk(self, st, what):
        if st != 0:
            msg = lib().cvo_fe_last_error(self._h)
            raise capi.CvoHipError("%s: %s (%s)" % (what, capi.lib().cvo_hip_error_string(st).decode(),
                                                     msg.decode() if msg else ""))

    def _set_struct(self, name, obj):
        """cvo_fe_set_<name> with a settings structure, or None: the setting cleared."""
        self._chk(getattr(lib(), "cvo_fe_set_" + name)(self._h, None if obj is None else C.byref(obj)), "set_" + name)

    def _get_struct(self, name, cls):
        """cvo_fe_get_<name>: the structure in force, or None where the library says "not set"."""
        out, isset = cls(), C.c_int(0)
        self._chk(getattr(lib(), "cvo_fe_get_" + name)(self._h, C.byref(out), C.byref(isset)), "get_" + name)
        return out if isset.value else None

    def _get_int(self, name, ctype):
        out = ctype(0)
        self._chk(getattr(lib(), "cvo_fe_get_" + name)(self._h, C.byref(out)), "get_" + name)
        return int(out.value)

    def _images(self, bgr, depth):
        """The two images of a frame as dense arrays of the sizes the context takes."""
        bgr = self._image(bgr)
        dtype = np.dtype(_DEPTH_DTYPES[self._dfmt])
        depth = np.ascontiguousarray(depth, dtype)
        if depth.shape != self._dshape:
            raise ValueError("expected a %dx%d %s depth map" % (self._dshape + (dtype.name,)))
        return bgr, depth

    def create_pointcloud(self, bgr, depth, dataset_seq=1, feature_type=FEATURES_RGB):
        """load_image + create_pointcloud (ref src/pcd_generator.cpp:387-420): returns
        (positions n x 3, features n x 5 row-major), points in image scan order."""
        bgr, depth = self._images(bgr, depth)
        n = C.c_int(0)
        st = lib().cvo_fe_create_pointcloud(
            self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)), self._ishape[1],
            depth.ctypes.data_as(C.POINTER(C.c_uint16)), self._dshape[1] * depth.itemsize, int(dataset_seq), int(feature_type),
            self._pos.ctypes.data_as(C.POINTER(C.c_float)), self._feat.ctypes.data_as(C.POINTER(C.c_float)),
            self.capacity, C.byref(n))
        self._chk(st, "create_pointcloud")
        return self._pos[:n.value].copy(), self._feat[:n.value].copy()

    def submit(self, bgr, depth, dataset_seq=1, feature_type=FEATURES_RGB):
        """First half of create_pointcloud: stage the images, enqueue everything, return."""
        bgr, depth = self._images(bgr, depth)
        self._chk(lib().cvo_fe_submit(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)), self._ishape[1],
                                      depth.ctypes.data_as(C.POINTER(C.c_uint16)), self._dshape[1] * depth.itemsize,
                                      int(dataset_seq), int(feature_type)), "submit")

    def submit_device(self, img, depth, dataset_seq=1, feature_type=FEATURES_RGB):
        """submit() for images that lie in device memory already (cvo_fe_submit_device; the device-input contract of
        include/cvo_frontend.h): `img` and `depth` are any objects with `__cuda_array_interface__` -- torch tensors on
        ROCm have it -- of the layout the host forms take: uint8 rows of the pixel format in force (h x w x 3 under BGR8),
        and an h x w plane of the depth format's dtype of the depth camera's size.  A slice of a wider array is taken with
        its pitch; nothing is copied to the host.  collect() / collect_device() as for any other frame.
        Streams: the images are read by work on this generator's stream.  What wrote them must have completed -- the
        caller synchronises the producer (torch.cuda.synchronize()) -- or the generator must have been created on the
        producer's stream (PcdGenerator(stream=...)).  They must stay alive and unwritten until the frame is collected;
        the generator keeps a reference until then."""
        pi, si = device_image(img, self._ishape[0], self._ishape[1], 1, "submit_device: the colour image")
        item = np.dtype(_DEPTH_DTYPES[self._dfmt]).itemsize
        pd, sd = device_image(depth, self._dshape[0], self._dshape[1] * item, item, "submit_device: the depth image")
        want = np.dtype(_DEPTH_DTYPES[self._dfmt]).str[1:]
        if str(depth.__cuda_array_interface__["typestr"])[1:] != want:
            raise ValueError("submit_device: the depth image: dtype %s is expected (the depth format in force)" % want)
        self._chk(lib().cvo_fe_submit_device(self._h, pi, si, pd, sd, int(dataset_seq), int(feature_type)), "submit_device")
        self._held = (img, depth)

    def submit_stereo_device(self, left, right, dataset_seq=4, feature_type=FEATURES_RGB):
        """submit_stereo() for a pair that lies in device memory already (cvo_fe_submit_stereo_device): two objects with
        `__cuda_array_interface__`, uint8 rows of the pixel format in force.  Streams and lifetime as submit_device()."""
        pl, sl = device_image(left, self._ishape[0], self._ishape[1], 1, "submit_stereo_device: the left image")
        pr, sr = device_image(right, self._ishape[0], self._ishape[1], 1, "submit_stereo_device: the right image")
        self._chk(lib().cvo_fe_submit_stereo_device(self._h, pl, sl, pr, sr, int(dataset_seq), int(feature_type)),
                  "submit_stereo_device")
        self._held = (left, right)

    def collect(self):
        """Second half: wait for the submitted frame and return its cloud."""
        n = C.c_int(0)
        self._chk(lib().cvo_fe_collect(self._h, self._pos.ctypes.data_as(C.POINTER(C.c_float)),
                                       self._feat.ctypes.data_as(C.POINTER(C.c_float)), self.capacity, C.byref(n)),
                  "collect")
        self._held = None
        return self._pos[:n.value].copy(), self._feat[:n.value].copy()

    def collect_device(self):
        """collect() without the copy to the host: (device address of the positions, of the
        features, number of points); valid until the next submit on this object."""
        dp, df, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._chk(lib().cvo_fe_collect_device(self._h, C.byref(dp), C.byref(df), C.byref(n)), "collect_device")
        self._held = None
        return dp.value, df.value, n.value

    def host_buffers(self):
        """numpy views of the context's pinned staging images (h x w x 3 uint8, h x w uint16): fill
        them in place and pass them to submit() / create_pointcloud() to save a copy.  The depth view is
        of the depth camera's size while one is set and valid until the next set_depth_camera().  Under a pixel
        format the image view is the packed image, rows x row_bytes, valid until the next set_pixel_format().  Under a
        float depth format the depth view is the float staging image (float32 or float16), valid until the next
        set_depth_format() / set_depth_camera().  Under input binning both views are of the input size, factor times the
        generator's each way (the depth view unless a depth camera is set), valid until the next set_input_binning()."""
        pi, pd = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint16)()
        self._chk(lib().cvo_fe_host_buffers(self._h, C.byref(pi), C.byref(pd)), "host_buffers")
        img = np.ctypeslib.as_array(pi, shape=self._ishape if self._pix != PIXEL_BGR8 else (self._ih, self._iw, 3))
        dep = np.ctypeslib.as_array(pd, shape=self._dshape)
        if self._dfmt != DEPTH_U16:   # (the same memory, seen as the format's values)
            dtype = np.dtype(_DEPTH_DTYPES[self._dfmt])
            raw = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_uint8)), shape=(self._dshape[0] * self._dshape[1] * dtype.itemsize,))
            dep = raw.view(dtype).reshape(self._dshape)
        return img, dep

    def set_device_output(self, on=True):
        """The following frames are taken with collect_device(): no copy of the cloud to the host."""
        self._chk(lib().cvo_fe_set_device_output(self._h, 1 if on else 0), "set_device_output")

    def set_camera(self, model):
        """A CameraModel for every following frame (their `dataset_seq` is then ignored); None: back
        to the reference's table.  A model with distortion makes each frame start with the
        rectification of both images on the device."""
        self._set_struct("camera", model)

    def camera(self):
        """The CameraModel set, or None while the table is in use."""
        return self._get_struct("camera", CameraModel)

    rectify_map = staticmethod(rectify_map)

    def set_depth_camera(self, rig):
        """A DepthCamera for every following frame: their `depth` is then rig.height x rig.width and is
        registered into the colour camera's frame on the device (the registration contract of
        include/cvo_frontend.h); None: depth is registered to colour already, as for a new object."""
        self._set_struct("depth_camera", rig)
        self._has_rig = rig is not None
        self._dshape = (self._ih, self._iw) if rig is None else (int(rig.height), int(rig.width))

    def depth_camera(self):
        """The DepthCamera set, or None."""
        return self._get_struct("depth_camera", DepthCamera)

    depth_rays = staticmethod(depth_rays)

    def set_depth_gate(self, gate):
        """A DepthGate for every following frame: pixels out of range or on / within `grow` of a depth
        discontinuity give no point (the gate contract of include/cvo_frontend.h); None: no gate, as for a
        new object."""
        self._set_struct("depth_gate", gate)

    def depth_gate(self):
        """The DepthGate set, or None."""
        return self._get_struct("depth_gate", DepthGate)

    def set_mask(self, mask):
        """A mask for every following frame: h x w uint8 or bool on the grid of the colour image as uploaded
        (any row stride), non-zero = no point from this pixel; None: no mask.  The bytes are copied; the mask
        stays until it is replaced or cleared."""
        if mask is None:
            self._chk(lib().cvo_fe_set_mask(self._h, None, 0), "set_mask")
            return
        mask = np.asarray(mask)
        if mask.dtype == np.bool_:
            mask = mask.view(np.uint8)
        if mask.dtype != np.uint8 or mask.shape != (self.height, self.width):
            raise ValueError("expected a %dx%d uint8 or bool mask" % (self.height, self.width))
        if mask.strides[1] != 1 or mask.strides[0] < self.width:
            mask = np.ascontiguousarray(mask)
        self._chk(lib().cvo_fe_set_mask(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.strides[0]), "set_mask")

    def set_stereo(self, stereo):
        """A Stereo for every following frame: a frame is then a rectified stereo pair (submit_stereo /
        create_pointcloud_stereo) and a semi-global matcher on the device fills the depth plane (the stereo contract
        of include/cvo_frontend.h); None: back to depth images, as for a new object."""
        self._set_struct("stereo", stereo)
        self._max_disp = 0 if stereo is None else int(stereo.max_disp)

    def stereo(self):
        """The Stereo set, or None."""
        return self._get_struct("stereo", Stereo)

    def set_stereo_paths(self, mask):
        """The path mask of the matcher for every following stereo frame (step 4 of the stereo contract): PATHS_4 (a new
        object's), PATHS_8, or any non-empty subset of the eight bits; one launch per path.  A setting of its own: it
        may be made with or without stereo set and survives set_stereo()."""
        mask = int(mask)
        if not 0 <= mask <= 0xFFFFFFFF:
            raise capi.CvoHipError("set_stereo_paths: a mask of 32 bits at the most")
        self._chk(lib().cvo_fe_set_stereo_paths(self._h, mask), "set_stereo_paths")

    def stereo_paths(self):
        """The path mask in force."""
        return self._get_int("stereo_paths", C.c_uint32)

    def set_stereo_speckle(self, speckle):
        """A Speckle for every following stereo frame: components of the disparity plane of `max_size` pixels at the
        most lose their disparity and their depth (the speckle contract of include/cvo_frontend.h); None: no filter, as
        for a new object.  A setting of its own: it may be made with or without stereo set and survives set_stereo()."""
        self._set_struct("stereo_speckle", speckle)

    def stereo_speckle(self):
        """The Speckle set, or None."""
        return self._get_struct("stereo_speckle", Speckle)

    def set_depth_median(self, median):
        """A DepthMedian for every following frame of any kind: the depth plane passes the median stage in front of the
        gate (the median contract of include/cvo_frontend.h); None: no filter, as for a new object.  A setting of its
        own: it survives every other setter."""
        self._set_struct("depth_median", median)

    def depth_median(self):
        """The DepthMedian set, or None."""
        return self._get_struct("depth_median", DepthMedian)

    def set_depth_infill(self, infill):
        """A DepthInfill for every following frame of any kind: the depth plane passes the infill stage directly behind
        whatever fills it (the infill contract of include/cvo_frontend.h); None: no stage, as for a new object.  A setting
        of its own: it survives every other setter."""
        self._set_struct("depth_infill", infill)

    def depth_infill(self):
        """The DepthInfill set, or None."""
        return self._get_struct("depth_infill", DepthInfill)

    def set_lidar(self, lidar):
        """A Lidar for every following frame: a frame is then a colour image and a scan (submit_lidar /
        create_pointcloud_lidar), projected into the colour camera on the device (the LiDAR contract of
        include/cvo_frontend.h); None: back to depth images, as for a new object.  Refused beside stereo and a depth
        camera, and they beside it."""
        self._set_struct("lidar", lidar)

    def lidar(self):
        """The Lidar set, or None."""
        return self._get_struct("lidar", Lidar)

    def set_lidar_sweep(self, sweep):
        """A LidarSweep for the scan source: every point of a frame's scan is moved into the scanner's frame at the
        instant of the colour image, by the twist of set_lidar_motion(), before it is projected (the sweep contract of
        include/cvo_frontend.h); None: no motion compensation, as for a new object.  Needs a scan source and goes
        with it; the twist is zero afterwards."""
        self._set_struct("lidar_sweep", sweep)

    def lidar_sweep(self):
        """The LidarSweep set, or None."""
        return self._get_struct("lidar_sweep", LidarSweep)

    def set_lidar_motion(self, twist):
        """The scanner's own motion over one full sweep, in its own frame, for the frames submitted from now on: w
        (radians per sweep) then v (metres per sweep); |w| <= 1 and |v| <= 64.  Needs a sweep."""
        tw = _twist(twist, "set_lidar_motion")
        self._chk(lib().cvo_fe_set_lidar_motion(self._h, tw.ctypes.data_as(C.POINTER(C.c_float))), "set_lidar_motion")

    def lidar_motion(self):
        """The twist in force: six float32, zero without a sweep."""
        out = np.zeros(6, np.float32)
        self._chk(lib().cvo_fe_get_lidar_motion(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "get_lidar_motion")
        return out

    def _image(self, bgr):
        """A colour image as a dense array: h x w x 3 under BGR8, else any uint8 array whose C-order bytes are the
        rows x row_bytes of the pixel format in force."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if self._pix == PIXEL_BGR8:
            if bgr.shape != (self._ih, self._iw, 3):
                raise ValueError("expected a %dx%dx3 uint8 image" % (self._ih, self._iw))
        elif bgr.size != self._ishape[0] * self._ishape[1]:
            raise ValueError("expected %d rows of %d bytes (the pixel format in force)" % self._ishape)
        return bgr

    def set_pixel_format(self, fmt):
        """The PIXEL_* format of every colour image of every following frame of any kind -- both images of a stereo
        pair (the unpack contract of include/cvo_frontend.h): the images are then handed over packed, pixel_layout()'s
        rows x row_bytes, and unpacked on the device in front of everything else.  PIXEL_BGR8: a new object's.  A
        setting of its own: it survives every other setter."""
        fmt = _c_int(fmt, "set_pixel_format")
        self._chk(lib().cvo_fe_set_pixel_format(self._h, fmt), "set_pixel_format")
        self._pix = fmt
        self._ishape = pixel_layout(fmt, self._iw, self._ih)

    def set_input_binning(self, binning):
        """A Binning for every following frame of any kind (the binning contract of include/cvo_frontend.h): every image
        handed over -- host or device, both of a stereo pair, the depth image unless a depth camera is set -- is then
        factor times the generator's size each way and is binned on the device in front of everything else.  THE
        CAMERAS AND THE MASK OF THE GENERATOR DESCRIBE THE BINNED IMAGE: hand set_camera() bin_camera()'s model and
        set_stereo_rig() bin_stereo_rig()'s rig, or the cloud comes out factor times too large.  None: off, a new
        object's.  A setting of its own: it survives every other setter.  Views of host_buffers() are valid until the
        next call."""
        self._set_struct("input_binning", binning)
        f = 1 if binning is None else int(binning.factor)
        self._iw, self._ih = f * self.width, f * self.height
        self._ishape = pixel_layout(self._pix, self._iw, self._ih)
        if not self._has_rig:
            self._dshape = (self._ih, self._iw)

    def input_binning(self):
        """The Binning in force, or None."""
        return self._get_struct("input_binning", Binning)

    def set_photometric(self, photometric, response=None, vignette=None):
        """A Photometric for every following frame of any kind (the photometric contract of include/cvo_frontend.h): the
        colour bytes -- both images of a stereo pair -- are corrected in place on the device behind the unpack and in
        front of the bin by `response` (3 x 256 uint16, B G R; response_table() makes a row), `vignette` (uint16 Q12
        gains of the size of the images a frame takes; vignette_gains() makes them) and the frame's gain per channel:
        the caller's (PHOTO_GAIN, set_photometric_gain) or estimated (PHOTO_AUTO).  Both tables are copied.  None: off,
        a new object's.  A setting of its own: it survives every other setter; with a vignette set, set_input_binning()
        refuses a change of the input size."""
        if photometric is None:
            self._chk(lib().cvo_fe_set_photometric(self._h, None, None, None, 0), "set_photometric")
            return
        response, vignette = _photo_tables(response, vignette, self._iw, self._ih, "set_photometric")
        self._chk(lib().cvo_fe_set_photometric(self._h, C.byref(photometric), _u16p(response), _u16p(vignette),
                                               self._iw * 2), "set_photometric")

    def photometric(self):
        """The Photometric in force, or None (the tables are not handed back)."""
        return self._get_struct("photometric", Photometric)

    def set_photometric_gain(self, gain):
        """The gains (one number, or B G R) of the frames submitted from now on, under PHOTO_GAIN: e.g. a reference
        exposure time over the frame's.  Finite, in [1/16, 15.99]; they hold until changed, and no graph is dropped."""
        g = np.broadcast_to(np.asarray(gain, np.float32), (3,))
        self._chk(lib().cvo_fe_set_photometric_gain(self._h, (C.c_float * 3)(*(float(v) for v in g))), "set_photometric_gain")

    def photometric_rearm(self):
        """Opens the lock of PHOTO_AUTO: the next frame with enough counted pixels sets the target."""
        self._chk(lib().cvo_fe_photometric_rearm(self._h), "photometric_rearm")

    def photometric_frame(self):
        """The PhotometricFrame of the last collected frame."""
        out = PhotometricFrame()
        self._chk(lib().cvo_fe_get_photometric_frame(self._h, C.byref(out)), "photometric_frame")
        return out

    def set_depth_format(self, fmt, unit=1.0):
        """The DEPTH_* format of the depth image of every following frame that has one (the depth-format contract of
        include/cvo_frontend.h): under DEPTH_F32 / DEPTH_F16 the depth images are float32 / float16 planes in `unit`
        metres per value (1: metres, 0.001: millimetres) and are converted on the device in front of everything else.
        DEPTH_U16 with unit 1: a new object's.  A setting of its own: it survives every other setter."""
        fmt = _c_int(fmt, "set_depth_format")
        self._chk(lib().cvo_fe_set_depth_format(self._h, fmt, float(unit)), "set_depth_format")
        self._dfmt = fmt

    def depth_format(self):
        """(format, unit) in force."""
        fmt, unit = C.c_int(0), C.c_float(0.0)
        self._chk(lib().cvo_fe_get_depth_format(self._h, C.byref(fmt), C.byref(unit)), "get_depth_format")
        return int(fmt.value), float(unit.value)

    def pixel_format(self):
        """The pixel format in force."""
        return self._get_int("pixel_format", C.c_int)

    def create_pointcloud_lidar(self, bgr, points, dataset_seq=4, feature_type=FEATURES_RGB):
        """create_pointcloud() for a colour image and a scan: `points` is n x k float32, x y z first (KITTI's .bin read
        with np.fromfile(..., np.float32).reshape(-1, 4))."""
        bgr = self._image(bgr)
        pts, addr, stride, npts = _scan(points)
        n = C.c_int(0)
        fp = C.POINTER(C.c_float)
        st = lib().cvo_fe_create_pointcloud_lidar(
            self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)), self._ishape[1], addr, stride, npts, int(dataset_seq),
            int(feature_type), self._pos.ctypes.data_as(fp), self._feat.ctypes.data_as(fp), self.capacity, C.byref(n))
        self._chk(st, "create_pointcloud_lidar")
        return self._pos[:n.value].copy(), self._feat[:n.value].copy()

    def submit_lidar(self, bgr, points, dataset_seq=4, feature_type=FEATURES_RGB):
        """submit() for a colour image and a scan; collect() / collect_device() as for any other frame.  The points are
        copied before the call returns."""
        bgr = self._image(bgr)
        pts, addr, stride, npts = _scan(points)
        self._chk(lib().cvo_fe_submit_lidar(self._h, bgr.ctypes.data_as(C.POINTER(C.c_uint8)), self._ishape[1], addr, stride,
                                            npts, int(dataset_seq), int(feature_type)), "submit_lidar")

    def set_select_mode(self, mode):
        """The selector's mode for every following frame (the selection contract of include/cvo_frontend.h): SELECT_IMAGE
        (a new object's: the reference's selector, by the image alone) or SELECT_DEPTH (a pixel without depth does not
        compete, so the cloud holds the num_want asked for).  A setting of its own: it survives every other setter."""
        mode = int(mode)
        if not -2 ** 31 <= mode < 2 ** 31:
            raise capi.CvoHipError("set_select_mode: SELECT_IMAGE or SELECT_DEPTH")
        self._chk(lib().cvo_fe_set_select_mode(self._h, mode), "set_select_mode")

    def select_mode(self):
        """The selector's mode in force."""
        return self._get_int("select_mode", C.c_int)

    def set_stereo_rig(self, rig):
        """A StereoRig for every following frame: submit_stereo / create_pointcloud_stereo then take the RAW pair and
        both images are rectified on the device in front of the matcher (the rig contract of include/cvo_frontend.h);
        the rig is the camera of the frame.  Stereo must be set and no camera model; None: rectified pairs again."""
        self._set_struct("stereo_rig", rig)

    def stereo_rig(self):
        """The StereoRig set, or None."""
        return self._get_struct("stereo_rig", StereoRig)

    stereo_rig_map = staticmethod(stereo_rig_map)

    def _pair(self, left, right):
        return self._image(left), self._image(right)

    def create_pointcloud_stereo(self, left, right, dataset_seq=4, feature_type=FEATURES_RGB):
        """create_pointcloud() for a stereo pair: two h x w x 3 uint8 images (a grey right image is replicated by the
        caller, or both are handed over as they are under set_pixel_format(PIXEL_GREY8)); the left one is the colour image
        of the frame."""
        left, right = self._pair(left, right)
        n = C.c_int(0)
        u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
        st = lib().cvo_fe_create_pointcloud_stereo(
            self._h, left.ctypes.data_as(u8p), self._ishape[1], right.ctypes.data_as(u8p), self._ishape[1], int(dataset_seq),
            int(feature_type), self._pos.ctypes.data_as(fp), self._feat.ctypes.data_as(fp), self.capacity, C.byref(n))
        self._chk(st, "create_pointcloud_stereo")
        return self._pos[:n.value].copy(), self._feat[:n.value].copy()

    def submit_stereo(self, left, right, dataset_seq=4, feature_type=FEATURES_RGB):
        """submit() for a stereo pair; collect() / collect_device() as for any other frame."""
        left, right = self._pair(left, right)
        u8p = C.POINTER(C.c_uint8)
        self._chk(lib().cvo_fe_submit_stereo(self._h, left.ctypes.data_as(u8p), self._ishape[1], right.ctypes.data_as(u8p),
                                             self._ishape[1], int(dataset_seq), int(feature_type)), "submit_stereo")

    def info(self):
        out = Info()
        self._chk(lib().cvo_fe_get_info(self._h, C.byref(out)), "get_info")
        return {k: getattr(out, k) for k, _ in Info._fields_ if k != "pad_"}

    def read_stage(self, stage):
        """An intermediate image of the last create_pointcloud (parity checks)."""
        w, h = self.width, self.height
        fw, fh = self._iw, self._ih
        shapes = {STAGE_FULL_BGR: ((fh, fw, 3), np.uint8), STAGE_FULL_RIGHT_BGR: ((fh, fw, 3), np.uint8),
                  STAGE_FULL_DEPTH: ((fh, fw), np.uint16),
                  STAGE_GRAY: ((h, w), np.uint8), STAGE_HSV: ((h, w, 3), np.uint8), STAGE_MAP: ((h, w), np.float32),
                  STAGE_AG0: ((h, w), np.float32), STAGE_AG1: ((h // 2, w // 2), np.float32),
                  STAGE_AG2: ((h // 4, w // 4), np.float32), STAGE_THS: ((h // 32, w // 32), np.float32),
                  STAGE_DX0: ((h, w), np.float32), STAGE_DY0: ((h, w), np.float32), STAGE_EDGES: ((h, w), np.uint8),
                  STAGE_RECT_BGR: ((h, w, 3), np.uint8), STAGE_RECT_DEPTH: ((h, w), np.uint16),
                  STAGE_RAW_DEPTH: (self._dshape if self._has_rig else (h, w), np.uint16), STAGE_UNGATED_DEPTH: ((h, w), np.uint16),
                  STAGE_GATE: ((h, w), np.uint8), STAGE_RIGHT_GRAY: ((h, w), np.uint8),
                  STAGE_CENSUS_L: ((h, w), np.uint64), STAGE_CENSUS_R: ((h, w), np.uint64),
                  STAGE_SGM_SUM: ((h, w, self._max_disp), np.uint16), STAGE_DISPARITY: ((h, w), np.uint16),
                  STAGE_STEREO: ((h, w), np.uint8), STAGE_RIGHT_BGR: ((h, w, 3), np.uint8),
                  STAGE_STEREO_VALID: ((h, w), np.uint8), STAGE_SPECKLE_SIZE: ((h, w), np.uint32),
                  STAGE_UNFILTERED_DEPTH: ((h, w), np.uint16), STAGE_MEDIAN: ((h, w), np.uint8),
                  STAGE_LIDAR_DEPTH: ((h, w), np.uint16), STAGE_LIDAR: ((h, w), np.uint8),
                  STAGE_SPARSE_DEPTH: ((h, w), np.uint16), STAGE_INFILL: ((h, w), np.uint8),
                  STAGE_INPUT_BGR: ((h, w, 3), np.uint8), STAGE_INPUT_RIGHT_BGR: ((h, w, 3), np.uint8)}
        shape, dt = shapes[stage]
        out = np.empty(shape, dt)
        self._chk(lib().cvo_fe_read_stage(self._h, stage, out.ctypes.data_as(C.c_void_p), out.nbytes), "read_stage")
        return out

    def close(self):
        if self._h:
            lib().cvo_fe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # pragma: no cover
            pass


# ---- the file side of the drivers -------------------------------------------------

def load_file_name(assoc_path):
    """The association list of a TUM sequence: lines `stamp_rgb rgb_path stamp_depth
    depth_path` -> (names, rgb paths, depth paths) (ref src/cvo_main.cpp:69-97)."""
    names, rgb, dep = [], [], []
    with open(assoc_path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            tok += [""] * (4 - len(tok))
            names.append(tok[0]); rgb.append(tok[1]); dep.append(tok[3])
    return names, rgb, dep


def load_img(rgb_path, depth_path):
    """cv::imread(rgb) -> h x w x 3 uint8 in B, G, R order; cv::imread(depth, ANYDEPTH)
    -> h x w uint16 (ref src/cvo_main.cpp:100-106).  Decoding is PIL's."""
    from PIL import Image
    rgb = np.asarray(Image.open(rgb_path).convert("RGB"), np.uint8)
    dep = np.asarray(Image.open(depth_path))
    if dep.dtype != np.uint16:
        dep = dep.astype(np.uint16)
    return np.ascontiguousarray(rgb[:, :, ::-1]), np.ascontiguousarray(dep)


def run_frames(registration, frames, dataset_seq, writer=None, generator=None, prefetch=False, device=True,
               camera=None, depth_camera=None, depth_gate=None, mask=None, stereo=None, stereo_rig=None, stereo_paths=None,
               stereo_speckle=None, select_mode=None, depth_median=None, lidar=None, depth_infill=None, pixel_format=None,
               lidar_sweep=None, lidar_motion=None, sweep_fraction=1.0, depth_format=None, device_input=False,
               input_binning=None, photometric=None, exposures=None):
    """The driver loop on decoded frames: `frames` yields (name, bgr, depth).
    `photometric`: a Photometric for the generator, or (Photometric, response, vignette) with the tables of
    set_photometric(); the vignette has the size of the images `frames` yields.  None leaves the generator as it is.
    `exposures`: the frames' exposure times (a sequence, frame i's at index i): frame i runs under the gain
    exposures[0] / exposures[i] on all channels (set_photometric_gain); the Photometric must have PHOTO_GAIN, and where
    `photometric` is None a Photometric(PHOTO_GAIN) is set.
    `input_binning`: a Binning for the generator: `frames` then yields images of the INPUT size, factor times the
    generator's each way (a first frame decides a new generator's size as shape // factor; a shape that is no multiple
    of the factor is a ValueError), and `camera`, `stereo_rig` and, where `camera` is None, the table row of
    `dataset_seq` describe those INPUT images: they go through bin_camera() / bin_stereo_rig() and the result is set, so
    the geometry is right without knowing the rule.  A `depth_camera` is passed as it is (its colour side is the
    generator's camera).  None leaves the generator as it is.
    `depth_format`: a DEPTH_* format, or (format, unit), for the generator: the depth images `frames` yields are then of
    that format; None leaves the generator as it is.
    `device_input`: `frames` yields device arrays (objects with `__cuda_array_interface__`), which go in through
    submit_device() / submit_stereo_device() and never touch host memory; not for LiDAR frames.  The producer of the
    arrays must be synchronised, or the generator created on its stream (see submit_device()).
    `lidar_sweep`: a LidarSweep for the generator's scan source (motion compensation of a spinning scan); None leaves the
    generator as it is.  `lidar_motion`: where each frame's twist comes from -- None: the generator's stays as it is
    (zero after `lidar_sweep`); a callable name -> twist (w then v, per sweep), asked before the frame is submitted;
    or "constant-velocity": lidar_twist() of the registration's last relative transform, the generator's Lidar and
    `sweep_fraction` (the sweep duration over the frame interval), zero until a pair has been registered and where the
    motion is over the caps.  With `prefetch` a frame is submitted before the frame in front of it is registered, so
    that transform is one frame older.
    `pixel_format`: a PIXEL_* format for the generator: the colour images `frames` yields are then packed in it (both of a
    stereo pair); None leaves the generator as it is.
    `lidar`: a Lidar for the generator: `frames` then yields (name, bgr, points), a colour image and a scan (n x k
    float32, x y z first), and the depth comes from the scan projected on the device; None leaves the generator as it is.
    `stereo`: a Stereo for the generator: `frames` then yields (name, left, right), two colour images of a rectified
    pair, and the depth comes from the matcher on the device; None leaves the generator as it is and takes depth frames.
    `stereo_rig`: a StereoRig for the generator, beside `stereo`: the pairs are then RAW and are rectified on the
    device (`dataset_seq` is ignored: the rig is the camera); None leaves the generator as it is.
    `stereo_paths`: a path mask for the generator's matcher (PATHS_4, PATHS_8, ...); None leaves the generator as it is.
    `stereo_speckle`: a Speckle for the generator's matcher; None leaves the generator as it is.
    `select_mode`: SELECT_IMAGE or SELECT_DEPTH for the generator's selector; None leaves the generator as it is.
    `depth_median`: a DepthMedian for the generator, for frames of either kind; None leaves the generator as it is.
    `depth_infill`: a DepthInfill for the generator, for frames of every kind; None leaves the generator as it is.
    `camera`: a CameraModel for the generator (`dataset_seq` is then ignored); None leaves the
    generator as it is -- a new one uses the table.
    `depth_camera`: a DepthCamera for the generator: the frames' depth images are then of its size and
    are registered to colour on the device; None leaves the generator as it is.
    `depth_gate`: a DepthGate for the generator; `mask`: an h x w mask for it, one for all frames (a caller with
    a mask per frame drives the generator itself); None leaves the generator as it is.
    `device`: the cloud goes from the front end to the registration in device memory
    (cvo_fe_collect_device -> cvo_hip_set_*_device) instead of through host arrays.
    `prefetch`: frame k+1 is in the front end (its own, low-priority stream) while frame k
    is being registered; the results are the same either way.  Off by default: measured on
    MI355X it is worth +4-5 % per frame in a process that has little else on the GPU's queues
    and -5 % in one that has (bench.py, after the batched legs).  Returns the number of frames."""
    ftype = FEATURES_HSV if registration.params.mode == capi.MODE_ACVO else FEATURES_RGB
    gen = generator
    it = iter(frames)
    count = 0
    cur = next(it, None)
    if cur is None:
        return 0
    if input_binning is not None:
        f = int(input_binning.factor)
        if gen is None:
            if f < 1 or cur[1].shape[0] % f or cur[1].shape[1] % f:
                raise ValueError("input_binning: the first frame's shape %r is no multiple of the factor" % (cur[1].shape[:2],))
            gen = PcdGenerator(cur[1].shape[1] // f, cur[1].shape[0] // f)
        gen.set_input_binning(input_binning)
        if stereo_rig is not None:
            stereo_rig = bin_stereo_rig(stereo_rig, f)
        elif camera is not None:
            camera = bin_camera(camera, f)
        else:   # (the table row, as a model of the input images)
            row = _table_row(dataset_seq)
            camera = bin_camera(CameraModel(row["scaling_factor"], row["fx"], row["fy"], row["cx"], row["cy"]), f)
    if gen is None:
        gen = PcdGenerator(cur[1].shape[1], cur[1].shape[0])
    if camera is not None:
        gen.set_camera(camera)
    if depth_camera is not None:
        gen.set_depth_camera(depth_camera)
    if depth_gate is not None:
        gen.set_depth_gate(depth_gate)
    if mask is not None:
        gen.set_mask(mask)
    if stereo is not None:
        gen.set_stereo(stereo)
    if stereo_rig is not None:
        gen.set_stereo_rig(stereo_rig)
    if stereo_paths is not None:
        gen.set_stereo_paths(stereo_paths)
    if stereo_speckle is not None:
        gen.set_stereo_speckle(stereo_speckle)
    if select_mode is not None:
        gen.set_select_mode(select_mode)
    if depth_median is not None:
        gen.set_depth_median(depth_median)
    if depth_infill is not None:
        gen.set_depth_infill(depth_infill)
    if pixel_format is not None:
        gen.set_pixel_format(pixel_format)
    if depth_format is not None:
        gen.set_depth_format(*(depth_format if isinstance(depth_format, (tuple, list)) else (depth_format,)))
    if lidar is not None:
        gen.set_lidar(lidar)
    if lidar_sweep is not None:
        gen.set_lidar_sweep(lidar_sweep)
    if device_input and lidar is not None:
        raise ValueError("device_input: not for LiDAR frames (a scan is staged by the host)")
    if exposures is not None and photometric is None:
        photometric = Photometric(PHOTO_GAIN)
    if photometric is not None:   # (behind input_binning: the vignette is of the input size)
        gen.set_photometric(*(photometric if isinstance(photometric, (tuple, list)) else (photometric,)))
    if exposures is not None and not gen.photometric().flags & PHOTO_GAIN:
        raise ValueError("exposures: the Photometric must have PHOTO_GAIN")
    submit = gen.submit_stereo if stereo is not None else gen.submit_lidar if lidar is not None else gen.submit
    if device_input:
        submit = gen.submit_stereo_device if stereo is not None else gen.submit_device
    if lidar_motion is not None:
        if lidar_motion != "constant-velocity" and not callable(lidar_motion):
            raise ValueError('lidar_motion: None, a callable name -> twist, or "constant-velocity"')
        mount, inner = gen.lidar(), submit

        def submit(bgr, points, seq, ft, name=None):
            if callable(lidar_motion):
                gen.set_lidar_motion(lidar_motion(name))
            else:
                twist = np.zeros(6, np.float32)
                if registration.init:
                    try:
                        twist = lidar_twist(registration.transform, mount, sweep_fraction)
                    except capi.CvoHipError:
                        pass   # (over the caps: such a frame is not compensated)
                gen.set_lidar_motion(twist)
            inner(bgr, points, seq, ft)
    else:
        inner0 = submit

        def submit(bgr, points, seq, ft, name=None):
            inner0(bgr, points, seq, ft)
    if exposures is not None:
        exposed, frame_no = submit, [0]

        def submit(bgr, second, seq, ft, name=None):
            gen.set_photometric_gain(float(exposures[0]) / float(exposures[frame_no[0]]))
            frame_no[0] += 1
            exposed(bgr, second, seq, ft, name)
    gen.set_device_output(device)
    submit(cur[1], cur[2], dataset_seq, ftype, cur[0])
    while cur is not None:
        if device:
            d_xyz, d_feat, npts = gen.collect_device()
            nxt = next(it, None)
            first = not registration.init
            registration.set_pcd_device(d_xyz, d_feat, npts)   # (consumed: the next frame may overwrite it)
            if nxt is not None and prefetch:
                submit(nxt[1], nxt[2], dataset_seq, ftype, nxt[0])
            if not first:
                registration.align()
        else:
            xyz, feat = gen.collect()
            nxt = next(it, None)
            if nxt is not None and prefetch:
                submit(nxt[1], nxt[2], dataset_seq, ftype, nxt[0])
            registration.run_cvo(xyz, feat)
        if writer is not None and registration.init:
            writer.append(cur[0], registration.accum_transform)
        if nxt is not None and not prefetch:
            submit(nxt[1], nxt[2], dataset_seq, ftype, nxt[0])
        count += 1
        cur = nxt
    return count


def run_directory(registration, folder, dataset_seq, writer=None, assoc="assoc.txt", limit=None,
                  generator=None, camera=None, depth_camera=None, depth_gate=None, mask=None, select_mode=None,
                  depth_median=None, depth_infill=None, input_binning=None, photometric=None, exposures=None):
    """The reference's main loop (ref src/cvo_main.cpp:20-66, adaptive_cvo_main.cpp): every
    frame of `folder`/assoc goes through the front end and `run_cvo`; a pose line per
    frame is handed to `writer` (trajectory.TrajectoryWriter).  cvo uses the raw colour
    features, acvo the HSV ones (ref src/cvo.cpp:329, src/adaptive_cvo.cpp:451).  `camera`: as in
    run_frames, e.g. TUM_CAMERAS["fr1"] for a freiburg1 sequence with its lens distortion removed.
    `depth_camera`: as in run_frames, for a recording whose depth images are not registered to colour.
    `depth_gate`, `mask`: as in run_frames, e.g. DepthGate(0.8, 4.0, 0.05, 1) for a Kinect-class sensor.
    `select_mode`: as in run_frames, e.g. SELECT_DEPTH beside a gate, which removes the pixels the selector likes best.
    `depth_median`: as in run_frames, e.g. DepthMedian(1, 5) for a sensor with salt and pinholes.
    `depth_infill`: as in run_frames, e.g. DepthInfill(2, 2, 0.05) for the holes a depth camera's registration leaves.
    `input_binning`: as in run_frames, e.g. Binning(2, 2) for a 1280 x 720 recording worked on at 640 x 360.
    `photometric`, `exposures`: as in run_frames, e.g. Photometric(PHOTO_AUTO) for a recording under auto exposure."""
    names, rgbs, deps = load_file_name(os.path.join(folder, assoc))
    if limit is not None:
        names, rgbs, deps = names[:limit], rgbs[:limit], deps[:limit]

    def decoded():
        for name, r, d in zip(names, rgbs, deps):
            bgr, depth = load_img(os.path.join(folder, r), os.path.join(folder, d))
            yield name, bgr, depth

    return run_frames(registration, decoded(), dataset_seq, writer=writer, generator=generator, camera=camera,
                      depth_camera=depth_camera, depth_gate=depth_gate, mask=mask, select_mode=select_mode,
                      depth_median=depth_median, depth_infill=depth_infill, input_binning=input_binning,
                      photometric=photometric, exposures=exposures)


def run_stereo_directory(registration, folder, dataset_seq, stereo, writer=None, left="image_2", right="image_3",
                         times="times.txt", limit=None, generator=None, camera=None, depth_gate=None, mask=None,
                         stereo_rig=None, stereo_paths=None, stereo_speckle=None, select_mode=None, depth_median=None,
                         depth_infill=None, input_binning=None, photometric=None, exposures=None):
    """run_directory() for the KITTI odometry layout: one line of `folder`/`times` per frame (the line is the frame's
    name), the pair in `folder`/`left`/%06d.png and `folder`/`right`/%06d.png, decoded by PIL as load_img does (B, G, R;
    a grey image is replicated).  `stereo`: the Stereo for the generator, e.g. Stereo(0.54, 128) with dataset_seq 4.
    `camera`, `depth_gate`, `mask`: as in run_frames.  `stereo_rig`: as in run_frames, for a raw recording (KITTI raw's
    image_02 / image_03 with the rig of its calib_cam_to_cam.txt).  `stereo_paths`, `stereo_speckle`, `select_mode`, `depth_median`,
    `depth_infill`, `input_binning`, `photometric`, `exposures`: as in run_frames."""
    with open(os.path.join(folder, times)) as fh:
        names = [line.strip() for line in fh if line.strip()]
    if limit is not None:
        names = names[:limit]

    def colour(path):
        from PIL import Image
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), np.uint8)[:, :, ::-1])

    def decoded():
        for k, name in enumerate(names):
            yield name, colour(os.path.join(folder, left, "%06d.png" % k)), colour(os.path.join(folder, right, "%06d.png" % k))

    return run_frames(registration, decoded(), dataset_seq, writer=writer, generator=generator, camera=camera,
                      depth_gate=depth_gate, mask=mask, stereo=stereo, stereo_rig=stereo_rig,
                      stereo_paths=stereo_paths, stereo_speckle=stereo_speckle, select_mode=select_mode,
                      depth_median=depth_median, depth_infill=depth_infill, input_binning=input_binning,
                      photometric=photometric, exposures=exposures)


def run_lidar_directory(registration, folder, dataset_seq, lidar, writer=None, image="image_2", scans="velodyne",
                        times="times.txt", limit=None, generator=None, camera=None, depth_gate=None, mask=None,
                        select_mode=None, depth_median=None, depth_infill=None, lidar_sweep=None, lidar_motion=None,
                        sweep_fraction=1.0, input_binning=None, photometric=None, exposures=None):
    """run_directory() for the KITTI odometry layout with its scans: one line of `folder`/`times` per frame (the line is
    the frame's name), the colour image in `folder`/`image`/%06d.png, decoded by PIL as load_img does (B, G, R; a grey
    image is replicated), and the scan in `folder`/`scans`/%06d.bin, records of four float32 (x y z reflectance).
    `lidar`: the Lidar for the generator, e.g. Lidar(130000, 1, R, T, occl_rel=0.25, occl_rx=7, occl_ry=1) with R, T of
    R_rect_00 * Tr_velo_to_cam and dataset_seq 4.  `camera`, `depth_gate`, `mask`, `select_mode`, `depth_median`: as in
    run_frames, e.g. SELECT_DEPTH and DepthMedian(1, 3) for a plane as sparse as a projected scan.  `depth_infill`: as in
    run_frames, e.g. DepthInfill(2, 8, 0.25) for scan lines some five rows apart.  `lidar_sweep`, `lidar_motion`,
    `sweep_fraction`: as in run_frames, e.g. LidarSweep(SWEEP_AZIMUTH, phase0=0.5, direction=1, s_ref=0.5) and
    "constant-velocity" for records that carry no time, as KITTI's: `direction` is the scanner's sense of rotation,
    `phase0` says at which azimuth its sweep begins and `s_ref` where in the sweep the image is taken.
    `input_binning`: as in run_frames (the colour image only; the scan is projected into the binned camera).
    `photometric`, `exposures`: as in run_frames."""
    with open(os.path.join(folder, times)) as fh:
        names = [line.strip() for line in fh if line.strip()]
    if limit is not None:
        names = names[:limit]

    def colour(path):
        from PIL import Image
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), np.uint8)[:, :, ::-1])

    def decoded():
        for k, name in enumerate(names):
            yield (name, colour(os.path.join(folder, image, "%06d.png" % k)),
                   np.fromfile(os.path.join(folder, scans, "%06d.bin" % k), np.float32).reshape(-1, 4))

    return run_frames(registration, decoded(), dataset_seq, writer=writer, generator=generator, camera=camera,
                      depth_gate=depth_gate, mask=mask, select_mode=select_mode, depth_median=depth_median, lidar=lidar,
                      depth_infill=depth_infill, lidar_sweep=lidar_sweep, lidar_motion=lidar_motion,
                      sweep_fraction=sweep_fraction, input_binning=input_binning, photometric=photometric,
                      exposures=exposures)
