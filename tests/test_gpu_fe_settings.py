"""GPU: the settings of a front-end context (every cvo_fe_set_* / cvo_fe_get_* of include/cvo_frontend.h), one table
for all of them, on the smallest context cvo_fe_create accepts (64 x 64): the protocol every setter and getter follow
(not set, set, the same again, another value, cleared, cleared again); every sentence with which a setter refuses a
call that neither runs out of memory nor fails in the runtime, as a whole string, and the setting unchanged behind it;
and no residue -- a context on which every setting was set and cleared makes the cloud of a new one, bit for bit, and
refuses to read the stages of a cleared setting as a new one does.  What each setting does to a frame is the business
of its own test_gpu_fe_*.py."""
import ctypes as C

import numpy as np
import pytest

from fe_gpu_common import _same_cloud

pytestmark = pytest.mark.gpu

W = H = 64
DIST = (0.2, -0.1, 0.001, 0.002, 0.05)


def _table(F):
    """Per setting: name (set_<name> / <name>), two valid values, one that is refused and the sentence, what must be
    set before it ((name, value), cleared behind it in reverse).  `default`: a plain setting -- it has no "not set", the
    getter gives this value on a new context and setting it again is its "clear"; the others are cleared by None."""
    pin = dict(fx=60.0, fy=60.0, cx=32.0, cy=32.0)
    lens = F.Lens(**pin)
    stereo = ("stereo", F.Stereo(baseline=0.1, max_disp=8))
    lidar = ("lidar", F.Lidar(max_points=16))
    sweep = ("lidar_sweep", F.LidarSweep(F.SWEEP_AZIMUTH, direction=1, phase0=0.25, s_ref=0.5))
    return [
        dict(name="camera", a=F.CameraModel(5000.0, **pin), b=F.CameraModel(5000.0, dist=DIST, **pin),
             bad=F.CameraModel(5000.0, 0.0, 60.0, 32.0, 32.0),
             sentence="set_camera: members must be finite and fx, fy, depth_scale positive"),
        dict(name="depth_camera", a=F.DepthCamera(8, 8, 5000.0, 8.0, 8.0, 4.0, 4.0),
             b=F.DepthCamera(16, 8, 5000.0, 8.0, 8.0, 4.0, 4.0, max_range=3.0),
             bad=F.DepthCamera(7, 8, 5000.0, 8.0, 8.0, 4.0, 4.0),
             sentence="set_depth_camera: size in [8, 8192], finite members, fx, fy, depth_scale positive, "
                      "max_range above min_range, R a rotation"),
        dict(name="depth_gate", a=F.DepthGate(0.5, 4.0, 0.05, 1, 0), b=F.DepthGate(0.5, 4.0, 0.05, 3, 1),
             bad=F.DepthGate(0.5, 4.0, 0.05, 4, 0),
             sentence="set_depth_gate: finite members, jump_rel >= 0, max_range above min_range, grow in [0, 3], "
                      "hole_border 0 or 1, pad_ 0"),
        dict(name="stereo", a=stereo[1], b=F.Stereo(baseline=0.2, max_disp=16), bad=F.Stereo(baseline=0.1, max_disp=12),
             sentence="set_stereo: baseline positive and finite, max_disp a multiple of 8 in [8, 128], min_disp >= 1, "
                      "1 <= p1 <= p2 <= 255, uniqueness in [0, 99], lr_max in [-1, 8], pad_ 0"),
        dict(name="stereo_paths", default=F.PATHS_4, a=F.PATHS_8, b=0x33, bad=0,
             sentence="set_stereo_paths: a non-empty subset of the eight bits, 1 <= mask <= 0xFF"),
        dict(name="stereo_speckle", a=F.Speckle(10, 4), b=F.Speckle(20, 0), bad=F.Speckle(0, 4),
             sentence="set_stereo_speckle: max_size in [1, 2^26], max_diff in [0, 65535]"),
        dict(name="depth_median", a=F.DepthMedian(1, 0), b=F.DepthMedian(2, 3), bad=F.DepthMedian(3, 0),
             sentence="set_depth_median: radius 1 or 2, fill_min in [0, (2*radius+1)^2 - 1], pad_ 0"),
        dict(name="depth_infill", a=F.DepthInfill(3, 3, 0.1), b=F.DepthInfill(5, 0, 0.0), bad=F.DepthInfill(16, 0, 0.0),
             sentence="set_depth_infill: gap_x in [0, 15], gap_y in [0, 31], jump_rel finite and >= 0, pad_ 0"),
        dict(name="lidar", a=lidar[1], b=F.Lidar(max_points=16, splat=1, occl_rel=0.25, occl_rx=1, occl_ry=1),
             bad=F.Lidar(max_points=0),
             sentence="set_lidar: max_points in [1, 2^21], splat in [0, 3], finite members, occl_rel >= 0, occl_rx and "
                      "occl_ry in [0, 7], max_range above min_range, R a rotation, pad_ 0"),
        dict(name="lidar_sweep", needs=[lidar], a=sweep[1], b=F.LidarSweep(F.SWEEP_TIME_F32, time_offset=12, time_scale=1.0),
             bad=F.LidarSweep(F.SWEEP_AZIMUTH, direction=0),
             sentence="set_lidar_sweep: a mode of CVO_FE_SWEEP_*, finite members, time_offset >= 12 and a multiple of 4, "
                      "time_scale not 0, direction +1 or -1 under the azimuth mode and 0 otherwise, phase0 in [0, 1), "
                      "s_ref in [0, 1], time_origin 0 outside the float mode, pad_ 0"),
        dict(name="lidar_motion", needs=[lidar, sweep], default=(0.0,) * 6, a=(0.125, 0.0, 0.0, 1.0, 0.0, 0.0),
             b=(0.0, 0.25, 0.0, 0.0, -2.0, 0.0), bad=(2.0, 0.0, 0.0, 0.0, 0.0, 0.0),
             sentence="set_lidar_motion: finite members, |w| <= 1 radian and |v| <= 64 metres per sweep"),
        dict(name="stereo_rig", needs=[stereo], a=F.StereoRig(lens, lens, baseline=0.1, depth_scale=1000.0, **pin),
             b=F.StereoRig(lens, lens, baseline=0.2, depth_scale=1000.0, **pin),
             bad=F.StereoRig(lens, lens, baseline=0.0, depth_scale=1000.0, **pin),
             sentence="set_stereo_rig: finite members, every fx, fy, depth_scale and baseline positive, R_left and R_right "
                      "rotations"),
        dict(name="select_mode", default=F.SELECT_IMAGE, a=F.SELECT_DEPTH, b=F.SELECT_IMAGE, bad=2,
             sentence="set_select_mode: CVO_FE_SELECT_IMAGE or CVO_FE_SELECT_DEPTH"),
        dict(name="pixel_format", default=F.PIXEL_BGR8, a=F.PIXEL_YUY2, b=F.PIXEL_GREY8, bad=99,
             sentence="set_pixel_format: a CVO_FE_PIXEL_* format that fits the context's size (YUY2, UYVY: an even width; "
                      "NV12: an even width and height)"),
        dict(name="depth_format", default=(F.DEPTH_U16, 1.0), a=(F.DEPTH_F32, 1.0), b=(F.DEPTH_F16, 0.5),
             bad=(F.DEPTH_U16, 2.0),
             sentence="set_depth_format: a CVO_FE_DEPTH_* format, a finite unit in [2^-20, 2^20], and a unit of 1 under "
                      "CVO_FE_DEPTH_U16"),
    ]


NAMES = ("camera", "depth_camera", "depth_gate", "stereo", "stereo_paths", "stereo_speckle", "depth_median", "depth_infill",
         "lidar", "lidar_sweep", "lidar_motion", "stereo_rig", "select_mode", "pixel_format", "depth_format")


def _set(gen, name, value):
    if name == "depth_format":
        gen.set_depth_format(*value)
    else:
        getattr(gen, "set_" + name)(value)


def _get(gen, name):
    got = getattr(gen, name)()
    return tuple(float(v) for v in got) if name == "lidar_motion" else got


def _unset(s):
    return s.get("default")   # (None: "not set")


def _last_error(pkg, gen):
    return pkg.frontend.lib().cvo_fe_last_error(gen._h).decode()


def _refused(pkg, gen, call, sentence):
    with pytest.raises(pkg.capi.CvoHipError):
        call()
    assert _last_error(pkg, gen) == sentence


def _state(pkg, gen):
    return [(n, _get(gen, n)) for n in NAMES]


def _generator(pkg):
    return pkg.frontend.PcdGenerator(W, H, num_want=W * H // 8)


def _frame(pkg):
    return pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=11, texture=1.0)


def _mask():
    m = np.zeros((H, W), np.uint8)
    m[8:24, 8:40] = 1
    return m


@pytest.mark.parametrize("name", NAMES)
def test_protocol(pkg, name):
    table = _table(pkg.frontend)
    assert tuple(s["name"] for s in table) == NAMES
    s = table[NAMES.index(name)]
    gen = _generator(pkg)
    for n, v in s.get("needs", []):
        _set(gen, n, v)
    unset = _unset(s)
    assert _get(gen, name) == unset
    _set(gen, name, s["a"])
    assert _get(gen, name) == s["a"]
    _set(gen, name, s["a"])
    assert _get(gen, name) == s["a"]
    _set(gen, name, s["b"])
    assert _get(gen, name) == s["b"]
    _refused(pkg, gen, lambda: _set(gen, name, s["bad"]), s["sentence"])   # the invalid-value sentence
    assert _get(gen, name) == s["b"]
    _set(gen, name, unset)
    assert _get(gen, name) == unset
    _set(gen, name, unset)
    assert _get(gen, name) == unset
    gen.close()


def test_protocol_mask(pkg):
    """the mask has no getter: every call of the protocol is accepted, and the one refusal leaves a frame possible"""
    F = pkg.frontend
    gen = _generator(pkg)
    gen.set_mask(None)
    gen.set_mask(_mask())
    gen.set_mask(_mask())
    gen.set_mask(_mask().T.copy() != 0)
    m = _mask()
    st = F.lib().cvo_fe_set_mask(gen._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), W - 1)
    assert st != 0 and _last_error(pkg, gen) == "set_mask: stride below the width"
    bgr, dep = _frame(pkg)
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert np.array_equal(gen.read_stage(F.STAGE_GATE) != 0, (_mask().T != 0) & (dep != 0))
    gen.set_mask(None)
    gen.set_mask(None)
    gen.close()


def test_in_flight(pkg):
    """each setter refuses while a frame is submitted and not collected, and changes nothing"""
    F = pkg.frontend
    gen = _generator(pkg)
    bgr, dep = _frame(pkg)
    fresh = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    before = _state(pkg, gen)
    gen.submit(bgr, dep, 1, F.FEATURES_RGB)
    for s in _table(F):
        if s["name"] == "lidar_motion":   # (read by the next submit, no graph holds it: it does not ask)
            continue
        _refused(pkg, gen, lambda: _set(gen, s["name"], s["a"]), "set_%s: a frame is in flight" % s["name"])
    _refused(pkg, gen, lambda: gen.set_mask(_mask()), "set_mask: a frame is in flight")
    _refused(pkg, gen, lambda: gen.set_device_output(True), "set_device_output: a frame is in flight")
    assert _state(pkg, gen) == before
    assert _same_cloud(gen.collect(), fresh)
    gen.close()


def _exclusions(F):
    """(what is set first, the refused call, its sentence): the exclusions between settings, in both directions"""
    t = {s["name"]: s for s in _table(F)}
    a = lambda n: (n, t[n]["a"])
    bent = ("camera", t["camera"]["b"])
    return [
        ([a("depth_camera")], a("stereo"), "set_stereo: a depth camera is set"),
        ([a("stereo")], a("depth_camera"), "set_depth_camera: stereo is set, there is no depth image"),
        ([a("lidar")], a("stereo"), "set_stereo: a scan source is set"),
        ([a("stereo")], a("lidar"), "set_lidar: stereo is set"),
        ([a("depth_camera")], a("lidar"), "set_lidar: a depth camera is set"),
        ([a("lidar")], a("depth_camera"), "set_depth_camera: a scan source is set, there is no depth image"),
        ([bent], a("stereo"), "set_stereo: the camera model has a lens distortion; the pair must be rectified"),
        ([a("stereo")], bent, "set_camera: stereo is set and takes a rectified pair: dist must be zero"),
        ([], a("stereo_rig"), "set_stereo_rig: stereo is not set (cvo_fe_set_stereo)"),
        ([a("stereo"), a("camera")], a("stereo_rig"),
         "set_stereo_rig: a camera model is set; the rig is the camera: clear the model first"),
        ([a("stereo"), a("stereo_rig")], a("camera"), "set_camera: a stereo rig is set and is the camera: clear the rig first"),
        ([a("stereo"), a("stereo_rig")], ("stereo", None), "set_stereo: a stereo rig is set: clear the rig first"),
        ([], a("lidar_sweep"), "set_lidar_sweep: no scan source (cvo_fe_set_lidar)"),
        ([a("lidar")], a("lidar_motion"), "set_lidar_motion: no sweep (cvo_fe_set_lidar_sweep)"),
    ]


@pytest.mark.parametrize("k", range(14))
def test_exclusion(pkg, k):
    first, (name, value), sentence = _exclusions(pkg.frontend)[k]
    gen = _generator(pkg)
    for n, v in first:
        _set(gen, n, v)
    before = _state(pkg, gen)
    _refused(pkg, gen, lambda: _set(gen, name, value), sentence)
    assert _state(pkg, gen) == before
    gen.close()


def test_motion_without_a_twist(pkg):
    F = pkg.frontend
    t = {s["name"]: s for s in _table(F)}
    gen = _generator(pkg)
    _set(gen, "lidar", t["lidar"]["a"])
    _set(gen, "lidar_sweep", t["lidar_sweep"]["a"])
    _set(gen, "lidar_motion", t["lidar_motion"]["a"])
    assert F.lib().cvo_fe_set_lidar_motion(gen._h, None) != 0
    assert _last_error(pkg, gen) == "set_lidar_motion: bad argument"
    assert _get(gen, "lidar_motion") == t["lidar_motion"]["a"]
    gen.close()


def test_no_residue(pkg):
    F = pkg.frontend
    bgr, dep = _frame(pkg)
    new = _generator(pkg)
    fresh = new.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert len(fresh[0]) > 0
    gen = _generator(pkg)
    for s in _table(F):
        for n, v in s.get("needs", []):
            _set(gen, n, v)
        _set(gen, s["name"], s["a"])
        _set(gen, s["name"], s["b"])
        _set(gen, s["name"], _unset(s))
        for n, _ in reversed(s.get("needs", [])):
            _set(gen, n, None)
    gen.set_mask(_mask())
    gen.set_mask(None)
    assert _state(pkg, gen) == _state(pkg, new)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), fresh)
    assert gen.info() == new.info()
    refusals = []
    for stage in (F.STAGE_RIGHT_GRAY, F.STAGE_SGM_SUM, F.STAGE_STEREO_VALID, F.STAGE_SPECKLE_SIZE, F.STAGE_UNFILTERED_DEPTH,
                  F.STAGE_MEDIAN, F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR, F.STAGE_SPARSE_DEPTH, F.STAGE_INFILL, F.STAGE_INPUT_BGR,
                  F.STAGE_INPUT_RIGHT_BGR):
        said = []
        for g in (new, gen):
            with pytest.raises(pkg.capi.CvoHipError):
                g.read_stage(stage)
            said.append(_last_error(pkg, g))
        assert said[0] == said[1] and said[0].startswith("read_stage: ")
        refusals.append(said[0])
    assert len(set(refusals)) == 5   # stereo, the median filter, a scan source, the infill stage, an unpacked image
    assert not np.any(gen.read_stage(F.STAGE_GATE)) and not np.any(new.read_stage(F.STAGE_GATE))
    gen.close()
    new.close()
