"""GPU: a caller's camera model in the front end (cvo_fe_set_camera, include/cvo_frontend.h):
k_fe_rectify against the numpy restatement of the rectification contract
(tests/fe_rectify_ref.py) and, downstream of it, the CPU restatement of the front end
(oracle/frontend_oracle.c) applied to the reference-rectified pair: every image and every
cloud bit for bit.  Custom intrinsics, the unchanged table path, the captured graphs across
changes of camera, the Python and C++ layers above, and the refusals."""
import io

import numpy as np
import pytest

import fe_rectify_ref as R
from conftest import low_texture_frame
from fe_gpu_common import _bits, _demo_lines, _digest, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
_RECT = {}


def _rect(key, model, bgr, dep):
    """The reference-rectified pair of a frame, computed once per (key) and left unchanged."""
    if key not in _RECT:
        rb, rd = R.rectify(model, bgr, dep)
        rb.setflags(write=False); rd.setflags(write=False)
        _RECT[key] = (rb, rd)
    return _RECT[key]


def _check_stages(pkg, gen, model, bgr, dep, key):
    F = pkg.frontend
    rb, rd = _rect(key, model, bgr, dep)
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), rb), "rectified colour"
    assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), rd), "rectified depth"
    g = fo.gray(rb)
    assert np.array_equal(gen.read_stage(F.STAGE_GRAY), g)
    assert np.array_equal(gen.read_stage(F.STAGE_HSV), fo.hsv(rb))
    _, dx0, dy0, _ = fo.pyramid(g)
    assert np.array_equal(_bits(gen.read_stage(F.STAGE_DX0)), _bits(dx0))
    assert np.array_equal(_bits(gen.read_stage(F.STAGE_DY0)), _bits(dy0))


# ---- 1. stages by bits ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_small_models_stages_by_bits(pkg, name):
    """96 x 64 (a multiple of four) with maps that leave the image, 127 x 193 (odd: the last
    group of pixels goes one by one) with shifts of 30 px"""
    w, h, model = R.SMALL[name]
    gen = pkg.frontend.PcdGenerator(w, h, num_want=max(200, w * h // 100))
    gen.set_camera(pkg.frontend.CameraModel(*model))
    for texture, seed in ((1.0, 61), (3.0, 62)):
        bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=texture)
        _check_stages(pkg, gen, model, bgr, dep, (name, seed))
    gen.close()


def test_fr1_vga_stages_by_bits(pkg):
    gen = pkg.frontend.PcdGenerator(640, 480)
    gen.set_camera(pkg.frontend.TUM_CAMERAS["fr1"])
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=63, texture=1.0)
    _check_stages(pkg, gen, R.FR1, bgr, dep, ("fr1", 63))
    rb, rd = _RECT[("fr1", 63)]
    assert np.count_nonzero(rb != bgr) > bgr.size // 2          # (the pass did something)
    assert not rd[0, 0] and dep[0, 0]                          # the corners look outside the image
    gen.close()


# ---- 2. the cloud by bits ---------------------------------------------------------------

def _check_cloud(pkg, gen, bgr, dep, key, ftype, num_want):
    """fr1 = the table's row 1 plus the lens: the oracle with dataset_seq 1 on the rectified pair"""
    rb, rd = _rect(key, R.FR1, bgr, dep)
    xyz, feat = gen.create_pointcloud(bgr, dep, 1, ftype)
    ref = fo.create_pointcloud(rb, rd, 1, ftype, num_want)
    info = gen.info()
    assert info["num_selected"] == ref["num_selected"]
    assert info["num_points"] == len(ref["positions"]) == len(xyz)
    assert np.array_equal(gen.read_stage(pkg.frontend.STAGE_MAP), ref["map"])
    assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
    return info


@pytest.mark.parametrize("w,h,num_want", [(96, 64, 200), (640, 480, 3000)])
def test_cloud_by_bits(pkg, w, h, num_want):
    F = pkg.frontend
    assert F.CameraModel(*(tuple(F.camera(1).values()) + (R.FR1[5],))) == F.TUM_CAMERAS["fr1"]
    gen = F.PcdGenerator(w, h, num_want=num_want)
    gen.set_camera(F.TUM_CAMERAS["fr1"])
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=64, texture=1.0)
    seen = [_check_cloud(pkg, gen, bgr, dep, ("cloud", w, 64), ftype, num_want)
            for ftype in (F.FEATURES_RGB, F.FEATURES_HSV)]
    assert seen[0]["num_points"] == seen[1]["num_points"] > num_want // 10
    gen.close()


def test_canny_top_up_runs_on_the_rectified_image(pkg):
    F = pkg.frontend
    gen = F.PcdGenerator(640, 480)
    gen.set_camera(F.TUM_CAMERAS["fr1"])
    bgr, dep = low_texture_frame(pkg)
    info = _check_cloud(pkg, gen, bgr, dep, ("low", 6), F.FEATURES_RGB, 3000)
    assert info["canny_used"] == 1
    rb, _ = _RECT[("low", 6)]
    assert np.array_equal(gen.read_stage(F.STAGE_EDGES), fo.canny(fo.blur3(fo.gray(rb))))
    gen.close()


# ---- 3. custom intrinsics without an oracle ---------------------------------------------

def test_custom_intrinsics_without_distortion(pkg):
    F = pkg.frontend
    model = F.CameraModel(1000.0, 400.25, 399.5, 300.75, 250.125, ZERO)
    gen = F.PcdGenerator(640, 480)
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=65, texture=1.0)
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
        gen.set_camera(None)
        xyz_t, feat_t = gen.create_pointcloud(bgr, dep, 1, ftype)
        map_t = gen.read_stage(F.STAGE_MAP)
        gen.set_camera(model)
        xyz, feat = gen.create_pointcloud(bgr, dep, 1, ftype)
        assert np.array_equal(gen.read_stage(F.STAGE_MAP), map_t)
        assert np.array_equal(_bits(feat), _bits(feat_t)) and len(xyz) == len(xyz_t) > 1000
        # no distortion: no rectification pass, the two new stages are the input images
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), bgr)
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), dep)
        ys, xs = np.nonzero((map_t != 0) & (dep != 0))
        f = np.float32
        z = dep[ys, xs].astype(np.float32) / f(1000.0)
        want = np.stack([((xs.astype(np.float32) - f(300.75)) * z) / f(400.25),
                         ((ys.astype(np.float32) - f(250.125)) * z) / f(399.5), z], axis=1)
        assert want.dtype == np.float32 and np.array_equal(_bits(xyz), _bits(want))
        assert not np.array_equal(xyz, xyz_t)
    gen.close()


# ---- 4. nothing changes without a model -------------------------------------------------

def test_table_path_is_unchanged(pkg):
    F = pkg.frontend
    gen = F.PcdGenerator(640, 480)
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=66, texture=1.0)
    assert gen.camera() is None
    want = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_HSV)
    info = gen.info()
    ref = fo.create_pointcloud(bgr, dep, 1, F.FEATURES_HSV)
    assert _same_cloud(want, (ref["positions"], ref["features"]))
    row1 = F.CameraModel(*(tuple(F.camera(1).values()) + (ZERO,)))
    gen.set_camera(row1)
    assert gen.camera() == row1
    for seq in (1, 4):                                   # dataset_seq is ignored while a model is set
        assert _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_HSV), want)
        assert gen.info() == info
    gen.set_camera(None)                                 # the table is back
    assert gen.camera() is None
    for seq in (2, 4):
        ref = fo.create_pointcloud(bgr, dep, seq, F.FEATURES_HSV)
        assert _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_HSV), (ref["positions"], ref["features"]))
    first = gen.create_pointcloud(bgr, dep, 0, F.FEATURES_HSV)
    for seq in (17, -3, 6):                              # out of the table: index 0
        assert _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_HSV), first)
    assert not np.array_equal(first[0], want[0])
    gen.close()


# ---- 5. graphs and order ----------------------------------------------------------------

def test_changes_of_camera_on_one_context(pkg):
    """fr1, no model, model B, fr1 again on ONE context, through every way of taking a frame:
    each cloud is the one a fresh context gives -- a graph captured for one camera is never
    launched for another, the map of one model never serves another"""
    F = pkg.frontend
    w, h, nw = 96, 64, 200
    cams = [F.TUM_CAMERAS["fr1"], None, F.CameraModel(*R.SMALL["B"][2]), F.TUM_CAMERAS["fr1"]]
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=67, texture=1.0)
    ftype = F.FEATURES_HSV
    want = []
    for cam in cams[:3]:
        fresh = F.PcdGenerator(w, h, num_want=nw)
        fresh.set_camera(cam)
        want.append(fresh.create_pointcloud(bgr, dep, 1, ftype))
        fresh.close()
    want.append(want[0])
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[2][0])
    assert min(len(c[0]) for c in want) > 20

    canon = pkg.capi.Context(mode=pkg.capi.MODE_ACVO)

    def canonical(n):
        """the live rows of the context's fixed cloud, sorted: whatever order the hand-over gave them"""
        d = canon.device_cloud(0)
        assert d["points"] == n
        rows = np.concatenate([d["pos"][:n], d["feat"][:n]], axis=1).view(np.uint32)
        return rows[np.lexsort(rows.T[::-1])].tobytes()

    gen = F.PcdGenerator(w, h, num_want=nw)
    for device_output in (False, True):
        gen.set_device_output(device_output)
        for rounds in range(2):                          # (per camera: one capture, then launches of that graph)
            for cam, cloud in zip(cams, want):
                gen.set_camera(cam)
                assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, ftype), cloud)
                gen.submit(bgr, dep, 1, ftype)
                assert _same_cloud(gen.collect(), cloud)
                gen.submit(bgr, dep, 1, ftype)
                dp, df, n = gen.collect_device()
                assert n == len(cloud[0])
                canon.set_fixed_device(dp, df, n)
                got = canonical(n)
                canon.set_fixed(cloud[0], cloud[1])
                assert got == canonical(n)
    # a change of camera between submit and collect is refused; the frame in flight arrives intact
    gen.set_device_output(False)
    gen.set_camera(cams[0])
    gen.submit(bgr, dep, 1, ftype)
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_camera(cams[2])
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_camera(None)
    assert _same_cloud(gen.collect(), want[0])
    assert gen.camera() == cams[0]
    gen.set_camera(cams[2])                              # ... and is accepted afterwards
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, ftype), want[2])
    canon.close()
    gen.close()


# ---- 6. the layers above ----------------------------------------------------------------

def test_run_frames_with_a_camera(pkg):
    """run_frames(camera=fr1) on the raw frames = run_frames(camera=fr1 without the lens) on the
    reference-rectified frames: the same poses"""
    F = pkg.frontend
    frames = _four_frames(pkg, 68)
    rect = [(name,) + _rect(("seq", k), R.FR1, bgr, dep) for k, (name, bgr, dep) in enumerate(frames)]
    pinhole = F.CameraModel(*(R.FR1[:5] + (ZERO,)))
    poses = []
    for fr, cam in ((frames, F.TUM_CAMERAS["fr1"]), (rect, pinhole)):
        reg = pkg.Cvo()
        buf = io.StringIO()
        assert F.run_frames(reg, fr, 3, writer=pkg.trajectory.TrajectoryWriter(buf), camera=cam) == 4
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close()
    assert poses[0][0] == poses[1][0] and len(poses[0][0].strip().split("\n")) == 4
    assert np.array_equal(poses[0][1], poses[1][1]) and poses[0][2] == poses[1][2] > 0
    # ... and not the poses of the raw frames through the table
    reg = pkg.Cvo()
    F.run_frames(reg, frames, 1)
    assert not np.array_equal(reg.accum_transform, poses[0][1])
    reg.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_a_camera(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_camera / clear_camera (tests/cpp/cvo_camera_demo.cpp): the
    clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    frames = _four_frames(pkg, 68)
    model = F.TUM_CAMERAS["fr1"]
    got = _demo_lines(tmp_path, "cvo_camera_demo", frames, w, h, bytes(model), [mode_name])
    acvo = mode_name == "acvo"
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    want = ["refused fx = 0"]
    sizes = []
    for k, (name, bgr, dep) in enumerate(frames):
        gen.set_camera(None if k == 2 else model)
        xyz, feat = gen.create_pointcloud(bgr, dep, 1, ftype)
        sizes.append(len(xyz))
        reg.run_cvo(xyz, feat)
        d = reg.ctx.device_cloud(0)
        assert d["points"] == len(xyz)
        want.append("cloud %s %d %d %d" % (name, len(xyz), _digest(d["pos"][:len(xyz)]), _digest(d["feat"][:len(xyz)])))
        buf = io.StringIO()
        pkg.trajectory.TrajectoryWriter(buf).append(name, reg.accum_transform)
        want.append(buf.getvalue().strip())
    want.append("points_last_frame %d iterations %d" % (sizes[-1], reg.num_iterations))
    assert got == want
    # the frames with the lens removed are other clouds than the table's would have been
    rb, rd = _rect(("seq", 0), R.FR1, frames[0][1], frames[0][2])
    assert sizes[0] == len(fo.create_pointcloud(rb, rd, 1, ftype)["positions"])
    reg.close(); gen.close()


# ---- 7. refusals -------------------------------------------------------------------------

def test_refused_models_leave_the_context_usable(pkg):
    F = pkg.frontend
    w, h, nw = 96, 64, 200
    gen = F.PcdGenerator(w, h, num_want=nw)
    good = F.CameraModel(*R.SMALL["A"][2])
    gen.set_camera(good)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=69, texture=1.0)
    want = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    bad = []
    for field, value in (("fx", float("nan")), ("cy", float("inf")), ("depth_scale", float("-inf")), ("fx", 0.0),
                         ("fy", 0.0), ("depth_scale", -5000.0), ("depth_scale", 0.0)):
        m = F.CameraModel(*R.SMALL["A"][2])
        setattr(m, field, value)
        bad.append(m)
    for k in (0, 4):
        m = F.CameraModel(*R.SMALL["A"][2])
        m.dist[k] = float("nan") if k == 0 else float("inf")
        bad.append(m)
    for m in bad:
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_camera(m)
        assert gen.camera() == good
        assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    # ... also on a context that never had a model: no memory is taken, the table stays
    fresh = F.PcdGenerator(w, h, num_want=nw)
    table = fresh.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    with pytest.raises(pkg.capi.CvoHipError):
        fresh.set_camera(bad[0])
    assert fresh.camera() is None and _same_cloud(fresh.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), table)
    fresh.close(); gen.close()
