"""GPU: a depth camera of its own in the front end (cvo_fe_set_depth_camera,
include/cvo_frontend.h): k_fe_depth_warp / k_fe_depth_final against the numpy restatement of
the registration contract (tests/fe_depth_ref.py) by bytes and, downstream of them, the CPU
restatement of the front end (oracle/frontend_oracle.c) applied to the reference-registered
depth: every cloud bit for bit.  The rectified colour frame as the target, the unchanged path
without a rig, the captured graphs across changes of rig and camera, the Python and C++
layers above, and the refusals."""
import io

import numpy as np
import pytest

import fe_depth_ref as D
import fe_rectify_ref as R
from conftest import low_texture_frame
from fe_gpu_common import _demo_lines, _device_path_lines, _four_frames, _pose_line_f32, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
_REG = {}


def _reg(key, rig, cam, w, h, dep):
    """The reference-registered depth of a frame, computed once per key and left unchanged."""
    if key not in _REG:
        out = D.register(rig, cam, w, h, dep)
        out.setflags(write=False)
        _REG[key] = out
    return _REG[key]


def _generator(pkg, name):
    F = pkg.frontend
    w, h, cam, rig = D.RIGS[name]
    gen = F.PcdGenerator(w, h, num_want=max(200, w * h // 100))
    gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
    gen.set_depth_camera(D.to_struct(F, rig))
    return gen


# ---- 1. the registered image by bytes ------------------------------------------------------

@pytest.mark.parametrize("name", ["K", "U", "D", "C", "W", "I", "I127x193"])
def test_registered_depth_by_bytes(pkg, name):
    F = pkg.frontend
    w, h, cam, rig = D.RIGS[name]
    gen = _generator(pkg, name)
    assert gen.depth_camera() == D.to_struct(F, rig)
    for seed, kw in ((72, {}), (73, {"holes": 0.2})):
        bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=1.0)
        dep = D.scene(pkg.data, rig, seed=seed, **kw)
        want = _reg((name, seed), rig, cam, w, h, dep)
        gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        raw = gen.read_stage(F.STAGE_RAW_DEPTH)
        assert raw.shape == (rig["height"], rig["width"]) and np.array_equal(raw, dep), "the depth image as uploaded"
        got = gen.read_stage(F.STAGE_RECT_DEPTH)
        assert got.shape == (h, w) and got.tobytes() == want.tobytes(), "registered depth"
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), bgr)
        if name.startswith("I"):
            assert np.array_equal(got, dep)
        else:
            assert np.count_nonzero(want) > w * h // 10
    gen.close()


def test_raw_depth_stage_without_a_rig(pkg):
    F = pkg.frontend
    w, h, model = R.SMALL["A"]
    gen = F.PcdGenerator(w, h, num_want=200)
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), dep)
    gen.set_camera(F.CameraModel(*model))
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), dep)
    assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), R.rectify(model, bgr, dep)[1])
    gen.close()


def test_a_distorting_colour_model_is_the_target(pkg):
    """colour model A and rig K: colour goes through k_fe_rectify, depth straight into A's pinhole"""
    F = pkg.frontend
    w, h, model = R.SMALL["A"]
    _, _, _, rig = D.RIGS["K"]
    gen = F.PcdGenerator(w, h, num_want=200)
    gen.set_camera(F.CameraModel(*model))
    gen.set_depth_camera(D.to_struct(F, rig))
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    dep = D.scene(pkg.data, rig)
    want = _reg(("K into A", 72), rig, model[:5], w, h, dep)
    for _ in range(2):
        gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        qu, qv = R.rectify_map(model, w, h)
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), R.remap_colour(bgr, qu, qv))
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == want.tobytes()
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), dep)
    assert not np.array_equal(want, R.remap_depth(dep, qu, qv))
    assert not np.array_equal(want, _reg(("K", 72), rig, D.RIGS["K"][2], w, h, dep))
    # the rig cleared: k_fe_rectify resamples depth again
    gen.set_depth_camera(None)
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), R.remap_depth(dep, qu, qv))
    gen.close()


# ---- 2. the cloud by bits -------------------------------------------------------------------

def _vga_frame(pkg, kind):
    if kind == "low":
        bgr, dep = low_texture_frame(pkg)
    else:
        bgr, dep = pkg.data.synthetic_rgbd_frame(seed=72, texture=1.0)
    return bgr, np.ascontiguousarray(dep // 5)      # what a camera counting 1000 units per metre delivers


@pytest.mark.parametrize("kind", ["textured", "low"])
def test_cloud_by_bits(pkg, kind):
    """the table's row 1 beside a VGA Kinect-like depth camera: the oracle on the reference-registered depth"""
    F = pkg.frontend
    assert tuple(np.float32(v) for v in F.camera(1).values()) == tuple(np.float32(v) for v in D.VGA_COLOUR)
    gen = F.PcdGenerator(640, 480)
    gen.set_depth_camera(D.to_struct(F, D.VGA_RIG))
    bgr, dep = _vga_frame(pkg, kind)
    rd = _reg(("vga", kind), D.VGA_RIG, D.VGA_COLOUR, 640, 480, dep)
    assert not np.array_equal(rd, dep * 5) and np.count_nonzero(rd) > 640 * 480 // 2
    points = []
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
        xyz, feat = gen.create_pointcloud(bgr, dep, 1, ftype)
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == rd.tobytes()
        ref = fo.create_pointcloud(bgr, rd, 1, ftype)
        info = gen.info()
        assert info["num_selected"] == ref["num_selected"]
        assert info["num_points"] == len(ref["positions"]) == len(xyz)
        assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
        assert info["canny_used"] == (1 if kind == "low" else 0)   # (the top-up re-emits from the registered depth)
        points.append(len(xyz))
    assert points[0] == points[1] > 100
    gen.close()


def test_identity_rig_gives_the_cloud_of_no_rig(pkg):
    F = pkg.frontend
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=72, texture=1.0)
    gen = F.PcdGenerator(640, 480)
    want = {ft: gen.create_pointcloud(bgr, dep, 1, ft) for ft in (F.FEATURES_RGB, F.FEATURES_HSV)}
    gen.set_depth_camera(D.to_struct(F, D.identity_rig(640, 480, D.VGA_COLOUR)))
    for ft, cloud in want.items():
        assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, ft), cloud) and len(cloud[0]) > 1000
        assert np.array_equal(gen.read_stage(F.STAGE_RECT_DEPTH), dep)
    gen.close()


# ---- 3. graphs and order --------------------------------------------------------------------

def test_changes_of_rig_on_one_context(pkg):
    """rig K, no rig (and the table), rig D (another depth size), rig K again beside a distorting colour
    model, on ONE context, through every way of taking a frame: each cloud is the one a fresh context gives"""
    F = pkg.frontend
    w, h, nw = 96, 64, 200
    cc = F.CameraModel(*(D.COLOUR[(w, h)] + (ZERO,)))
    rig_k, rig_d = D.to_struct(F, D.RIGS["K"][3]), D.to_struct(F, D.RIGS["D"][3])
    bgr, plain = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=74, texture=1.0)
    dep_k, dep_d = D.scene(pkg.data, D.RIGS["K"][3], seed=74), D.scene(pkg.data, D.RIGS["D"][3], seed=74)
    states = [(rig_k, cc, dep_k), (None, None, plain), (rig_d, cc, dep_d), (rig_k, F.CameraModel(*R.SMALL["A"][2]), dep_k),
              (rig_k, cc, dep_k)]
    ftype = F.FEATURES_HSV
    want = []
    for rig, cam, dep in states[:4]:
        fresh = F.PcdGenerator(w, h, num_want=nw)
        fresh.set_camera(cam)
        fresh.set_depth_camera(rig)
        want.append(fresh.create_pointcloud(bgr, dep, 1, ftype))
        fresh.close()
    want.append(want[0])
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(want[a][0], want[b][0])
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
        for rounds in range(2):
            for (rig, cam, dep), cloud in zip(states, want):
                if rounds:                               # (either order of the two changes)
                    gen.set_depth_camera(rig); gen.set_camera(cam)
                else:
                    gen.set_camera(cam); gen.set_depth_camera(rig)
                assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, ftype), cloud)
                gen.submit(bgr, dep, 1, ftype)
                assert _same_cloud(gen.collect(), cloud)
                img, stage = gen.host_buffers()          # (the staging image follows the depth size)
                assert stage.shape == dep.shape
                img[:] = bgr; stage[:] = dep
                gen.submit(img, stage, 1, ftype)
                dp, df, n = gen.collect_device()
                assert n == len(cloud[0])
                canon.set_fixed_device(dp, df, n)
                got = canonical(n)
                canon.set_fixed(cloud[0], cloud[1])
                assert got == canonical(n)
    # a set or clear of the rig between submit and collect is refused; the frame in flight arrives intact
    gen.set_device_output(False)
    gen.set_camera(cc)
    gen.set_depth_camera(rig_k)
    gen.submit(bgr, dep_k, 1, ftype)
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_depth_camera(rig_d)
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_depth_camera(None)
    assert _same_cloud(gen.collect(), want[0])
    assert gen.depth_camera() == rig_k
    with pytest.raises(ValueError):
        gen.submit(bgr, dep_d, 1, ftype)                 # the depth image must be the rig's size
    gen.set_depth_camera(rig_d)                          # ... and the change is accepted afterwards
    assert _same_cloud(gen.create_pointcloud(bgr, dep_d, 1, ftype), want[2])
    canon.close()
    gen.close()


def test_twenty_repeats_give_the_same_bytes(pkg):
    F = pkg.frontend
    w, h, cam, rig = D.RIGS["U"]
    gen = _generator(pkg, "U")
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    dep = D.scene(pkg.data, rig)
    want = _reg(("U", 72), rig, cam, w, h, dep).tobytes()
    for _ in range(20):
        gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == want
    gen.close()


# ---- 4. the layers above --------------------------------------------------------------------

def _frames(pkg):
    return _four_frames(pkg, 75, lambda k, dep: np.ascontiguousarray(dep // 5))


def test_run_frames_with_a_depth_camera(pkg):
    """run_frames(depth_camera=rig) on the raw frames = run_frames without a rig on the reference-registered
    frames: the same poses"""
    F = pkg.frontend
    frames = _frames(pkg)
    reg_frames = [(name, bgr, _reg(("seq", k), D.VGA_RIG, D.VGA_COLOUR, 640, 480, dep))
                  for k, (name, bgr, dep) in enumerate(frames)]
    poses = []
    for fr, rig in ((frames, D.to_struct(F, D.VGA_RIG)), (reg_frames, None)):
        reg = pkg.Cvo()
        buf = io.StringIO()
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), depth_camera=rig) == 4
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close()
    assert poses[0][0] == poses[1][0] and len(poses[0][0].strip().split("\n")) == 4
    assert np.array_equal(poses[0][1], poses[1][1]) and poses[0][2] == poses[1][2] > 0


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_a_depth_camera(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_depth_camera / clear_depth_camera (tests/cpp/cvo_depth_camera_demo.cpp):
    the clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    # frame 2 goes without a rig: a depth image of the colour size, registered already; the others come from a
    # depth camera of half the size
    frames = [(name, bgr, np.ascontiguousarray(dep * 5 if k == 2 else dep[::2, ::2]))
              for k, (name, bgr, dep) in enumerate(_frames(pkg))]
    small = dict(D.VGA_RIG, width=320, height=240, fx=290.0, fy=290.0, cx=156.75, cy=125.75)
    rig = D.to_struct(F, small)
    got = _demo_lines(tmp_path, "cvo_depth_camera_demo", frames, w, h, bytes(rig), [mode_name], depth_sizes=True)
    gen = F.PcdGenerator(w, h)

    def prepare(k):
        gen.set_depth_camera(None if k == 2 else rig)
        return ["refused a reflection"] if k == 3 else []

    want, sizes, poses = _device_path_lines(pkg, mode_name, gen, frames, prepare)
    assert got == ["refused a reflection"] + want
    # ... whose pose lines are the Python writer's up to the float64 of its quaternion
    for name, M in poses:
        line = _pose_line_f32(name, M)
        assert line in want
        buf = io.StringIO()
        pkg.trajectory.TrajectoryWriter(buf).append(name, M)
        assert buf.getvalue().split()[:4] == line.split()[:4]
        assert np.allclose([float(v) for v in buf.getvalue().split()[4:]], [float(v) for v in line.split()[4:]],
                           rtol=1e-5, atol=0)
    ftype = F.FEATURES_HSV if mode_name == "acvo" else F.FEATURES_RGB
    # the clouds of the rig's frames are the oracle's on the reference-registered depth (half-size depth: 2 x 2 footprints)
    rd = D.register(small, D.VGA_COLOUR, w, h, frames[0][2])
    assert sizes[0] == len(fo.create_pointcloud(frames[0][1], rd, 1, ftype)["positions"]) > 100
    gen.close()


# ---- 5. refusals ----------------------------------------------------------------------------

def test_refused_rigs_leave_the_context_usable(pkg):
    F = pkg.frontend
    w, h, cam, rig = D.RIGS["K"]
    gen = _generator(pkg, "K")
    good = D.to_struct(F, rig)
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    dep = D.scene(pkg.data, rig)
    want = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert len(want[0]) > 20
    bad = [D.to_struct(F, r) for r in D.bad_rigs()]
    for m in bad:
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_camera(m)
        assert gen.depth_camera() == good
        assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    # ... also on a context that never had a rig: it stays without one, its depth image of the colour size (memory is
    # not observed here: these buffers are below what a reading of free memory resolves; see the test below)
    fresh = F.PcdGenerator(w, h, num_want=200)
    _, plain = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    table = fresh.create_pointcloud(bgr, plain, 1, F.FEATURES_RGB)
    for m in bad:
        with pytest.raises(pkg.capi.CvoHipError):
            fresh.set_depth_camera(m)
    assert fresh.depth_camera() is None and fresh.host_buffers()[1].shape == (h, w)
    assert _same_cloud(fresh.create_pointcloud(bgr, plain, 1, F.FEATURES_RGB), table)
    fresh.set_depth_camera(None)                           # clearing what was never set is no error
    fresh.close(); gen.close()


def test_a_refused_rig_takes_no_memory(pkg):
    """A rig of 8192 x 8192 that is refused for its R alone: accepted, it would take 128 MiB of raw depth and 512 MiB
    of rays on the device and 128 MiB of pinned memory; refused on a context that never had a rig, the free device
    memory stays where it was, to the 8 MiB such a reading resolves."""
    import torch
    F = pkg.frontend
    gen = F.PcdGenerator(640, 480)
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=72, texture=1.0)
    table = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    big = dict(D.VGA_RIG, width=8192, height=8192)
    assert F.check_depth_camera(D.to_struct(F, big))
    bad = [D.to_struct(F, dict(big, R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0))),
           D.to_struct(F, dict(big, min_range=2.0, max_range=1.0)), D.to_struct(F, dict(big, width=8193))]
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for m in bad:
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_camera(m)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 1024 * 1024, "a refused rig took %d bytes" % (free0 - free1)
    assert gen.depth_camera() is None and gen.host_buffers()[1].shape == (480, 640)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), table)
    gen.close()
