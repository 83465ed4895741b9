"""GPU: a LiDAR scan in place of the depth image (cvo_fe_set_lidar, cvo_fe_submit_lidar, cvo_fe_project_points; the
LiDAR contract of include/cvo_frontend.h): k_fe_lidar_project and k_fe_lidar_cull of csrc/cvo_lidar.hip, with
k_fe_depth_final between them, against the restatement tests/fe_lidar_ref.py by bytes -- the plane, the plane before
culling, the flags and both counts on every scan made on purpose at every point of the grid, and the planes of frames
on a context -- and the cloud by bits against the CPU restatement of the front end (oracle/frontend_oracle.c) on the
colour image and the plane.  Counts alternating on one context, with and without captured graphs (a stale count or a
stale graph would show), settings changed between frames, the stages behind the plane, the refusals, the memory,
run_frames and the C++ objects above.  What the scans reach, and which errors they would show, is asserted in
tests/test_fe_lidar_cpu.py."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_gate_ref as G
import fe_lidar_ref as K
import fe_median_ref as KM
import fe_rectify_ref as R
from fe_gpu_common import ROOT, _demo_lines, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
SEQS = {(64, 64): 1, (96, 64): 4}          # the table row a frame of that size is taken under
FRAME_GRID = ((1, 7, 1, 0.25), (0, 0, 0, 0.0), (2, 3, 1, 0.25), (3, 0, 7, 0.25))


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _table(F, seq):
    return tuple(F.camera(seq).values())


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _stand_alone(F, points, s, cam, w, h, want, what):
    got = F.project_points(points, K.to_struct(F, s), cam, w, h)
    for k, part in enumerate(("P", "P0", "the flags")):
        _differ(got[k], want[k], "%s of %s" % (part, what))
    assert got[3:] == tuple(want[3:]), (what, got[3:], want[3:])


def _planes_equal(gen, F, want, final=None):
    """the stage's planes, and the plane every later stage read; without median and gate (final None) that is P"""
    P, P0, flags = want[:3]
    last = P if final is None else final
    for stage, plane, what in ((F.STAGE_LIDAR_DEPTH, P0, "P0"), (F.STAGE_LIDAR, flags, "the flags"), (F.STAGE_RAW_DEPTH, P, "P"),
                               (F.STAGE_RECT_DEPTH, last, "the plane every later stage read")):
        _differ(gen.read_stage(stage), plane, what)
    if final is None:
        _differ(gen.read_stage(F.STAGE_UNGATED_DEPTH), P, "the plane the gate would read")


def _cloud_equal(gen, F, cloud, bgr, depth, seq, ftype):
    """the cloud against the front-end oracle on the colour image and the plane the cloud is made from, by bits"""
    ref = fo.create_pointcloud(bgr, depth, seq, ftype, num_want=gen.num_want)
    info = gen.info()
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(cloud[0])
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud(cloud, (ref["positions"], ref["features"]))


def _lidar_frame(gen, F, bgr, points, s, seq, ftype=None):
    ftype = F.FEATURES_RGB if ftype is None else ftype
    h, w = bgr.shape[:2]
    want = K.lidar(points, s, _table(F, seq), w, h)
    cloud = gen.create_pointcloud_lidar(bgr, points, seq, ftype)
    _planes_equal(gen, F, want)
    _cloud_equal(gen, F, cloud, bgr, want[0], seq, ftype)
    return cloud, want


# ---- 1. the stand-alone entry on scans made on purpose -----------------------------------------------

@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_project_points_on_a_made_scan(pkg, name):
    """every made scan at both image sizes and every point of the grid: P, P0, the flags and both counts by bytes"""
    F = pkg.frontend
    for size in K.SIZES:
        for grid in K.GRID:
            points, s, cam, w, h, want = K.made(name, size, grid)
            _stand_alone(F, points, s, cam, w, h, want, (name, size, grid))
        print(name, size, "hits", want[3], "occluded", want[4])


@pytest.mark.parametrize("floats", [3, 4, 8], ids=["stride12", "stride16", "stride32"])
def test_project_points_takes_a_stride(pkg, floats):
    """records of 12, 16 and 32 bytes: what lies behind x y z is not read (it is NaN here), and a view with that row
    stride goes in without a copy"""
    F = pkg.frontend
    for name, grid in (("clutter-257", (1, 7, 1, 0.25)), ("skips", (0, 0, 0, 0.0)), ("clutter-4097", (2, 7, 7, 0.25))):
        points, s, cam, w, h, want = K.made(name, K.SIZES[1], grid)
        records = K.with_stride(points, floats)
        _stand_alone(F, records, s, cam, w, h, want, (name, floats))
        _stand_alone(F, records[:, :3], s, cam, w, h, want, (name, floats, "a view"))


def test_the_order_of_the_points_does_not_matter(pkg):
    F = pkg.frontend
    for name, grid in (("pile", (0, 0, 0, 0.0)), ("pile", (2, 7, 7, 0.25)), ("clutter-4097", (1, 3, 1, 0.25))):
        points, s, cam, w, h, want = K.made(name, K.SIZES[0], grid)
        for seed in (9, 10):
            _stand_alone(F, K.shuffled(points, seed), s, cam, w, h, want, (name, grid, seed))


@pytest.mark.parametrize("size", [(8192, 3), (3, 8192), (1, 1)], ids=["8192x3", "3x8192", "1x1"])
def test_project_points_at_the_size_limits(pkg, size):
    """the largest width, the largest height and one pixel; `unculled` and `flags` may be NULL"""
    F = pkg.frontend
    w, h = size
    s = K.setting((1, 7, 7, 0.25), **K.MOUNT)
    cam = (2000.0, 300.0, 300.0, w / 2.0, h / 2.0)
    points = K.scan_clutter(w, h, 3000, 21, s, cam)
    want = K.lidar(points, s, cam, w, h)
    assert want[3] >= min(w * h, 1000)
    _stand_alone(F, points, s, cam, w, h, want, size)
    plane, hits, occl = np.zeros((h, w), np.uint16), C.c_int(-1), C.c_int(-1)
    camf = np.asarray(cam, np.float32)
    rc = F.lib().cvo_fe_project_points(0, points.ctypes.data, 12, len(points), C.byref(K.to_struct(F, s)),
                                       camf.ctypes.data_as(C.POINTER(C.c_float)), w, h, plane.ctypes.data_as(C.POINTER(C.c_uint16)),
                                       None, None, C.byref(hits), C.byref(occl))
    assert rc == 0 and plane.tobytes() == want[0].tobytes() and (hits.value, occl.value) == tuple(want[3:])


# ---- 2. frames on a context --------------------------------------------------------------------------

@pytest.mark.parametrize("size", list(SEQS), ids=["%dx%d" % s for s in SEQS])
def test_frames_on_a_context(pkg, size):
    """P0, P and the flags; RAW, UNGATED and RECT_DEPTH are P; the cloud by bits against the oracle on the colour image
    and P.  Every setting twice: the second frame replays the captured graph, on another scan."""
    F = pkg.frontend
    w, h = size
    seq = SEQS[size]
    bgr = G.frame(w, h, 72)
    gen = _generator(pkg, w, h)
    assert gen.lidar() is None
    for grid in FRAME_GRID:
        s = K.setting(grid, **K.MOUNT)
        gen.set_lidar(K.to_struct(F, s))
        assert gen.lidar() == K.to_struct(F, s)
        for k, n in enumerate((4097, 3000)):
            points = K.scan_clutter(w, h, n, 50 + k, s, _table(F, seq))
            cloud, want = _lidar_frame(gen, F, bgr, points, s, seq, F.FEATURES_HSV if k else F.FEATURES_RGB)
            print(size, grid, "hits", want[3], "occluded", want[4], "points", len(cloud[0]))
            assert len(cloud[0]) >= 20 and want[3] >= 1000 and (want[4] >= 5) == (grid[3] > 0)
    gen.close()


def _alternating(pkg):
    """300, 0, 4097 and 1 points on one context, twice over: every frame by bytes"""
    F = pkg.frontend
    w, h = 96, 64
    seq = SEQS[(w, h)]
    bgr = G.frame(w, h, 72)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    scans = K.frame_scans(w, h, s, _table(F, seq))
    gen = _generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s, max_points=4097))
    sizes = []
    for k in range(2 * len(scans)):
        cloud, want = _lidar_frame(gen, F, bgr, scans[k % len(scans)], s, seq)
        sizes.append((want[3], len(cloud[0])))
    gen.close()
    assert sizes[1] == (0, 0) and sizes[3][0] == 9 and sizes[0][0] > 300 and sizes[:4] == sizes[4:]
    return sizes


def test_counts_alternate_on_one_context(pkg):
    """the count is read on the device, from the header that travels with the points: a captured graph carries it"""
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    _alternating(pkg)


def test_counts_alternate_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_lidar as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_settings_change_between_frames(pkg):
    """other settings, the same settings again, none (a depth frame), and a scan source again, on two alternating
    scans: a graph captured under other settings and launched again would give that frame's planes"""
    F = pkg.frontend
    w, h = 96, 64
    seq = SEQS[(w, h)]
    bgr, dep = G.frame(w, h, 72), KM.surface(w, h, 30)
    gen = _generator(pkg, w, h)
    k = 0
    for grid in FRAME_GRID + (None,) + FRAME_GRID[:2]:
        if grid is None:
            gen.set_lidar(None)
            assert gen.lidar() is None
            for _ in range(2):
                cloud = gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB)
                for stage in (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH):
                    assert gen.read_stage(stage).tobytes() == dep.tobytes()
                _cloud_equal(gen, F, cloud, bgr, dep, seq, F.FEATURES_RGB)
            continue
        s = K.setting(grid, **(K.MOUNT if k % 4 else {}))
        gen.set_lidar(K.to_struct(F, s, max_points=4200 + 100 * (k % 3)))
        for _ in range(2):
            points = K.scan_clutter(w, h, 3500 + 100 * (k % 5), 60 + k % 2, s, _table(F, seq))
            _lidar_frame(gen, F, bgr, points, s, seq, F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB)
            k += 1
    gen.close()


# ---- 3. the stages behind the plane ------------------------------------------------------------------

def test_the_median_fills_behind_the_stage(pkg):
    """splat 0 leaves a sparse plane; the median stage with fill_min reads P and closes gaps"""
    F = pkg.frontend
    w, h = 96, 64
    seq, m = SEQS[(w, h)], (1, 2)
    bgr = G.frame(w, h, 72)
    s = K.setting((0, 7, 1, 0.25), **K.MOUNT)
    points = K.scan_clutter(w, h, 4097, 52, s, _table(F, seq))
    want = K.lidar(points, s, _table(F, seq), w, h)
    B, mflags, changed, filled = KM.median(want[0], m)
    print("coverage", np.mean(want[0] != 0), "->", np.mean(B != 0), "filled", filled)
    assert filled >= 100 and np.mean(want[0] != 0) < 0.6
    gen = _generator(pkg, w, h)
    gen.set_depth_median(KM.to_struct(F, m))
    gen.set_lidar(K.to_struct(F, s))
    assert gen.depth_median() == F.DepthMedian(*m)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _planes_equal(gen, F, want, final=B)
        _differ(gen.read_stage(F.STAGE_UNFILTERED_DEPTH), want[0], "A of the median stage")
        _differ(gen.read_stage(F.STAGE_MEDIAN), mflags, "the median's flags")
        _cloud_equal(gen, F, cloud, bgr, B, seq, F.FEATURES_RGB)
    gen.close()


LIDAR_GATE = G.make_gate(1.1, 5.0, 0.05, 1, 0)


def test_the_gate_and_a_mask_read_the_plane(pkg):
    F = pkg.frontend
    w, h = 96, 64
    seq = SEQS[(w, h)]
    cam = _table(F, seq)
    bgr, mask = G.frame(w, h, 72), G.mask_scene(w, h, 72)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    points = K.scan_clutter(w, h, 4097, 53, s, cam)
    want = K.lidar(points, s, cam, w, h)
    dep, gflags = G.gate(want[0], LIDAR_GATE, cam[0], mask)
    for k in (G.MASKED, G.RANGE, G.JUMP):
        assert np.count_nonzero(gflags & k) >= 5
    gen = _generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s))
    gen.set_depth_gate(G.to_struct(F, LIDAR_GATE))
    gen.set_mask(mask)
    assert gen.lidar() == K.to_struct(F, s)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _planes_equal(gen, F, want, final=dep)
        _differ(gen.read_stage(F.STAGE_UNGATED_DEPTH), want[0], "the plane the gate read")
        _differ(gen.read_stage(F.STAGE_GATE), gflags, "the gate's flags")
        _cloud_equal(gen, F, cloud, bgr, dep, seq, F.FEATURES_RGB)
    gen.close()


def test_selecting_by_depth_holds_the_cloud(pkg):
    """CVO_FE_SELECT_DEPTH on a sparse plane: num_points == num_selected, and every pixel of the map has a depth"""
    F = pkg.frontend
    w, h = 96, 64
    seq = SEQS[(w, h)]
    bgr = G.frame(w, h, 72)
    s = K.setting((0, 7, 1, 0.25), **K.MOUNT)
    points = K.scan_clutter(w, h, 3000, 54, s, _table(F, seq))
    want = K.lidar(points, s, _table(F, seq), w, h)
    gen = _generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s))
    by_image = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
    gen.set_select_mode(F.SELECT_DEPTH)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _planes_equal(gen, F, want)
        info = gen.info()
        picked = gen.read_stage(F.STAGE_MAP) != 0
        print("by the image", len(by_image[0]), "by depth", len(cloud[0]), "selected", info["num_selected"])
        assert info["canny_used"] == 0 and info["num_points"] == info["num_selected"] == len(cloud[0]) > len(by_image[0]) >= 20
        assert picked.any() and (want[0][picked] != 0).all()
    gen.close()


def test_a_frame_under_a_distorting_model(pkg):
    """model C (127 x 193, an odd width): the colour image is rectified, the points go through the model's pinhole, and
    the mask follows the map"""
    F = pkg.frontend
    w, h, model = R.SMALL["C"]
    cam = model[:5]
    bgr, mask = G.frame(w, h, 72), G.mask_scene(w, h, 72)
    qu, qv = R.rectify_map(model, w, h)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    points = K.scan_clutter(w, h, 4097, 55, s, cam)
    want = K.lidar(points, s, cam, w, h)
    dep, gflags = G.gate(want[0], LIDAR_GATE, cam[0], mask, qu, qv)
    plain_gate = G.gate(want[0], LIDAR_GATE, cam[0], mask)
    assert np.count_nonzero(gflags & G.MASKED) >= 5 and not np.array_equal(plain_gate[1], gflags) and want[4] >= 5
    gen = _generator(pkg, w, h)
    gen.set_lidar(K.to_struct(F, s))
    gen.set_camera(F.CameraModel(*model))
    gen.set_depth_gate(G.to_struct(F, LIDAR_GATE))
    gen.set_mask(mask)
    assert gen.lidar() == K.to_struct(F, s)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, want, final=dep)
        _differ(gen.read_stage(F.STAGE_GATE), gflags, "the gate's flags")
        rect = gen.read_stage(F.STAGE_RECT_BGR)
        assert np.array_equal(rect, R.remap_colour(bgr, qu, qv))
        assert len(cloud[0]) >= 20
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(*(cam + (ZERO,))))
    assert _same_cloud(plain.create_pointcloud(rect, dep, 1, F.FEATURES_RGB), cloud)
    plain.close(); gen.close()


# ---- 4. the context ----------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h = 96, 64
    seq = SEQS[(w, h)]
    bgr, dep = G.frame(w, h, 72), KM.surface(w, h, 30)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    good = K.to_struct(F, s, max_points=4097)
    points = K.scan_clutter(w, h, 4097, 56, s, _table(F, seq))
    gen = _generator(pkg, w, h)
    plain = gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB)
    for reason, bad in K.bad_lidars().items():
        with pytest.raises(Err):
            gen.set_lidar(F.Lidar(*bad))                          # on a context without a scan source
        assert gen.lidar() is None, reason
    assert b"set_lidar" in F.lib().cvo_fe_last_error(gen._h)
    for stage in (F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR):
        with pytest.raises(Err):
            gen.read_stage(stage)                                 # no scan source: no such plane
    with pytest.raises(Err):
        gen.submit_lidar(bgr, points, seq)                        # no scan source
    with pytest.raises(Err):
        gen.create_pointcloud_lidar(bgr, points, seq)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB), plain)
    gen.set_lidar(good)
    want, _ = _lidar_frame(gen, F, bgr, points, s, seq)
    for reason, bad in K.bad_lidars().items():
        with pytest.raises(Err):
            gen.set_lidar(F.Lidar(*bad))
        assert gen.lidar() == good, reason
    with pytest.raises(Err):
        gen.submit(bgr, dep, seq)                                 # a frame is an image and a scan now
    with pytest.raises(Err):
        gen.create_pointcloud(bgr, dep, seq)
    L, u8p = F.lib(), C.POINTER(C.c_uint8)
    img = bgr.ctypes.data_as(u8p)
    one_more = np.concatenate([points, points[:1]])
    for pts, stride, n in ((points.ctypes.data, 12, -1), (one_more.ctypes.data, 12, 4098), (points.ctypes.data, 8, 10),
                           (points.ctypes.data, 14, 10), (None, 12, 1)):
        assert L.cvo_fe_submit_lidar(gen._h, img, w * 3, pts, stride, n, seq, F.FEATURES_RGB) == -1
        assert b"submit_lidar" in L.cvo_fe_last_error(gen._h)
    assert L.cvo_fe_submit_lidar(gen._h, img, w * 3, None, 12, 0, seq, F.FEATURES_RGB) == 0       # no points: NULL will do
    empty = gen.collect()
    assert len(empty[0]) == 0 and not gen.read_stage(F.STAGE_RAW_DEPTH).any()
    gen.submit_lidar(bgr, points, seq, F.FEATURES_RGB)
    for other in (K.to_struct(F, K.setting((0, 0, 0, 0.0))), good, None):
        with pytest.raises(Err):
            gen.set_lidar(other)                                  # while a frame is pending, even the settings in force
    assert _same_cloud(gen.collect(), want) and gen.lidar() == good
    gen.set_lidar(good)                                           # the value it has: nothing happens
    assert _same_cloud(_lidar_frame(gen, F, bgr, points, s, seq)[0], want)
    # the points are copied before submit returns: the caller's array may change at once
    mine = points.copy()
    gen.submit_lidar(bgr, mine, seq, F.FEATURES_RGB)
    mine[:] = np.nan
    assert _same_cloud(gen.collect(), want)
    gen.set_lidar(None)
    for stage in (F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR):
        with pytest.raises(Err):
            gen.read_stage(stage)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB), plain)
    gen.close()


def test_a_scan_source_excludes_stereo_and_a_depth_camera(pkg):
    """in both directions, the context keeping what it had"""
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h = 96, 64
    lidar = K.to_struct(F, K.setting((1, 7, 1, 0.25), **K.MOUNT))
    stereo = F.Stereo(0.54, 32)
    rig = F.DepthCamera(80, 60, 5000.0, 60.0, 60.0, 40.0, 30.0)
    gen = _generator(pkg, w, h)
    gen.set_lidar(lidar)
    for call in (lambda: gen.set_stereo(stereo), lambda: gen.set_depth_camera(rig)):
        with pytest.raises(Err):
            call()
    assert gen.lidar() == lidar and gen.stereo() is None and gen.depth_camera() is None
    gen.set_stereo(None); gen.set_depth_camera(None)              # clearing what is not set is no error
    gen.set_lidar(None)
    gen.set_stereo(stereo)
    with pytest.raises(Err):
        gen.set_lidar(lidar)
    assert gen.lidar() is None and gen.stereo() == stereo
    gen.set_lidar(None)
    gen.set_stereo(None)
    gen.set_depth_camera(rig)
    with pytest.raises(Err):
        gen.set_lidar(lidar)
    assert gen.lidar() is None and gen.depth_camera() == rig
    gen.set_depth_camera(None)
    gen.set_lidar(lidar)
    assert gen.lidar() == lidar
    gen.close()


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set a scan source, ran a frame under it and cleared it: in bytes and in the cloud"""
    F = pkg.frontend
    w, h = 96, 64
    seq = SEQS[(w, h)]
    bgr, dep = G.frame(w, h, 72), KM.surface(w, h, 30)
    s = K.setting((1, 7, 1, 0.25), **K.MOUNT)
    never, cleared = _generator(pkg, w, h), _generator(pkg, w, h)
    stages = (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_GATE, F.STAGE_MAP, F.STAGE_AG0)
    clouds, planes = [], []
    for gen in (never, cleared):
        if gen is cleared:
            gen.set_lidar(K.to_struct(F, s))
            _lidar_frame(gen, F, bgr, K.scan_clutter(w, h, 4097, 57, s, _table(F, seq)), s, seq)
            gen.set_lidar(None)
        assert gen.lidar() is None
        gen.set_lidar(None)                                        # clearing what is not set is no error
        clouds.append(gen.create_pointcloud(bgr, dep, seq, F.FEATURES_RGB))
        planes.append([gen.read_stage(st).tobytes() for st in stages])
        assert planes[-1][2] == dep.tobytes()
    assert _same_cloud(clouds[0], clouds[1]) and planes[0] == planes[1]
    never.close(); cleared.close()


def test_the_source_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 4096 x 2048 the z-buffer is 32 MiB, P0 and the flags 24 MiB, and a scan of 2^21 points 24 MiB,
    against the 8 MiB a reading of the free device memory resolves.  Refused settings leave it where it was; the first
    settings are seen by the same reading, and clearing the source gives all of it back."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(4096, 2048)
    free0 = free()
    for bad in K.bad_lidars().values():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_lidar(F.Lidar(*bad))
    gen.set_lidar(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_lidar(F.Lidar(K.MAX_POINTS, 1))
    free2 = free()
    assert free1 - free2 >= 48 * MiB, "the first settings took only %d bytes" % (free1 - free2)
    gen.set_lidar(F.Lidar(K.MAX_POINTS, 1, occl_rel=0.25, occl_rx=7))
    free3 = free()
    assert free2 - free3 >= 16 * MiB, "the occlusion test's planes took only %d bytes" % (free2 - free3)
    gen.set_lidar(F.Lidar(K.MAX_POINTS, 2, occl_rel=0.5, occl_rx=3))
    free4 = free()
    assert abs(free3 - free4) < 8 * MiB, "other settings moved the free memory by %d bytes" % (free3 - free4)
    gen.set_lidar(None)
    free5 = free()
    assert free5 - free4 >= 72 * MiB, "clearing the source gave back only %d bytes" % (free5 - free4)
    gen.close()


# ---- 5. the layers above -----------------------------------------------------------------------------

RUN_GRID = (1, 7, 1, 0.25)


def _scan_of(dep, cam, s, step=2):
    """the scan a scanner at the mount of `s` would give of a depth image: every `step`-th pixel lifted; n x 4 float32
    (the fourth is not read), a multiple of 16 records"""
    h, w = dep.shape
    v, u = np.mgrid[0:h:step, 0:w:step]
    z = dep[::step, ::step].astype(np.float64) / cam[0]
    keep = z > 0
    pts = K.back(u[keep].astype(np.float64), v[keep].astype(np.float64), z[keep], cam, s)
    pts = pts[:len(pts) // 16 * 16]
    return K.with_stride(pts, 4, fill=0.5)


def _lidar_frames(pkg):
    F = pkg.frontend
    s = K.setting(RUN_GRID, **K.MOUNT)
    return s, [(name, bgr, _scan_of(dep, _table(F, 1), s)) for name, bgr, dep in _four_frames(pkg, 75)]


def test_run_frames_takes_the_setting(pkg):
    """run_frames(lidar=) on (name, bgr, points) = the generator driven by hand = run_frames without it on the planes
    the restatement makes of the scans: the same poses"""
    F = pkg.frontend
    s, frames = _lidar_frames(pkg)
    lidar = K.to_struct(F, s, max_points=80000)
    planes = [(name, bgr, K.lidar(pts, s, _table(F, 1), 640, 480)[0]) for name, bgr, pts in frames]
    assert all(np.mean(p[2] != 0) > 0.5 for p in planes)
    poses = []
    for fr, l in ((frames, lidar), (planes, None)):
        reg, buf = pkg.Cvo(), io.StringIO()
        gen = F.PcdGenerator(640, 480)
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen, lidar=l) == 4
        assert gen.lidar() == l
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == planes[3][2].tobytes()
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close(); gen.close()
    reg, buf = pkg.Cvo(), io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(640, 480)
    gen.set_lidar(lidar)
    gen.set_device_output(True)
    for k, (name, bgr, pts) in enumerate(frames):
        gen.submit_lidar(bgr, pts, 1, F.FEATURES_RGB)
        dp, df, n = gen.collect_device()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == planes[k][2].tobytes()
        reg.run_cvo_device(dp, df, n)
        writer.append(name, reg.accum_transform)
    poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
    reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


class _ScanFrames:
    """a generator whose submit() takes the scan a demo frame carries in its depth image's place"""

    def __init__(self, gen):
        self._gen = gen

    def __getattr__(self, name):
        return getattr(self._gen, name)

    def submit(self, bgr, dep, seq, ftype):
        self._gen.submit_lidar(bgr, dep.view(np.float32).reshape(-1, 4), seq, ftype)


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_setting(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_lidar / clear_lidar / run_cvo_lidar (tests/cpp/cvo_lidar_demo.cpp): the clouds
    the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    s, frames = _lidar_frames(pkg)
    lidar = K.to_struct(F, s, max_points=80000)
    # a frame's scan travels as a "depth image" of 128 x (n / 16) uint16
    carried = [(name, bgr, pts.view(np.uint16).reshape(-1, 128)) for name, bgr, pts in frames]
    got = _demo_lines(tmp_path, "cvo_lidar_demo", carried, w, h, bytes(lidar), [mode_name], depth_sizes=True)
    gen = F.PcdGenerator(w, h)
    gen.set_lidar(lidar)
    others = ["refused bad settings", "refused stereo", "refused depth camera"]

    def prepare(k):
        return others + ["refused depth image", "refused scan"] if k == 2 else []

    want, sizes, _ = _device_path_lines(pkg, mode_name, _ScanFrames(gen), carried, prepare)
    assert got == others + want
    ftype = F.FEATURES_HSV if mode_name == "acvo" else F.FEATURES_RGB
    P = K.lidar(frames[0][2], s, _table(F, 1), w, h)[0]
    assert sizes[0] == len(fo.create_pointcloud(frames[0][1], P, 1, ftype)["positions"]) > 100
    gen.close()
