"""GPU: the infill stage of the front end (cvo_fe_set_depth_infill, cvo_fe_infill_plane; the infill contract of
include/cvo_frontend.h): k_fe_infill of csrc/cvo_infill.hip against the restatement tests/fe_infill_ref.py by bytes --
F, the flags and both counts on every plane made on purpose at every setting, and the planes of depth frames, frames
under a scan source, the stereo matcher, a depth camera and a distorting model in front of the stage, the median stage,
the gate and a mask behind it -- and the cloud by bits against the CPU restatement of the front end
(oracle/frontend_oracle.c) on the colour image and the plane the cloud is made from.  Settings alternating with "off" on
one context, with and without captured graphs (a stale graph would show), a context that never made the call, the
refusals, the memory, run_frames and the C++ objects above.  What the planes reach, and which errors of a tiled
two-pass interpolation they would show, is asserted in tests/test_fe_infill_cpu.py."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_depth_ref as D
import fe_gate_ref as G
import fe_infill_ref as K
import fe_lidar_ref as KL
import fe_median_ref as KM
import fe_rectify_ref as R
import fe_speckle_ref as KS
import fe_stereo_paths_ref as P
import fe_stereo_ref as S
from fe_gpu_common import ROOT, _demo_lines, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
SIZES = ((64, 64), (96, 64))
_REF = {}


def _ref(key, make):
    """A reference result, computed once per key and left unchanged."""
    if key not in _REF:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _planes_equal(gen, F, Sp, Fp, flags, gate_read=None, final=None):
    """the stage's two planes; the plane the gate read (F, or the median's B); the plane every later stage read"""
    read = Fp if gate_read is None else gate_read
    for stage, want, what in ((F.STAGE_SPARSE_DEPTH, Sp, "S"), (F.STAGE_INFILL, flags, "the flags"),
                              (F.STAGE_UNGATED_DEPTH, read, "the plane the gate read"),
                              (F.STAGE_RECT_DEPTH, read if final is None else final, "the plane every later stage read")):
        _differ(gen.read_stage(stage), want, what)


def _cloud_equal(gen, F, cloud, bgr, depth, seq, ftype):
    """the cloud against the front-end oracle on the colour image and the plane the cloud is made from, by bits"""
    ref = fo.create_pointcloud(bgr, depth, seq, ftype, num_want=gen.num_want)
    info = gen.info()
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(cloud[0])
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud(cloud, (ref["positions"], ref["features"]))


def _depth_frame(gen, F, bgr, Sp, f, ftype=None):
    ftype = F.FEATURES_RGB if ftype is None else ftype
    Fp, flags, nr, nc = K.infill(Sp, f)
    cloud = gen.create_pointcloud(bgr, Sp, 1, ftype)
    _planes_equal(gen, F, Sp, Fp, flags)
    _differ(gen.read_stage(F.STAGE_RAW_DEPTH), Sp, "the depth image as uploaded")
    _cloud_equal(gen, F, cloud, bgr, Fp, 1, ftype)
    return cloud


def _plain_frame(gen, F, bgr, Sp, ftype=None):
    """a frame of a context without the stage: today's planes"""
    ftype = F.FEATURES_RGB if ftype is None else ftype
    cloud = gen.create_pointcloud(bgr, Sp, 1, ftype)
    for stage in (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH):
        _differ(gen.read_stage(stage), Sp, "a plane of a frame without the stage")
    _cloud_equal(gen, F, cloud, bgr, Sp, 1, ftype)
    return cloud


# ---- 1. the stand-alone entry on planes made on purpose ----------------------------------------------

def _stand_alone(F, Sp, f, what, **kw):
    want = K.infill(Sp, f)
    arg = Sp.copy()
    got = F.infill_plane(arg, K.to_struct(F, f), **kw)
    assert np.array_equal(arg, Sp)
    print(what, f, "rows", got[2], want[2], "columns", got[3], want[3])
    _differ(got[0], want[0], "F of %s at %s" % (what, f))
    _differ(got[1], want[1], "the flags of %s at %s" % (what, f))
    assert got[2:] == tuple(want[2:]), (what, f, got[2:], want[2:])
    return want


@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_infill_plane_on_a_made_plane(pkg, name):
    """every made plane at every setting: F, the flags and both counts by bytes; the argument is left as it is"""
    F = pkg.frontend
    for f in K.SETTINGS:
        Sp, Fp, flags, nr, nc = K.made(name, f)
        got = F.infill_plane(Sp, K.to_struct(F, f))
        print(name, f, "rows", got[2], nr, "columns", got[3], nc)
        _differ(got[0], Fp, "F of %s at %s" % (name, f))
        _differ(got[1], flags, "the flags of %s at %s" % (name, f))
        assert got[2:] == (nr, nc), (name, f)


@pytest.mark.parametrize("size", [(1, 1), (8192, 3), (3, 8192)], ids=["1x1", "8192x3", "3x8192"])
def test_infill_plane_at_the_size_limits(pkg, size):
    """one pixel, the largest width and the largest height: 128 tiles side by side, 512 on top of each other"""
    F = pkg.frontend
    Sp = K.long_plane(*size)
    for f in ((15, 31, 0.25), (2, 5, 0.0)):
        want = _stand_alone(F, Sp, f, size)
        assert size == (1, 1) or want[2] + want[3] >= 1000


def test_infill_plane_takes_a_row_stride(pkg):
    """rows further apart than their pixels: what lies between them stays"""
    F = pkg.frontend
    for name, f in (("sparse-127x193", (2, 5, 0.25)), ("ground-96x64", (15, 31, 0.0))):
        _stand_alone(F, K.plane(name), f, name, stride=K.plane(name).shape[1] + 5)


# ---- 2. frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_a_depth_frame(pkg, size):
    """every plane of a depth frame by bytes and the cloud by bits against the oracle on the colour image and F; every
    setting twice: the second frame replays the captured graph"""
    F = pkg.frontend
    w, h = size
    bgr = G.frame(w, h, 72)
    planes = [K.sparse(w, h, 11), K.spoil(KM.surface(w, h, 30), 1)]
    gen = _generator(pkg, w, h)
    assert gen.depth_infill() is None
    for f in K.FRAME_SETTINGS:
        gen.set_depth_infill(K.to_struct(F, f))
        assert gen.depth_infill() == F.DepthInfill(*f)
        for k in range(2):
            cloud = _depth_frame(gen, F, bgr, planes[k], f, F.FEATURES_HSV if k else F.FEATURES_RGB)
            assert len(cloud[0]) >= 20
    gen.close()


INFILL_GATE = G.make_gate(1.3, 2.3, 0.05, 1, 0)


def test_the_median_and_the_gate_read_the_filled_plane(pkg):
    """F is the median's A (UNFILTERED_DEPTH), its B the gate's U; range, jump marks and mask act on B"""
    F = pkg.frontend
    w, h = 96, 64
    f, m = (2, 5, 0.25), (1, 5)
    Sp, bgr, mask = K.spoil(KM.stepped(w, h, 31), 2), G.frame(w, h, 72), G.mask_scene(w, h, 72)
    Fp, flags, nr, nc = K.infill(Sp, f)
    B = KM.median(Fp, m)
    dep, gflags = G.gate(B[0], INFILL_GATE, G.SCALE, mask)
    assert nr >= 100 and nc >= 100 and B[2] + B[3] >= 5 and np.count_nonzero(gflags) >= 20 and np.count_nonzero(dep) >= 100
    gen = _generator(pkg, w, h)
    gen.set_depth_infill(K.to_struct(F, f))
    gen.set_depth_median(KM.to_struct(F, m))
    assert gen.depth_infill() == F.DepthInfill(*f)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, Sp, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, Sp, Fp, flags, gate_read=B[0])
        _differ(gen.read_stage(F.STAGE_UNFILTERED_DEPTH), Fp, "A of the median contract")
        _differ(gen.read_stage(F.STAGE_MEDIAN), B[1], "the median's flags")
        _cloud_equal(gen, F, cloud, bgr, B[0], 1, F.FEATURES_RGB)
    gen.set_depth_gate(G.to_struct(F, INFILL_GATE))
    gen.set_mask(mask)
    assert gen.depth_infill() == F.DepthInfill(*f)            # (the other setters: the setting stays)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, Sp, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, Sp, Fp, flags, gate_read=B[0], final=dep)
        _differ(gen.read_stage(F.STAGE_GATE), gflags, "the gate's flags")
        _cloud_equal(gen, F, cloud, bgr, dep, 1, F.FEATURES_RGB)
    gen.set_depth_median(None)                                # the gate alone behind the stage: U is F
    dep, gflags = G.gate(Fp, INFILL_GATE, G.SCALE, mask)
    cloud = gen.create_pointcloud(bgr, Sp, 1, F.FEATURES_RGB)
    _planes_equal(gen, F, Sp, Fp, flags, final=dep)
    _differ(gen.read_stage(F.STAGE_GATE), gflags, "the gate's flags")
    _cloud_equal(gen, F, cloud, bgr, dep, 1, F.FEATURES_RGB)
    gen.close()


def test_selecting_by_depth_reads_the_filled_plane(pkg):
    """CVO_FE_SELECT_DEPTH: num_points == num_selected, every pixel of the map has a depth in F, and more pixels
    compete than on S"""
    F = pkg.frontend
    w, h = 96, 64
    f = (2, 5, 0.25)
    Sp, bgr = K.spoil(KM.surface(w, h, 30), 1), G.frame(w, h, 72)
    Fp = K.infill(Sp, f)[0]
    gen = _generator(pkg, w, h)
    gen.set_select_mode(F.SELECT_DEPTH)
    sparse_cloud = gen.create_pointcloud(bgr, Sp, 1, F.FEATURES_RGB)
    gen.set_depth_infill(K.to_struct(F, f))
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, Sp, 1, F.FEATURES_RGB)
        info, picked = gen.info(), gen.read_stage(F.STAGE_MAP) != 0
        assert info["canny_used"] == 0 and info["num_points"] == info["num_selected"] == len(cloud[0]) >= 20
        assert picked.any() and (Fp[picked] != 0).all() and not (Sp[picked] != 0).all()
    print("points under SELECT_DEPTH: on S", len(sparse_cloud[0]), "on F", len(cloud[0]))
    assert len(cloud[0]) >= len(sparse_cloud[0])
    gen.close()


def test_a_lidar_frame_at_splat_0_with_the_cull(pkg):
    """the projection and its cull write S; P0 and the scan's flags stay what they are without the stage"""
    F = pkg.frontend
    w, h, seq = 96, 64, 4
    f = (2, 5, 0.25)
    cam = tuple(F.camera(seq).values())
    bgr = G.frame(w, h, 72)
    s = KL.setting((0, 7, 1, 0.25), **KL.MOUNT)
    points = KL.scan_clutter(w, h, 4097, 52, s, cam)
    want = KL.lidar(points, s, cam, w, h)
    Fp, flags, nr, nc = K.infill(want[0], f)
    print("coverage", np.mean(want[0] != 0), "->", np.mean(Fp != 0), "rows", nr, "columns", nc, "occluded", want[4])
    assert nr >= 100 and nc >= 100 and want[4] >= 5
    gen = _generator(pkg, w, h)
    gen.set_depth_infill(K.to_struct(F, f))
    gen.set_lidar(KL.to_struct(F, s))
    assert gen.depth_infill() == F.DepthInfill(*f)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _planes_equal(gen, F, want[0], Fp, flags)
        _differ(gen.read_stage(F.STAGE_LIDAR_DEPTH), want[1], "P0")
        _differ(gen.read_stage(F.STAGE_LIDAR), want[2], "the scan's flags")
        _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want[0], "P")
        _cloud_equal(gen, F, cloud, bgr, Fp, seq, F.FEATURES_RGB)
    gen.set_lidar(KL.to_struct(F, KL.setting((0, 0, 0, 0.0), **KL.MOUNT)))     # no cull: P0 is P, and the flags are made from it
    want = KL.lidar(points, KL.setting((0, 0, 0, 0.0), **KL.MOUNT), cam, w, h)
    Fp, flags, nr, nc = K.infill(want[0], f)
    gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
    _planes_equal(gen, F, want[0], Fp, flags)
    _differ(gen.read_stage(F.STAGE_LIDAR_DEPTH), want[1], "P0 without the cull")
    _differ(gen.read_stage(F.STAGE_LIDAR), want[2], "the scan's flags without the cull")
    gen.close()


def test_a_stereo_frame(pkg):
    """DISPARITY and STEREO stay the matcher's, byte-equal to the frame without the stage; the stage reads the depth
    plane behind the speckle filter and a filled pixel has a depth and DISPARITY 0"""
    F = pkg.frontend
    name, sp, f = "default-96x64-82", (12, 16), (2, 5, 0.25)
    w, h, st, left, right = P.inputs(name)
    Q = KS.case_frame(name, sp)
    Sp = Q["depth"]
    Fp, flags, nr, nc = K.infill(Sp, f)
    print("stereo: rows", nr, "columns", nc)
    filled = (flags == K.ROW) | (flags == K.COL)
    assert nr + nc >= 20 and (Q["disparity"][filled] == 0).all()
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_speckle(KS.to_struct(F, sp))
    gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    stages = (F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_SGM_SUM, F.STAGE_SPECKLE_SIZE)
    before = [gen.read_stage(s).tobytes() for s in stages]
    _differ(gen.read_stage(F.STAGE_RECT_DEPTH), Sp, "the matcher's depth")
    gen.set_depth_infill(K.to_struct(F, f))
    assert gen.stereo_speckle() == F.Speckle(*sp) and gen.stereo() == S.to_struct(F, st)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        assert [gen.read_stage(s).tobytes() for s in stages] == before
        _planes_equal(gen, F, Sp, Fp, flags)
        _differ(gen.read_stage(F.STAGE_RAW_DEPTH), Sp, "the plane stereo wrote")
        _cloud_equal(gen, F, cloud, left, Fp, S.SEQ, F.FEATURES_RGB)
    gen.set_stereo(None)                                      # (the setting survives, and depth frames read it)
    assert gen.depth_infill() == F.DepthInfill(*f)
    _depth_frame(gen, F, left, K.sparse(w, h, 12), f)
    gen.close()


def test_a_frame_under_a_depth_camera(pkg):
    """rig K: k_fe_depth_final writes S, and the holes the forward warp leaves are bridged"""
    F = pkg.frontend
    w, h, cam, rig = D.RIGS["K"]
    f = (2, 2, 0.05)
    bgr = G.frame(w, h, 72)
    raw = D.scene(pkg.data, rig)
    Sp, = _ref("rig K", lambda: (D.register(rig, cam, w, h, raw),))
    Fp, flags, nr, nc = K.infill(Sp, f)
    print("under the depth camera: holes", np.count_nonzero(Sp == 0), "rows", nr, "columns", nc)
    assert nr + nc >= 20
    gen = _generator(pkg, w, h)
    gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
    gen.set_depth_infill(K.to_struct(F, f))
    gen.set_depth_camera(D.to_struct(F, rig))
    assert gen.depth_infill() == F.DepthInfill(*f)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, Sp, Fp, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), raw)
        assert len(cloud[0]) >= 20
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(*(cam + (ZERO,))))
    assert _same_cloud(plain.create_pointcloud(bgr, Fp, 1, F.FEATURES_RGB), cloud)
    plain.close(); gen.close()


def test_a_frame_under_a_distorting_model(pkg):
    """model C (an odd width): k_fe_rectify writes S"""
    F = pkg.frontend
    w, h, model = R.SMALL["C"]
    f = (2, 5, 0.25)
    U0, bgr = K.spoil(KM.surface(w, h, 32), 1), G.frame(w, h, 72)
    qu, qv = R.rectify_map(model, w, h)
    Sp = R.remap_depth(U0, qu, qv)
    Fp, flags, nr, nc = K.infill(Sp, f)
    assert nr + nc >= 100
    gen = _generator(pkg, w, h)
    gen.set_depth_infill(K.to_struct(F, f))
    gen.set_camera(F.CameraModel(*model))
    assert gen.depth_infill() == F.DepthInfill(*f)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, U0, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, Sp, Fp, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), U0)
        rect = gen.read_stage(F.STAGE_RECT_BGR)
        assert len(cloud[0]) >= 20
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(*(model[:5] + (ZERO,))))
    assert _same_cloud(plain.create_pointcloud(rect, Fp, 1, F.FEATURES_RGB), cloud)
    plain.close(); gen.close()


# ---- 3. the context ----------------------------------------------------------------------------------

ALTERNATING = ((2, 5, 0.25), None, (15, 31, 0.0), None, (1, 0, 0.0), (0, 0, 0.0))


def _alternating(pkg):
    """settings alternating with "off" on two alternating planes: every frame by bytes.  A graph captured under other
    settings, or without the stage, and launched again would give that frame's planes."""
    F = pkg.frontend
    w, h = 96, 64
    bgr = G.frame(w, h, 72)
    planes = [K.sparse(w, h, 11), K.sparse(w, h, 13)]
    gen = _generator(pkg, w, h)
    k, sizes = 0, []
    for f in ALTERNATING + ALTERNATING[:2]:
        gen.set_depth_infill(K.to_struct(F, f))
        assert gen.depth_infill() == K.to_struct(F, f)
        for _ in range(2):
            ftype = F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB
            cloud = _plain_frame(gen, F, bgr, planes[k % 2], ftype) if f is None else _depth_frame(gen, F, bgr, planes[k % 2], f, ftype)
            sizes.append(len(cloud[0]))
            k += 1
    gen.close()
    return sizes


def test_settings_alternate_with_off_on_one_context(pkg):
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    assert len(_alternating(pkg)) == 16


def test_settings_alternate_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_infill as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set the stage, ran a frame under it and cleared it: in bytes and in the cloud"""
    F = pkg.frontend
    w, h = 96, 64
    Sp, bgr = K.sparse(w, h, 11), G.frame(w, h, 72)
    never, cleared = _generator(pkg, w, h), _generator(pkg, w, h)
    stages = (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_GATE, F.STAGE_MAP, F.STAGE_AG0)
    clouds, planes = [], []
    for gen in (never, cleared):
        if gen is cleared:
            gen.set_depth_infill(F.DepthInfill(2, 5, 0.25))
            filled = _depth_frame(gen, F, bgr, Sp, (2, 5, 0.25))
            gen.set_depth_infill(None)
        assert gen.depth_infill() is None
        gen.set_depth_infill(None)                             # clearing what is not set is no error
        clouds.append(_plain_frame(gen, F, bgr, Sp))
        planes.append([gen.read_stage(s).tobytes() for s in stages])
    assert _same_cloud(clouds[0], clouds[1]) and planes[0] == planes[1] and not _same_cloud(filled, clouds[0])
    never.close(); cleared.close()


def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h = 96, 64
    f = (2, 5, 0.25)
    Sp, bgr = K.sparse(w, h, 11), G.frame(w, h, 72)
    assert F.check_depth_infill(F.DepthInfill(0, 0, 0.0)) and F.check_depth_infill(F.DepthInfill(15, 31, 7.5))
    assert not F.check_depth_infill(None) and not any(F.check_depth_infill(F.DepthInfill(*bad)) for bad in K.bad_infills())
    gen = _generator(pkg, w, h)
    plain = _plain_frame(gen, F, bgr, Sp)
    for bad in K.bad_infills():
        with pytest.raises(Err):
            gen.set_depth_infill(F.DepthInfill(*bad))         # on a context without the stage
        assert gen.depth_infill() is None
    assert b"set_depth_infill" in F.lib().cvo_fe_last_error(gen._h)
    for stage in (F.STAGE_SPARSE_DEPTH, F.STAGE_INFILL):
        with pytest.raises(Err):
            gen.read_stage(stage)                             # no stage: no such plane
    assert _same_cloud(_plain_frame(gen, F, bgr, Sp), plain)
    for bad in (F.DepthInfill(16, 0, 0.0), None):
        with pytest.raises(Err):
            F.infill_plane(np.ones((4, 4), np.uint16), bad)
    with pytest.raises(Err):
        F.infill_plane(np.ones((1, 8193), np.uint16), F.DepthInfill(*f))
    gen.set_depth_infill(F.DepthInfill(*f))
    want = _depth_frame(gen, F, bgr, Sp, f)
    for bad in K.bad_infills():
        with pytest.raises(Err):
            gen.set_depth_infill(F.DepthInfill(*bad))
        assert gen.depth_infill() == F.DepthInfill(*f)
    gen.submit(bgr, Sp, 1, F.FEATURES_RGB)
    for other in (F.DepthInfill(15, 31, 0.0), F.DepthInfill(*f), None):
        with pytest.raises(Err):
            gen.set_depth_infill(other)                       # while a frame is pending, even the settings in force
    assert _same_cloud(gen.collect(), want) and gen.depth_infill() == F.DepthInfill(*f)
    gen.set_depth_infill(F.DepthInfill(*f))                   # the value it has: nothing happens
    assert _same_cloud(_depth_frame(gen, F, bgr, Sp, f), want)
    gen.set_depth_infill(None)
    for stage in (F.STAGE_SPARSE_DEPTH, F.STAGE_INFILL):
        with pytest.raises(Err):
            gen.read_stage(stage)
    assert _same_cloud(_plain_frame(gen, F, bgr, Sp), plain)
    gen.close()


def test_the_stage_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 4096 x 2048 the two planes of the stage are 24 MiB, three times the 8 MiB a reading of the free
    device memory resolves.  Refused settings leave it where it was; the first settings are seen by the same reading,
    other settings take nothing more, and clearing the stage gives all of it back."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(4096, 2048)
    free0 = free()
    for bad in K.bad_infills():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_infill(F.DepthInfill(*bad))
    gen.set_depth_infill(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_depth_infill(F.DepthInfill(2, 5, 0.25))
    free2 = free()
    assert free1 - free2 >= 16 * MiB, "the first settings took only %d bytes" % (free1 - free2)
    gen.set_depth_infill(F.DepthInfill(15, 31, 0.0))
    free3 = free()
    assert abs(free2 - free3) < 8 * MiB, "other settings moved the free memory by %d bytes" % (free2 - free3)
    gen.set_depth_infill(None)
    free4 = free()
    assert free4 - free3 >= 16 * MiB, "clearing the stage gave back only %d bytes" % (free4 - free3)
    gen.close()


# ---- 4. the layers above -----------------------------------------------------------------------------

RUN_INFILL = (2, 5, 0.25)


def _frames(pkg):
    return _four_frames(pkg, 75, lambda k, dep: K.spoil(dep, 40 + k))


def test_run_frames_takes_the_setting(pkg):
    """run_frames(depth_infill=) on the thinned frames = the generator driven by hand = run_frames without it on frames
    filled beforehand by the restatement: the same poses"""
    F = pkg.frontend
    frames = _frames(pkg)
    filled = [(name, bgr, _ref(("seq", k), lambda: K.infill(dep, RUN_INFILL))[0]) for k, (name, bgr, dep) in enumerate(frames)]
    assert all(not np.array_equal(a[2], b[2]) for a, b in zip(frames, filled))
    poses = []
    for fr, f in ((frames, F.DepthInfill(*RUN_INFILL)), (filled, None)):
        reg, buf = pkg.Cvo(), io.StringIO()
        gen = F.PcdGenerator(640, 480)
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen, depth_infill=f) == 4
        assert gen.depth_infill() == f
        _differ(gen.read_stage(F.STAGE_RECT_DEPTH), filled[3][2], "the last frame's depth")
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close(); gen.close()
    reg, buf = pkg.Cvo(), io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(640, 480)
    gen.set_depth_infill(F.DepthInfill(*RUN_INFILL))
    gen.set_device_output(True)
    for k, (name, bgr, dep) in enumerate(frames):
        gen.submit(bgr, dep, 1, F.FEATURES_RGB)
        dp, df, n = gen.collect_device()
        _differ(gen.read_stage(F.STAGE_RECT_DEPTH), filled[k][2], "frame %d's depth" % k)
        reg.run_cvo_device(dp, df, n)
        writer.append(name, reg.accum_transform)
    poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
    reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_setting(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_depth_infill / clear_depth_infill (tests/cpp/cvo_depth_infill_demo.cpp): the
    clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    frames = _frames(pkg)
    infill = F.DepthInfill(*RUN_INFILL)
    got = _demo_lines(tmp_path, "cvo_depth_infill_demo", frames, w, h, bytes(infill), [mode_name])
    gen = F.PcdGenerator(w, h)

    def prepare(k):
        gen.set_depth_infill(None if k == 2 else infill)
        return ["refused bad settings"] if k == 3 else []

    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, frames, prepare)
    assert got == ["refused bad settings"] + want
    ftype = F.FEATURES_HSV if mode_name == "acvo" else F.FEATURES_RGB
    # the filled frames' clouds are the oracle's on the restatement's plane, and larger than the thinned frame's
    Fp = _ref(("seq", 0), lambda: K.infill(frames[0][2], RUN_INFILL))[0]
    assert sizes[0] == len(fo.create_pointcloud(frames[0][1], Fp, 1, ftype)["positions"]) > 100
    assert sizes[2] == len(fo.create_pointcloud(frames[2][1], frames[2][2], 1, ftype)["positions"]) < min(sizes[0], sizes[1], sizes[3])
    gen.close()
