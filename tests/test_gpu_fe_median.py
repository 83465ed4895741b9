"""GPU: the median stage of the front end (cvo_fe_set_depth_median, cvo_fe_median_plane; the median contract of
include/cvo_frontend.h): k_fe_median of csrc/cvo_median.hip against the restatement tests/fe_median_ref.py by bytes --
the plane, the flags and both counts on every plane made on purpose at every setting, and the planes of depth frames,
frames under a depth camera, a distorting model, the stereo matcher and a stereo rig behind the stage -- and the cloud by
bits against the CPU restatement of the front end (oracle/frontend_oracle.c) on the colour image and the filtered plane.
Settings alternating on one context (a stale captured graph would show), a context that never made the call, the
refusals, the memory, run_frames and the C++ objects above.  What the planes reach, and which errors of a tiled median
they would show, is asserted in tests/test_fe_median_cpu.py."""
import ctypes as C
import io

import numpy as np
import pytest

import fe_depth_ref as D
import fe_gate_ref as G
import fe_median_ref as K
import fe_rectify_ref as R
import fe_speckle_ref as KS
import fe_stereo_paths_ref as P
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
from fe_gpu_common import _demo_lines, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
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


def _planes_equal(gen, F, A, B, flags, final=None):
    """the stage's two planes, and the plane the gate read; without a gate (final None) that is RECT_DEPTH too"""
    for stage, want, what in ((F.STAGE_UNFILTERED_DEPTH, A, "A"), (F.STAGE_MEDIAN, flags, "the flags"),
                              (F.STAGE_UNGATED_DEPTH, B, "B, the plane the gate read"),
                              (F.STAGE_RECT_DEPTH, B if final is None else final, "the plane every later stage read")):
        got = gen.read_stage(stage)
        assert got.dtype == want.dtype and got.shape == want.shape, what
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                                 % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _cloud_equal(gen, F, cloud, bgr, depth, seq, ftype):
    """the cloud against the front-end oracle on the colour image and the plane the cloud is made from, by bits"""
    ref = fo.create_pointcloud(bgr, depth, seq, ftype, num_want=gen.num_want)
    info = gen.info()
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(cloud[0])
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud(cloud, (ref["positions"], ref["features"]))


def _depth_frame(gen, F, bgr, A, m, ftype=None):
    ftype = F.FEATURES_RGB if ftype is None else ftype
    B, flags, changed, filled = K.median(A, m)
    cloud = gen.create_pointcloud(bgr, A, 1, ftype)
    _planes_equal(gen, F, A, B, flags)
    assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == A.tobytes()
    _cloud_equal(gen, F, cloud, bgr, B, 1, ftype)
    return cloud


# ---- 1. the stand-alone entry on planes made on purpose ----------------------------------------------

@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_median_plane_on_a_made_plane(pkg, name):
    """every made plane at every setting: the plane, the flags and both counts by bytes; the argument is left as it is"""
    F = pkg.frontend
    for m in K.SETTINGS:
        A, B, flags, changed, filled = K.made(name, m)
        arg = A.copy()
        got = F.median_plane(arg, K.to_struct(F, m))
        assert np.array_equal(arg, A)
        assert got[0].dtype == np.uint16 and got[1].dtype == np.uint8 and got[0].shape == got[1].shape == A.shape
        print(name, m, "changed", got[2], changed, "filled", got[3], filled)
        assert got[0].tobytes() == B.tobytes(), (name, m)
        assert got[1].tobytes() == flags.tobytes(), (name, m)
        assert got[2:] == (changed, filled), (name, m)


def test_median_plane_takes_a_row_stride_and_no_flags(pkg):
    """rows further apart than their pixels: what lies between them stays; `flags` may be NULL"""
    F = pkg.frontend
    for name, m in (("surface", (1, 5)), ("noise-holes", (2, 13))):
        A, B, flags, changed, filled = K.made(name, m)
        h, w = A.shape
        wide = np.full((h, w + 5), 777, np.uint16)
        wide[:, :w] = A
        nc, nf = C.c_int(-1), C.c_int(-1)
        rc = F.lib().cvo_fe_median_plane(0, wide.ctypes.data_as(C.POINTER(C.c_uint16)), (w + 5) * 2, w, h,
                                         C.byref(K.to_struct(F, m)), None, C.byref(nc), C.byref(nf))
        assert rc == 0 and (nc.value, nf.value) == (changed, filled)
        assert np.array_equal(wide[:, :w], B) and (wide[:, w:] == 777).all()


@pytest.mark.parametrize("size", [(8192, 3), (3, 8192)], ids=["8192x3", "3x8192"])
def test_median_plane_at_the_size_limits(pkg, size):
    """the largest width and the largest height: 128 tiles side by side, 512 on top of each other"""
    F = pkg.frontend
    A = K.long_plane(*size)
    for m in K.LONG_SETTINGS:
        B, flags, changed, filled = K.median(A, m)
        got = F.median_plane(A, K.to_struct(F, m))
        assert got[0].tobytes() == B.tobytes() and got[1].tobytes() == flags.tobytes() and got[2:] == (changed, filled)
        assert changed >= 20 and filled >= 20


# ---- 2. frames ---------------------------------------------------------------------------------------

def test_a_depth_frame_at_the_smallest_context(pkg):
    F = pkg.frontend
    w, h = 64, 64
    A, bgr = K.surface(w, h, 30), G.frame(w, h, 72)
    gen = _generator(pkg, w, h)
    for m in K.FRAME_SETTINGS:
        gen.set_depth_median(K.to_struct(F, m))
        assert gen.depth_median() == F.DepthMedian(*m)
        for k in range(2):                                   # (the second frame replays the captured graph)
            cloud = _depth_frame(gen, F, bgr, A, m, F.FEATURES_HSV if k else F.FEATURES_RGB)
        assert len(cloud[0]) >= 20
    gen.close()


@pytest.mark.parametrize("m", K.FRAME_SETTINGS, ids=["%d-%d" % m for m in K.FRAME_SETTINGS])
def test_a_depth_frame_with_pinholes_and_salt(pkg, m):
    """160 x 120: neither side a multiple of the tile, more than one tile each way; every plane by bytes, the cloud by
    bits against the oracle on the colour image and B"""
    F = pkg.frontend
    w, h = 160, 120
    A, bgr = K.surface(w, h, 31), G.frame(w, h, 72)
    B, flags, changed, filled = K.median(A, m)
    print("settings", m, "changed", changed, "filled", filled)
    assert changed >= 20 and (m[1] == 0 or filled >= 20) and (m[1] > 0 or filled == 0)
    gen = _generator(pkg, w, h)
    gen.set_depth_median(K.to_struct(F, m))
    for k in range(2):
        cloud = _depth_frame(gen, F, bgr, A, m, F.FEATURES_HSV if k else F.FEATURES_RGB)
        print("points", len(cloud[0]))
        assert len(cloud[0]) >= 20
    gen.close()


MEDIAN_GATE = G.make_gate(1.3, 2.3, 0.05, 1, 0)


@pytest.mark.parametrize("m", [(1, 5), (2, 0)], ids=["1-5", "2-0"])
def test_the_gate_reads_the_filtered_plane(pkg, m):
    """range, jump marks and mask act on B: GATE and RECT_DEPTH are the gate's restatement applied to B"""
    F = pkg.frontend
    w, h = 160, 120
    A, bgr = K.stepped(w, h, 31), G.frame(w, h, 72)
    mask = G.mask_scene(w, h, 72)
    B, flags, changed, filled = K.median(A, m)
    dep, gflags = G.gate(B, MEDIAN_GATE, G.SCALE, mask)
    on_a = G.gate(A, MEDIAN_GATE, G.SCALE, mask)
    for k in (G.MASKED, G.RANGE, G.JUMP):
        assert np.count_nonzero(gflags & k) >= 1
    assert np.count_nonzero(dep) >= np.count_nonzero(B) // 4 and not np.array_equal(on_a[1], gflags)
    assert np.count_nonzero(on_a[1] & G.JUMP) > np.count_nonzero(gflags & G.JUMP)     # a plane with less noise to mark
    gen = _generator(pkg, w, h)
    gen.set_depth_median(K.to_struct(F, m))
    gen.set_depth_gate(G.to_struct(F, MEDIAN_GATE))
    gen.set_mask(mask)
    assert gen.depth_median() == F.DepthMedian(*m)           # (the other setters: the setting stays)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, A, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, A, B, flags, final=dep)
        assert gen.read_stage(F.STAGE_GATE).tobytes() == gflags.tobytes()
        _cloud_equal(gen, F, cloud, bgr, dep, 1, F.FEATURES_RGB)
        assert len(cloud[0]) >= 20
    gen.set_depth_gate(None)
    gen.set_mask(None)
    assert gen.depth_median() == F.DepthMedian(*m)
    _depth_frame(gen, F, bgr, A, m)
    gen.close()


def test_a_frame_under_a_depth_camera(pkg):
    """rig K: k_fe_depth_final writes A, and the holes the forward warp leaves get filled"""
    F = pkg.frontend
    w, h, cam, rig = D.RIGS["K"]
    m = (1, 5)
    bgr = G.frame(w, h, 72)
    raw = D.scene(pkg.data, rig)
    A, = _ref("rig K", lambda: (D.register(rig, cam, w, h, raw),))
    B, flags, changed, filled = K.median(A, m)
    print("under the depth camera: holes", np.count_nonzero(A == 0), "changed", changed, "filled", filled)
    assert filled >= 20 and changed >= 20
    gen = _generator(pkg, w, h)
    gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
    gen.set_depth_median(K.to_struct(F, m))
    gen.set_depth_camera(D.to_struct(F, rig))
    assert gen.depth_median() == F.DepthMedian(*m)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, A, B, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), raw)
        assert len(cloud[0]) >= 20
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(*(cam + (ZERO,))))
    assert _same_cloud(plain.create_pointcloud(bgr, B, 1, F.FEATURES_RGB), cloud)
    plain.close(); gen.close()


def test_a_frame_under_a_distorting_model(pkg):
    """model C (an odd width): k_fe_rectify writes A"""
    F = pkg.frontend
    w, h, model = R.SMALL["C"]
    m = (2, 13)
    U0, bgr = K.surface(w, h, 32), G.frame(w, h, 72)
    qu, qv = R.rectify_map(model, w, h)
    A = R.remap_depth(U0, qu, qv)
    B, flags, changed, filled = K.median(A, m)
    assert filled >= 20 and changed >= 20
    gen = _generator(pkg, w, h)
    gen.set_depth_median(K.to_struct(F, m))
    gen.set_camera(F.CameraModel(*model))
    assert gen.depth_median() == F.DepthMedian(*m)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, U0, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, A, B, flags)
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), U0)
        rect = gen.read_stage(F.STAGE_RECT_BGR)
        assert np.array_equal(rect, R.remap_colour(bgr, qu, qv))
        assert len(cloud[0]) >= 20
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(*(model[:5] + (ZERO,))))
    assert _same_cloud(plain.create_pointcloud(rect, B, 1, F.FEATURES_RGB), cloud)
    plain.close(); gen.close()


def test_a_stereo_frame_behind_the_speckle_filter(pkg):
    """DISPARITY and STEREO stay the matcher's, byte-equal to the frame without the median; the stage reads the depth
    plane behind the speckle filter and a filled pixel has a depth and DISPARITY 0"""
    F = pkg.frontend
    name, sp, m = "default-96x64-82", (12, 16), (1, 5)
    w, h, st, left, right = P.inputs(name)
    Q = KS.case_frame(name, sp)
    A = Q["depth"]
    B, flags, changed, filled = K.median(A, m)
    print("stereo: changed", changed, "filled", filled)
    assert changed >= 2 and filled >= 20 and np.count_nonzero((flags == K.FILLED) & (Q["disparity"] == 0)) == filled
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_speckle(KS.to_struct(F, sp))
    gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    stages = (F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_SGM_SUM, F.STAGE_SPECKLE_SIZE)
    before = [gen.read_stage(s).tobytes() for s in stages]
    assert before[0] == Q["disparity"].tobytes() and before[1] == Q["flags"].tobytes()
    assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == A.tobytes()
    gen.set_depth_median(K.to_struct(F, m))
    assert gen.stereo_speckle() == F.Speckle(*sp) and gen.stereo() == S.to_struct(F, st)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        assert [gen.read_stage(s).tobytes() for s in stages] == before
        _planes_equal(gen, F, A, B, flags)
        assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == A.tobytes()
        _cloud_equal(gen, F, cloud, left, B, S.SEQ, F.FEATURES_RGB)
    gen.set_stereo(None)                                      # (the setting survives, and depth frames read it)
    assert gen.depth_median() == F.DepthMedian(*m)
    _depth_frame(gen, F, left, K.surface(w, h, 33), m)
    gen.close()


def test_a_frame_under_a_stereo_rig_selecting_by_depth(pkg):
    """rig A under CVO_FE_SELECT_DEPTH: the selector reads B, so num_points == num_selected still holds and every pixel
    of the map has a depth in B"""
    F = pkg.frontend
    w, h, st, rig, raw_l, raw_r, Q = RG.case("A")
    m = (1, 3)
    A = Q["depth"]
    B, flags, changed, filled = K.median(A, m)
    assert filled >= 20
    gen = _generator(pkg, w, h)
    gen.set_depth_median(K.to_struct(F, m))
    gen.set_select_mode(F.SELECT_DEPTH)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_rig(RG.to_struct(F, rig))
    assert gen.depth_median() == F.DepthMedian(*m)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
        _planes_equal(gen, F, A, B, flags)
        assert gen.read_stage(F.STAGE_DISPARITY).tobytes() == Q["disparity"].tobytes()
        assert gen.read_stage(F.STAGE_STEREO).tobytes() == Q["flags"].tobytes()
        info = gen.info()
        picked = gen.read_stage(F.STAGE_MAP) != 0
        assert info["canny_used"] == 0 and info["num_points"] == info["num_selected"] == len(cloud[0]) >= 20
        assert picked.any() and (B[picked] != 0).all()
    gen.set_stereo_rig(None)
    assert gen.depth_median() == F.DepthMedian(*m)
    gen.close()


# ---- 3. the context ----------------------------------------------------------------------------------

ALTERNATING = ((1, 0), (2, 13), None, (1, 5))


def test_settings_alternate_on_one_context(pkg):
    """(1, 0), (2, 13), none, (1, 5) on two alternating planes: every frame by bytes.  A graph captured under other
    settings, or without the stage, and launched again would give that frame's planes."""
    F = pkg.frontend
    w, h = 160, 120
    bgr = G.frame(w, h, 72)
    planes = [K.surface(w, h, 31), K.surface(w, h, 34)]
    gen = _generator(pkg, w, h)
    k = 0
    for m in ALTERNATING + ALTERNATING[:2]:
        gen.set_depth_median(K.to_struct(F, m))
        assert gen.depth_median() == K.to_struct(F, m)
        for _ in range(2):
            A = planes[k % 2]
            ftype = F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB
            if m is None:
                cloud = gen.create_pointcloud(bgr, A, 1, ftype)
                for stage in (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH):
                    assert gen.read_stage(stage).tobytes() == A.tobytes()
                _cloud_equal(gen, F, cloud, bgr, A, 1, ftype)
            else:
                _depth_frame(gen, F, bgr, A, m, ftype)
            k += 1
    gen.close()


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set the filter, ran a frame under it and cleared it: in bytes and in the cloud"""
    F = pkg.frontend
    w, h = 160, 120
    A, bgr = K.surface(w, h, 31), G.frame(w, h, 72)
    never, cleared = _generator(pkg, w, h), _generator(pkg, w, h)
    stages = (F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_GATE, F.STAGE_MAP, F.STAGE_AG0)
    clouds, planes = [], []
    for gen in (never, cleared):
        if gen is cleared:
            gen.set_depth_median(F.DepthMedian(2, 13))
            filtered = _depth_frame(gen, F, bgr, A, (2, 13))
            gen.set_depth_median(None)
        assert gen.depth_median() is None
        gen.set_depth_median(None)                             # clearing what is not set is no error
        clouds.append(gen.create_pointcloud(bgr, A, 1, F.FEATURES_RGB))
        planes.append([gen.read_stage(s).tobytes() for s in stages])
        assert planes[-1][2] == A.tobytes()
    assert _same_cloud(clouds[0], clouds[1]) and planes[0] == planes[1] and not _same_cloud(filtered, clouds[0])
    never.close(); cleared.close()


def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h = 160, 120
    m = (1, 5)
    A, bgr = K.surface(w, h, 31), G.frame(w, h, 72)
    gen = _generator(pkg, w, h)
    plain = gen.create_pointcloud(bgr, A, 1, F.FEATURES_RGB)
    for bad in K.bad_medians():
        with pytest.raises(Err):
            gen.set_depth_median(F.DepthMedian(*bad))         # on a context without the filter
        assert gen.depth_median() is None
    assert b"set_depth_median" in F.lib().cvo_fe_last_error(gen._h)
    for stage in (F.STAGE_UNFILTERED_DEPTH, F.STAGE_MEDIAN):
        with pytest.raises(Err):
            gen.read_stage(stage)                             # no filter: no such plane
    assert _same_cloud(gen.create_pointcloud(bgr, A, 1, F.FEATURES_RGB), plain)
    with pytest.raises(Err):
        F.median_plane(np.ones((4, 4), np.uint16), F.DepthMedian(3, 0))
    with pytest.raises(Err):
        F.median_plane(np.ones((4, 4), np.uint16), None)
    gen.set_depth_median(F.DepthMedian(*m))
    want = _depth_frame(gen, F, bgr, A, m)
    for bad in K.bad_medians():
        with pytest.raises(Err):
            gen.set_depth_median(F.DepthMedian(*bad))
        assert gen.depth_median() == F.DepthMedian(*m)
    gen.submit(bgr, A, 1, F.FEATURES_RGB)
    for other in (F.DepthMedian(2, 13), F.DepthMedian(*m), None):
        with pytest.raises(Err):
            gen.set_depth_median(other)                       # while a frame is pending, even the settings in force
    assert _same_cloud(gen.collect(), want) and gen.depth_median() == F.DepthMedian(*m)
    assert _same_cloud(_depth_frame(gen, F, bgr, A, m), want)
    gen.set_depth_median(F.DepthMedian(*m))                   # the value it has: nothing happens
    assert _same_cloud(_depth_frame(gen, F, bgr, A, m), want)
    gen.set_depth_median(None)
    for stage in (F.STAGE_UNFILTERED_DEPTH, F.STAGE_MEDIAN):
        with pytest.raises(Err):
            gen.read_stage(stage)
    assert _same_cloud(gen.create_pointcloud(bgr, A, 1, F.FEATURES_RGB), plain)
    gen.close()


def test_the_filter_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 4096 x 2048 the two planes of the stage are 24 MiB, three times the 8 MiB a reading of the free
    device memory resolves.  Refused settings leave it where it was; the first settings are seen by the same reading,
    other settings take nothing more, and clearing the filter gives all of it back."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(4096, 2048)
    free0 = free()
    for bad in K.bad_medians():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_depth_median(F.DepthMedian(*bad))
    gen.set_depth_median(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_depth_median(F.DepthMedian(1, 0))
    free2 = free()
    assert free1 - free2 >= 16 * MiB, "the first settings took only %d bytes" % (free1 - free2)
    gen.set_depth_median(F.DepthMedian(2, 13))
    free3 = free()
    assert abs(free2 - free3) < 8 * MiB, "other settings moved the free memory by %d bytes" % (free2 - free3)
    gen.set_depth_median(None)
    free4 = free()
    assert free4 - free3 >= 16 * MiB, "clearing the filter gave back only %d bytes" % (free4 - free3)
    gen.close()


# ---- 4. the layers above -----------------------------------------------------------------------------

RUN_MEDIAN = (1, 5)


def _frames(pkg):
    return _four_frames(pkg, 75, lambda k, dep: K.spoil(dep, 40 + k))


def test_run_frames_takes_the_setting(pkg):
    """run_frames(depth_median=) on the raw frames = the generator driven by hand = run_frames without it on frames
    filtered beforehand by the restatement: the same poses"""
    F = pkg.frontend
    frames = _frames(pkg)
    filtered = [(name, bgr, _ref(("seq", k), lambda: K.median(dep, RUN_MEDIAN))[0]) for k, (name, bgr, dep) in enumerate(frames)]
    assert all(not np.array_equal(f[2], g[2]) for f, g in zip(frames, filtered))
    poses = []
    for fr, m in ((frames, F.DepthMedian(*RUN_MEDIAN)), (filtered, None)):
        reg, buf = pkg.Cvo(), io.StringIO()
        gen = F.PcdGenerator(640, 480)
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen, depth_median=m) == 4
        assert gen.depth_median() == m
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == filtered[3][2].tobytes()
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close(); gen.close()
    reg, buf = pkg.Cvo(), io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(640, 480)
    gen.set_depth_median(F.DepthMedian(*RUN_MEDIAN))
    gen.set_device_output(True)
    for k, (name, bgr, dep) in enumerate(frames):
        gen.submit(bgr, dep, 1, F.FEATURES_RGB)
        dp, df, n = gen.collect_device()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == filtered[k][2].tobytes()
        reg.run_cvo_device(dp, df, n)
        writer.append(name, reg.accum_transform)
    poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
    reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_setting(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_depth_median / clear_depth_median (tests/cpp/cvo_depth_median_demo.cpp): the
    clouds the C++ object registers and its pose lines equal the Python path's"""
    F = pkg.frontend
    w, h = 640, 480
    frames = _frames(pkg)
    median = F.DepthMedian(*RUN_MEDIAN)
    got = _demo_lines(tmp_path, "cvo_depth_median_demo", frames, w, h, bytes(median), [mode_name])
    gen = F.PcdGenerator(w, h)

    def prepare(k):
        gen.set_depth_median(None if k == 2 else median)
        return ["refused bad settings"] if k == 3 else []

    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, frames, prepare)
    assert got == ["refused bad settings"] + want
    ftype = F.FEATURES_HSV if mode_name == "acvo" else F.FEATURES_RGB
    # the filtered frames' clouds are the oracle's on the restatement's plane, and larger than the unfiltered frame's:
    # the pinholes under the selector's picks are filled
    B = _ref(("seq", 0), lambda: K.median(frames[0][2], RUN_MEDIAN))[0]
    assert sizes[0] == len(fo.create_pointcloud(frames[0][1], B, 1, ftype)["positions"]) > 100
    assert sizes[2] == len(fo.create_pointcloud(frames[2][1], frames[2][2], 1, ftype)["positions"]) < min(sizes[0], sizes[1], sizes[3])
    gen.close()
