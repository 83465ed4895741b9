"""GPU: a stereo pair in place of the depth image (cvo_fe_set_stereo, cvo_fe_submit_stereo, include/cvo_frontend.h):
the kernels of csrc/cvo_stereo.hip against the numpy restatement of the stereo contract (tests/fe_stereo_ref.py) by
bytes, stage by stage, and, downstream of them, the CPU restatement of the front end (oracle/frontend_oracle.c)
applied to the left image and the reference's depth plane: every cloud bit for bit.  The gate behind the matcher, the
captured graphs across changes of settings and camera, the unchanged path without stereo, the three ways of taking a
cloud, the refusals, the memory, and run_frames, run_stereo_directory and the C++ objects above; last, the edge cases: the seam
between a lane's two disparities, the ends of D, extreme settings, hostile images.  What the shared cases and the edge
cases reach is asserted in tests/test_fe_stereo_cpu.py."""
import ctypes as C
import io

import numpy as np
import pytest

import fe_gate_ref as G
import fe_stereo_ref as S
from fe_gpu_common import _demo_lines, _digest, _pose_line_f32, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=max(200, w * h // 100))


def _stages_equal(gen, F, P, left):
    """every plane of a stereo frame against match()'s, by bytes (without a gate)"""
    for stage, want in ((F.STAGE_GRAY, P["gray_l"]), (F.STAGE_RIGHT_GRAY, P["gray_r"]), (F.STAGE_CENSUS_L, P["census_l"]),
                        (F.STAGE_CENSUS_R, P["census_r"]), (F.STAGE_SGM_SUM, P["sum"]), (F.STAGE_DISPARITY, P["disparity"]),
                        (F.STAGE_STEREO, P["flags"]), (F.STAGE_RAW_DEPTH, P["depth"]), (F.STAGE_UNGATED_DEPTH, P["depth"]),
                        (F.STAGE_RECT_DEPTH, P["depth"]), (F.STAGE_RECT_BGR, left)):
        got = gen.read_stage(stage)
        assert got.dtype == want.dtype and got.shape == want.shape, stage
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("stage %d differs at %d places, first at %s: %s against %s"
                                 % (stage, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- 1. every plane by bytes and the cloud by bits ---------------------------------------------

@pytest.mark.parametrize("name", list(S.CASES))
def test_every_stage_by_bytes_and_the_cloud_by_bits(pkg, name):
    """Every shared case: 64 x 64 (the smallest image), 96 x 64 and 127 x 193 at D 48 (an odd width, neither side a
    multiple of any tile or chunk of steps, a D that is no power of two), three seeds; D 128 (two disparities per
    lane) with winners beyond 64; the tests switched off one by one; a texture-free pair."""
    F = pkg.frontend
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    P = S.case_planes(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo() == S.to_struct(F, st)
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
        xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, ftype)
        _stages_equal(gen, F, P, left)
        assert not gen.read_stage(F.STAGE_GATE).any()
        ref = fo.create_pointcloud(left, P["depth"], S.SEQ, ftype, num_want=gen.num_want)
        info = gen.info()
        assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(xyz)
        assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
        assert len(xyz) > 20 or name == "flat"
    gen.close()


def test_a_callers_camera_gives_the_table(pkg):
    """fx and depth_scale of the cvo_fe_set_camera model (no distortion) in place of the table row, whatever dataset_seq
    says; the model cleared: the row again"""
    F = pkg.frontend
    name = "default-96x64-81"
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    cam = (1000.0, 500.0, 510.0, 47.5, 31.5)
    own = S.match(left, right, st, cam[1], cam[0])
    row = S.case_planes(name)
    assert not np.array_equal(own["depth"], row["depth"]) and np.array_equal(own["sum"], row["sum"])
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    for _ in range(2):
        gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
        cloud = gen.create_pointcloud_stereo(left, right, 1, F.FEATURES_RGB)
        _stages_equal(gen, F, own, left)
        fresh = _generator(pkg, w, h)
        fresh.set_camera(F.CameraModel(*(cam + (ZERO,))))
        assert _same_cloud(fresh.create_pointcloud(left, own["depth"], 1, F.FEATURES_RGB), cloud) and len(cloud[0]) > 20
        fresh.close()
        gen.set_camera(None)
        gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        _stages_equal(gen, F, row, left)
    # row 5 has another focal length: another table on the same context, with the graphs of both kept
    five = S.match(left, right, st, F.camera(5)["fx"], F.camera(5)["scaling_factor"])
    assert not np.array_equal(five["depth"], row["depth"])
    for _ in range(2):
        gen.create_pointcloud_stereo(left, right, 5, F.FEATURES_RGB)
        _stages_equal(gen, F, five, left)
        gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        _stages_equal(gen, F, row, left)
    gen.close()


# ---- 2. the gate behind the matcher ------------------------------------------------------------

def test_gate_and_mask_read_the_stereo_plane(pkg):
    """the background at 6 pixels lies at 30 m and the box at 15 pixels at 12 m (2000 units per metre): a gate of
    13 m and up drops the box and a jump test of 20 % what lies on or beside a step of the plane stereo wrote (the
    plane's own sub-pixel ripple stays below it; measured on the reference: 493 pixels by the jump test alone)"""
    F = pkg.frontend
    name = "default-127x193-82"
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    P = S.case_planes(name)
    gate = G.make_gate(13.0, 0.0, 0.2, 1, 0)
    mask = G.mask_scene(w, h, 72)
    dep, flags = G.gate(P["depth"], gate, S.SCALE, mask)
    for k in (G.MASKED, G.RANGE, G.JUMP):
        assert np.count_nonzero(flags == k) >= 1
    assert np.count_nonzero(dep) >= np.count_nonzero(P["depth"]) // 4
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_stereo(S.to_struct(F, st))
    gen.set_mask(mask)
    for _ in range(2):
        xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        assert gen.read_stage(F.STAGE_UNGATED_DEPTH).tobytes() == P["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == P["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep.tobytes()
        assert gen.read_stage(F.STAGE_GATE).tobytes() == flags.tobytes()
        assert gen.read_stage(F.STAGE_STEREO).tobytes() == P["flags"].tobytes()
        assert gen.read_stage(F.STAGE_DISPARITY).tobytes() == P["disparity"].tobytes()
        ref = fo.create_pointcloud(left, dep, S.SEQ, F.FEATURES_RGB, num_want=gen.num_want)
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"])) and len(xyz) > 20
    # the gate cleared under stereo: the three depth stages are one plane again
    gen.set_depth_gate(None)
    gen.set_mask(None)
    gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    _stages_equal(gen, F, P, left)
    gen.close()


# ---- 3. graphs and order -----------------------------------------------------------------------

def test_stereo_frames_alternate_with_changes_of_settings(pkg):
    """a depth frame before stereo was ever set; settings A, B, A at D 48 (other cost sums), none, A again, on ONE
    context, two frames after each, through both feature types: every plane is the reference's, every cloud the one a
    fresh context gives, and a depth frame after set_stereo(None) equals the one before, by bytes"""
    F = pkg.frontend
    name = "default-96x64-83"
    w, h = S.CASES[name][:2]
    a, left, right, _ = S.case_inputs(name)
    b = S.make_stereo(p1=3, p2=90, uniqueness=0, lr_max=0, min_disp=5)
    c = dict(a, max_disp=48)
    dep0 = G.gate_scene(w, h, 73, "blocks")
    refs = {id(s): S.match(left, right, s, S.FX, S.SCALE) for s in (a, b, c)}
    assert not np.array_equal(refs[id(a)]["flags"], refs[id(b)]["flags"])
    assert not np.array_equal(refs[id(a)]["sum"][:, :, :32], refs[id(c)]["sum"][:, :, :32])
    gen = _generator(pkg, w, h)
    before = {ft: gen.create_pointcloud(left, dep0, 1, ft) for ft in (F.FEATURES_RGB, F.FEATURES_HSV)}
    assert gen.stereo() is None and len(before[F.FEATURES_RGB][0]) > 20
    want = {}
    for ft in (F.FEATURES_RGB, F.FEATURES_HSV):
        for s in (a, b, c):
            fresh = _generator(pkg, w, h)
            want[(ft, id(s))] = fresh.create_pointcloud(left, refs[id(s)]["depth"], S.SEQ, ft)
            fresh.close()
    for rounds in range(2):
        for k, s in enumerate((a, b, c, None, a)):
            ft = F.FEATURES_HSV if (k + rounds) % 2 else F.FEATURES_RGB
            gen.set_stereo(S.to_struct(F, s))
            assert gen.stereo() == S.to_struct(F, s)
            for _ in range(2):
                if s is None:
                    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, ft), before[ft])
                    assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep0.tobytes()
                    assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == dep0.tobytes()
                else:
                    assert _same_cloud(gen.create_pointcloud_stereo(left, right, S.SEQ, ft), want[(ft, id(s))])
                    _stages_equal(gen, F, refs[id(s)], left)
    gen.close()


def test_the_three_ways_of_taking_a_cloud(pkg):
    F = pkg.frontend
    name = "default-127x193-81"
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    P = S.case_planes(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_HSV)
    assert len(cloud[0]) > 20
    canon = pkg.capi.Context(mode=pkg.capi.MODE_ACVO)

    def canonical(n):
        d = canon.device_cloud(0)
        assert d["points"] == n
        rows = np.concatenate([d["pos"][:n], d["feat"][:n]], axis=1).view(np.uint32)
        return rows[np.lexsort(rows.T[::-1])].tobytes()

    canon.set_fixed(cloud[0], cloud[1])
    want = canonical(len(cloud[0]))
    padded = np.zeros((h, w + 3, 3), np.uint8)                # rows further apart than they are long
    padded[:, :w] = right
    for device_output in (False, True):
        gen.set_device_output(device_output)
        gen.submit_stereo(left, right, S.SEQ, F.FEATURES_HSV)
        assert _same_cloud(gen.collect(), cloud)
        gen.submit_stereo(left, right, S.SEQ, F.FEATURES_HSV)
        dp, df, n = gen.collect_device()
        assert n == len(cloud[0]) == gen.info()["num_points"]
        canon.set_fixed_device(dp, df, n)
        assert canonical(n) == want
        u8p = C.POINTER(C.c_uint8)
        assert F.lib().cvo_fe_submit_stereo(gen._h, left.ctypes.data_as(u8p), w * 3, padded.ctypes.data_as(u8p), (w + 3) * 3,
                                            S.SEQ, F.FEATURES_HSV) == 0
        assert _same_cloud(gen.collect(), cloud)
        _stages_equal(gen, F, P, left)
    first = None
    for _ in range(10):                                       # repeats give the same bytes
        got = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_HSV)
        assert _same_cloud(got, cloud)
        s = gen.read_stage(F.STAGE_SGM_SUM).tobytes()
        first = first or s
        assert s == first
    canon.close(); gen.close()


# ---- 4. nothing changes without stereo ---------------------------------------------------------

def test_without_stereo_nothing_changes(pkg):
    F = pkg.frontend
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=72, texture=1.0)
    never = F.PcdGenerator(640, 480)
    want = {ft: never.create_pointcloud(bgr, dep, 1, ft) for ft in (F.FEATURES_RGB, F.FEATURES_HSV)}
    ref = fo.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert _same_cloud(want[F.FEATURES_RGB], (ref["positions"], ref["features"]))
    assert never.stereo() is None
    never.set_stereo(None)                                    # clearing what was never set is no error
    for stage in (F.STAGE_RIGHT_GRAY, F.STAGE_CENSUS_L, F.STAGE_CENSUS_R, F.STAGE_SGM_SUM, F.STAGE_DISPARITY, F.STAGE_STEREO):
        with pytest.raises(pkg.capi.CvoHipError):
            never.read_stage(stage)
    had = F.PcdGenerator(640, 480)
    had.set_stereo(F.Stereo(0.25, 16))
    right = np.ascontiguousarray(np.roll(bgr, -6, axis=1))
    assert not _same_cloud(had.create_pointcloud_stereo(bgr, right, 4, F.FEATURES_RGB), want[F.FEATURES_RGB])
    had.set_stereo(None)
    for ft, cloud in want.items():
        assert _same_cloud(had.create_pointcloud(bgr, dep, 1, ft), cloud) and len(cloud[0]) > 1000
        assert np.array_equal(had.read_stage(F.STAGE_RECT_DEPTH), dep) and np.array_equal(had.read_stage(F.STAGE_RAW_DEPTH), dep)
    never.close(); had.close()


# ---- 5. refusals -------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    name = "default-96x64-81"
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    P = S.case_planes(name)
    good = S.to_struct(F, st)
    dep0 = G.gate_scene(w, h, 73, "blocks")
    bent = F.CameraModel(2000.0, 700.0, 700.0, 48.0, 32.0, (0.05, -0.02, 0.001, 0.001, 0.0))
    straight = F.CameraModel(2000.0, 700.0, 700.0, 48.0, 32.0)
    rig = F.DepthCamera(w, h, 2000.0, 700.0, 700.0, 48.0, 32.0)
    gen = _generator(pkg, w, h)
    # without stereo set: the stereo forms refuse, and what set_stereo refuses leaves the context without
    table = gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    assert b"stereo" in F.lib().cvo_fe_last_error(gen._h)
    for bad in S.bad_stereos():
        with pytest.raises(Err):
            gen.set_stereo(F.Stereo(**bad))
        assert gen.stereo() is None
    gen.set_depth_camera(rig)
    with pytest.raises(Err):
        gen.set_stereo(good)                                  # while a depth camera is set
    gen.set_depth_camera(None)
    gen.set_camera(bent)
    with pytest.raises(Err):
        gen.set_stereo(good)                                  # while a model with a non-zero dist is set
    assert gen.stereo() is None and gen.camera() == bent
    gen.set_camera(None)
    gen.submit(left, dep0, 1, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.set_stereo(good)                                  # while a frame is pending
    assert _same_cloud(gen.collect(), table) and gen.stereo() is None
    # with stereo set
    gen.set_stereo(good)
    want = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    assert len(want[0]) > 20
    for bad in S.bad_stereos():
        with pytest.raises(Err):
            gen.set_stereo(F.Stereo(**bad))
        assert gen.stereo() == good
    with pytest.raises(Err):
        gen.set_depth_camera(rig)
    assert gen.depth_camera() is None
    with pytest.raises(Err):
        gen.set_camera(bent)
    assert gen.camera() is None
    gen.set_camera(straight)                                  # (a model without distortion is welcome)
    gen.set_camera(None)
    with pytest.raises(Err):
        gen.submit(left, dep0, 1, F.FEATURES_RGB)             # the depth forms
    with pytest.raises(Err):
        gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB)
    with pytest.raises(ValueError):
        gen.submit_stereo(left, right[:, :-1], S.SEQ, F.FEATURES_RGB)
    u8p = C.POINTER(C.c_uint8)
    L = F.lib()
    assert L.cvo_fe_submit_stereo(gen._h, left.ctypes.data_as(u8p), w * 3, right.ctypes.data_as(u8p), w * 3 - 1, S.SEQ, 1) != 0
    assert L.cvo_fe_submit_stereo(gen._h, left.ctypes.data_as(u8p), w * 3, None, w * 3, S.SEQ, 1) != 0
    assert L.cvo_fe_submit_stereo(gen._h, left.ctypes.data_as(u8p), w * 3, right.ctypes.data_as(u8p), w * 3, S.SEQ, 7) != 0
    gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    for call in (lambda: gen.set_stereo(F.Stereo(0.3, 16)), lambda: gen.set_stereo(None),
                 lambda: gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)):
        with pytest.raises(Err):
            call()                                            # while a frame is pending
    assert _same_cloud(gen.collect(), want) and gen.stereo() == good
    _stages_equal(gen, F, P, left)
    gen.set_stereo(None)
    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB), table)
    gen.close()


def test_stereo_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 1024 x 1024 at D 32 the cost sums are 64 MiB and the other planes 29 MiB more.  Refused settings
    leave the free device memory where it was, to the 8 MiB such a reading resolves; accepted ones are seen by the same
    reading; set_stereo(None) gives the cost sums back, and a closed context everything (four rounds, as the gate's)."""
    import torch
    F = pkg.frontend
    n = 1024
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(n, n)
    free0 = free()
    for bad in S.bad_stereos():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_stereo(F.Stereo(**bad))
    gen.set_stereo(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_stereo(F.Stereo(0.25, 32))
    free2 = free()
    assert free1 - free2 >= 80 * MiB, "accepted settings took only %d bytes" % (free1 - free2)
    gen.set_stereo(None)
    free3 = free()
    assert free3 - free2 >= 56 * MiB, "set_stereo(None) gave back only %d bytes" % (free3 - free2)
    gen.close()

    def one_round():
        g = F.PcdGenerator(n, n)
        g.set_stereo(F.Stereo(0.25, 32))
        g.set_stereo(F.Stereo(0.25, 64))
        g.close()
        return free()

    left = [one_round() for _ in range(5)]
    print("free device memory after each round:", left)
    assert abs(left[0] - left[4]) < 8 * MiB, "four closed contexts left %d bytes taken" % (left[0] - left[4])


# ---- 6. the layer above ------------------------------------------------------------------------

def test_run_frames_on_stereo_pairs(pkg):
    """run_frames(stereo=) on four synthetic pairs (one texture, the box coming nearer) = run_frames without stereo on
    the left images and the reference's depth planes: the same poses"""
    F = pkg.frontend
    w, h = 192, 128
    st = S.make_stereo()
    pairs, planes = [], []
    for k in range(4):
        left, right, _ = S.pair(w, h, 84, box=15.0 + k, back=6.0)
        name = "%e" % (0.1 * k)
        pairs.append((name, left, right))
        planes.append((name, left, S.match(left, right, st, S.FX, S.SCALE)["depth"]))
    poses = []
    for frames, stereo in ((pairs, S.to_struct(F, st)), (planes, None)):
        for prefetch in (False, True):
            reg = pkg.Cvo()
            buf = io.StringIO()
            gen = F.PcdGenerator(w, h, num_want=1500)
            assert F.run_frames(reg, frames, S.SEQ, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen,
                                prefetch=prefetch, stereo=stereo) == 4
            assert gen.info()["num_points"] > 100
            if stereo is not None:
                assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == planes[3][2].tobytes()
            poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
            reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


def _run_pairs(pkg):
    """four pairs of one texture, the box coming nearer (an even width: the C++ demo's file)"""
    return [("%d.5" % (100 + k),) + S.pair(192, 128, 84, box=15.0 + k, back=6.0)[:2] for k in range(4)]


def test_run_stereo_directory_reads_the_kitti_layout(pkg, tmp_path):
    """times.txt, image_2/%06d.png and image_3/%06d.png (the right one grey: replicated) = run_frames on the arrays"""
    from PIL import Image
    F = pkg.frontend
    w, h = 192, 128
    st = S.to_struct(F, S.make_stereo())
    pairs = []
    (tmp_path / "image_2").mkdir(); (tmp_path / "image_3").mkdir()
    for k, (name, left, right) in enumerate(_run_pairs(pkg)[:3]):
        grey = np.ascontiguousarray(np.repeat(S.grey(right)[:, :, None], 3, axis=2))
        Image.fromarray(left[:, :, ::-1]).save(str(tmp_path / "image_2" / ("%06d.png" % k)))
        Image.fromarray(grey[:, :, 0]).save(str(tmp_path / "image_3" / ("%06d.png" % k)))
        pairs.append((name, left, grey))
    (tmp_path / "times.txt").write_text("".join(name + "\n" for name, _, _ in pairs))
    out = []
    for run in (lambda reg, wr, gen: F.run_stereo_directory(reg, str(tmp_path), S.SEQ, st, writer=wr, generator=gen),
                lambda reg, wr, gen: F.run_frames(reg, pairs, S.SEQ, writer=wr, generator=gen, stereo=st)):
        reg = pkg.Cvo()
        buf = io.StringIO()
        gen = F.PcdGenerator(w, h, num_want=1500)
        assert run(reg, pkg.trajectory.TrajectoryWriter(buf), gen) == 3
        out.append((buf.getvalue(), gen.read_stage(F.STAGE_RIGHT_GRAY).tobytes(), reg.num_iterations))
        reg.close(); gen.close()
    assert out[0] == out[1] and out[0][1] == S.grey(pairs[2][2]).tobytes() and out[0][2] > 0
    assert [line.split()[0] for line in out[0][0].strip().split("\n")] == [name for name, _, _ in pairs]


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_a_stereo_pair(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_stereo / run_cvo_stereo (tests/cpp/cvo_stereo_demo.cpp): the clouds the C++
    object registers and its pose lines equal the Python path's with the hand-over the object uses (device memory)"""
    F = pkg.frontend
    w, h = 192, 128
    pairs = _run_pairs(pkg)
    st = S.make_stereo()
    no_lr = dict(st, lr_max=-1)
    # (the demo's file stores a frame's second image as uint16 behind its own size: the right image's bytes, as they are)
    frames = [(name, left, np.ascontiguousarray(right).reshape(h, w * 3).view(np.uint16)) for name, left, right in pairs]
    got = _demo_lines(tmp_path, "cvo_stereo_demo", frames, w, h, bytes(S.to_struct(F, st)), [mode_name], depth_sizes=True)
    acvo = mode_name == "acvo"
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    gen.set_device_output(True)
    want = ["refused a pair without settings", "refused bad settings"]
    sizes = []
    for k, (name, left, right) in enumerate(pairs):
        gen.set_stereo(S.to_struct(F, no_lr if k == 2 else st))
        if k == 3:
            want += ["refused bad settings", "refused a depth frame under stereo"]
        gen.submit_stereo(left, right, S.SEQ, ftype)
        dp, df, n = gen.collect_device()
        sizes.append(n)
        reg.run_cvo_device(dp, df, n)
        d = reg.ctx.device_cloud(0)
        assert d["points"] == n
        want.append("cloud %s %d %d %d" % (name, n, _digest(d["pos"][:n]), _digest(d["feat"][:n])))
        want.append(_pose_line_f32(name, reg.accum_transform))
    want.append("points_last_frame %d iterations %d" % (sizes[-1], reg.num_iterations))
    reg.close(); gen.close()
    assert got == want
    depth = S.match(pairs[0][1], pairs[0][2], st, S.FX, S.SCALE)["depth"]
    assert sizes[0] == len(fo.create_pointcloud(pairs[0][1], depth, S.SEQ, ftype)["positions"]) > 100
    assert sizes[2] > sizes[1]                                # without the left-right test more pixels keep a depth


# ---- 7. the seam between a lane's two disparities, the ends of D, extreme settings, hostile images ---------------

def _edge_frame(gen, F, name, left, right, P, ftype):
    """one frame of an edge case: every plane by bytes, the cloud against the front-end oracle by bits, and an empty
    cloud where the reference keeps nothing"""
    xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, ftype)
    _stages_equal(gen, F, P, left)
    info = gen.info()
    ref = fo.create_pointcloud(left, P["depth"], S.SEQ, ftype, num_want=gen.num_want)
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(xyz)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
    if not P["depth"].any():
        assert len(xyz) == 0 and len(feat) == 0 and info["num_points"] == 0, name
    else:
        assert len(xyz) > 20 or np.count_nonzero(P["depth"]) <= 200, name


@pytest.mark.parametrize("name", list(S.EDGE_CASES))
def test_edge_cases_by_bytes_on_two_frames(pkg, name):
    """Every case of EDGE_CASES (what each reaches, and which error of the device it would show, is asserted in
    tests/test_fe_stereo_cpu.py) on two consecutive frames of one context -- the second replays the captured graph --
    with the other feature type between them.  seam-128 also takes its left image with padded rows, and switches D on
    the one context 128 -> 64 -> 72 -> 8 -> 128 with a frame after each: both kernel templates (one and two
    disparities per lane) and the cost sums allocated anew across D = 64."""
    F = pkg.frontend
    w, h = S.EDGE_CASES[name][:2]
    st, left, right, _ = S.edge_inputs(name)
    P = S.edge_planes(name)
    # (an eighth of the pixels wanted: the 133 and 164 pixels the lr0 seam scenes keep still give 17 and 24 points)
    gen = pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)
    gen.set_stereo(S.to_struct(F, st))
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV, F.FEATURES_HSV):
        _edge_frame(gen, F, name, left, right, P, ftype)
    if name == "seam-128":
        want = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_HSV)
        padded = np.zeros((h, w + 5, 3), np.uint8)            # rows further apart than they are long
        padded[:, :w] = left
        padded[:, w:] = 255
        u8p = C.POINTER(C.c_uint8)
        for _ in range(2):
            assert F.lib().cvo_fe_submit_stereo(gen._h, padded.ctypes.data_as(u8p), (w + 5) * 3, right.ctypes.data_as(u8p),
                                                w * 3, S.SEQ, F.FEATURES_HSV) == 0
            assert _same_cloud(gen.collect(), want) and len(want[0]) > 20
            _stages_equal(gen, F, P, left)
        # D 8 has no case of this size: full-64's pair under d8's settings
        st8 = S.EDGE_CASES["d8"][2]
        _, left8, right8, _ = S.edge_inputs("full-64")
        P8 = S.match(left8, right8, st8, S.FX, S.SCALE)
        assert np.count_nonzero(P8["depth"]) > 1000
        for other in ("full-64", "seam-72", None, "seam-128"):
            if other is None:
                s, l, r, Q = st8, left8, right8, P8
            else:
                assert S.EDGE_CASES[other][:2] == (w, h)
                s, l, r, _ = S.edge_inputs(other)
                Q = S.edge_planes(other)
            gen.set_stereo(S.to_struct(F, s))
            assert gen.stereo() == S.to_struct(F, s)
            for ftype in (F.FEATURES_RGB, F.FEATURES_RGB):
                _edge_frame(gen, F, other or "d8 on full-64's pair", l, r, Q, ftype)
    gen.close()
