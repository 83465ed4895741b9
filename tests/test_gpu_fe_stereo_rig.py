"""GPU: a raw stereo pair with its rig (cvo_fe_set_stereo_rig, include/cvo_frontend.h): k_fe_stereo_rectify and the
matcher behind it against the numpy restatement of the rig contract (tests/fe_stereo_rig_ref.py) by bytes, stage by
stage, and, downstream of them, the CPU restatement of the front end (oracle/frontend_oracle.c) applied to the
rectified left image and the reference's depth plane: every cloud bit for bit.  Rigs that are no rig at all against
frames without one, rigs alternating on one context, the gate behind a rig frame, the refusals, the memory, run_frames
and the C++ object, and the unchanged paths without a rig.  What rigs A and B reach is asserted in
tests/test_fe_stereo_rig_cpu.py."""
import io

import numpy as np
import pytest

import fe_gate_ref as GATE
import fe_stereo_rig_ref as G
import fe_stereo_ref as S
from fe_gpu_common import _demo_lines, _digest, _pose_line_f32, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=max(200, w * h // 100))


def _stages_equal(gen, F, P):
    """every plane of a frame under a rig against frame()'s, by bytes (without a gate)"""
    for stage, want in ((F.STAGE_RECT_BGR, P["rect_l"]), (F.STAGE_RIGHT_BGR, P["rect_r"]), (F.STAGE_STEREO_VALID, P["valid"]),
                        (F.STAGE_GRAY, P["gray_l"]), (F.STAGE_RIGHT_GRAY, P["gray_r"]), (F.STAGE_CENSUS_L, P["census_l"]),
                        (F.STAGE_CENSUS_R, P["census_r"]), (F.STAGE_SGM_SUM, P["sum"]), (F.STAGE_DISPARITY, P["disparity"]),
                        (F.STAGE_STEREO, P["flags"]), (F.STAGE_RAW_DEPTH, P["depth"]), (F.STAGE_UNGATED_DEPTH, P["depth"]),
                        (F.STAGE_RECT_DEPTH, P["depth"])):
        got = gen.read_stage(stage)
        assert got.dtype == want.dtype and got.shape == want.shape, stage
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("stage %d differs at %d places, first at %s: %s against %s"
                                 % (stage, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _oracle_cloud(rect_l, depth, cam, ftype, num_want):
    """The front-end oracle on (rectified left image, depth plane) with the pinhole `cam` = (depth_scale, fx, fy, cx,
    cy) in place of its table row: selection and features do not depend on the camera; the positions are
    k_fe_emit's three float32 operations, restated here and checked against the oracle's own on its table row."""
    f = np.float32
    ref = fo.create_pointcloud(rect_l, depth, S.SEQ, ftype, num_want=num_want)
    ys, xs = np.nonzero((ref["map"] != 0) & (depth != 0))
    assert len(ys) == len(ref["positions"])

    def positions(c):
        c = [f(v) for v in c]
        z = depth[ys, xs].astype(f) / c[0]
        return np.stack([(xs.astype(f) - c[3]) * z / c[1], (ys.astype(f) - c[4]) * z / c[2], z], axis=1)

    row = fo.camera(S.SEQ)
    assert np.array_equal(positions(row).view(np.uint32), ref["positions"].view(np.uint32))
    out = positions(cam)
    assert out.dtype == f
    return dict(ref, positions=out)


def _cam(rig):
    return (rig["depth_scale"], rig["fx"], rig["fy"], rig["cx"], rig["cy"])


def _frame_equals(gen, F, rig, raw_l, raw_r, P, ftype, few=False):
    xyz, feat = gen.create_pointcloud_stereo(raw_l, raw_r, 1, ftype)   # (dataset_seq is ignored under a rig)
    _stages_equal(gen, F, P)
    ref = _oracle_cloud(P["rect_l"], P["depth"], _cam(rig), ftype, gen.num_want)
    info = gen.info()
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(xyz)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
    assert few or len(xyz) > 20
    return xyz, feat


# ---- 1. every plane by bytes and the cloud by bits ---------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_every_stage_by_bytes_and_the_cloud_by_bits(pkg, name):
    """rig A: 96 x 64 at D 32, a barrel pair that stays inside its raw images; rig B: 127 x 193 at D 48 -- an odd width,
    a pixel count that is no multiple of four (the kernel's last group goes pixel by pixel), more than one workgroup --
    a pincushion pair a quarter of whose maps leave the raw images.  Two frames each: the second replays the graph."""
    F = pkg.frontend
    w, h, st, rig, raw_l, raw_r, P = G.case(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo_rig() is None
    gen.set_stereo_rig(G.to_struct(F, rig))
    assert gen.stereo_rig() == G.to_struct(F, rig)
    cam = gen.camera()
    assert cam is not None and cam.astuple() == (rig["depth_scale"], rig["fx"], rig["fy"], rig["cx"], rig["cy"], G.ZERO)
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV, F.FEATURES_HSV):
        _frame_equals(gen, F, rig, raw_l, raw_r, P, ftype)
        assert not gen.read_stage(F.STAGE_GATE).any()
    # the library's helper gives a rig whose frame is the restatement's too (the two may differ in a last place of a
    # member: then in a few map entries at most, and the planes are compared through the library's own rig)
    own = F.stereo_rectify(G.calib_struct(F, G.CALIBS[name][3]), w, h, G.DEPTH_SCALE)
    members = np.frombuffer(bytes(own), np.float32).astype(np.float64)
    as_dict = dict(left=(tuple(members[0:4]) + (tuple(members[4:9]),)), right=(tuple(members[9:13]) + (tuple(members[13:18]),)),
                   R_left=members[18:27], R_right=members[27:36], fx=members[36], fy=members[37], cx=members[38],
                   cy=members[39], baseline=members[40], depth_scale=members[41])
    gen.set_stereo_rig(own)
    _frame_equals(gen, F, as_dict, raw_l, raw_r, P if own == G.to_struct(F, rig) else G.frame(as_dict, raw_l, raw_r, st),
                  F.FEATURES_RGB)
    gen.close()


# ---- 2, 3. rigs that are none ------------------------------------------------------------------

def _all_stages(gen, F):
    return [gen.read_stage(s).tobytes() for s in (F.STAGE_RECT_BGR, F.STAGE_RIGHT_BGR, F.STAGE_GRAY, F.STAGE_RIGHT_GRAY,
                                                  F.STAGE_CENSUS_L, F.STAGE_CENSUS_R, F.STAGE_SGM_SUM, F.STAGE_DISPARITY,
                                                  F.STAGE_STEREO, F.STAGE_RAW_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_MAP,
                                                  F.STAGE_HSV, F.STAGE_DX0)]


@pytest.mark.parametrize("flipped", [False, True])
def test_a_rig_that_is_none_gives_the_frame_without_one(pkg, flipped):
    """rig I (both cameras the rectified pinhole, no lens, no rotation) on a context of either feature type = the frame
    WITHOUT a rig under cvo_fe_set_camera(that pinhole) and Stereo(baseline=0.2), every plane by bytes and the cloud by
    bits.  `flipped`: the right camera mounted upside down -- the frame without a rig on (left, right[::-1, ::-1])."""
    F = pkg.frontend
    w = h = 64
    left, right, _ = S.pair(w, h, G.SEED)
    rig = dict(G.RIG_I, R_right=np.diag([-1.0, -1.0, 1.0]).reshape(9)) if flipped else G.RIG_I
    raw_r = np.ascontiguousarray(right[::-1, ::-1]) if flipped else right
    st = S.make_stereo(baseline=0.2)
    pinhole = F.CameraModel(G.DEPTH_SCALE, 60.0, 60.0, 31.5, 31.5)
    for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
        plain = _generator(pkg, w, h)
        plain.set_camera(pinhole)
        plain.set_stereo(S.to_struct(F, st))
        want = plain.create_pointcloud_stereo(left, right, 1, ftype)
        with pytest.raises(pkg.capi.CvoHipError):
            plain.read_stage(F.STAGE_STEREO_VALID)            # no rig: no such plane
        assert plain.read_stage(F.STAGE_RIGHT_BGR).tobytes() == right.tobytes()   # ... and the right image as uploaded
        gen = _generator(pkg, w, h)
        gen.set_stereo(S.to_struct(F, dict(st, baseline=0.9)))    # (not read under a rig)
        gen.set_stereo_rig(G.to_struct(F, rig))
        for _ in range(2):
            got = gen.create_pointcloud_stereo(left, raw_r, 4, ftype)
            assert _same_cloud(got, want) and len(want[0]) > 20
            assert _all_stages(gen, F) == _all_stages(plain, F)
            assert gen.info() == plain.info()
            assert (gen.read_stage(F.STAGE_STEREO_VALID) == 3).all()
        plain.close(); gen.close()


# ---- 4. graphs, maps and tables across changes of rig ---------------------------------------------

def test_rigs_alternate_on_one_context(pkg):
    """rig A, no rig, a second rig (A's cameras one degree further apart, 4000 units per metre: other maps, another
    table), several times on ONE context through both feature types, two frames after each: every frame is its
    reference's, and the frame without a rig the one of a context that never had one"""
    F = pkg.frontend
    w, h, st, rig_a, raw_l, raw_r, Pa = G.case("A")
    calib = G.CALIBS["A"][3]
    rig_b = G.rectify(dict(calib, R=G.f32(G.exp_so3((0.010, -0.037, 0.005))).reshape(9)), w, h, 4000.0)
    Pb = G.frame(rig_b, raw_l, raw_r, st)
    assert not np.array_equal(Pa["rect_l"], Pb["rect_l"]) and not np.array_equal(Pa["depth"], Pb["depth"])
    never = _generator(pkg, w, h)
    never.set_stereo(S.to_struct(F, st))
    plain = {ft: never.create_pointcloud_stereo(raw_l, raw_r, S.SEQ, ft) for ft in (F.FEATURES_RGB, F.FEATURES_HSV)}
    plain_stages = _all_stages(never, F)
    never.close()
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    for rounds in range(2):
        for k, (rig, P) in enumerate(((rig_a, Pa), (None, None), (rig_b, Pb), (rig_a, Pa))):
            ft = F.FEATURES_HSV if (k + rounds) % 2 else F.FEATURES_RGB
            gen.set_stereo_rig(G.to_struct(F, rig))
            assert gen.stereo_rig() == G.to_struct(F, rig)
            for _ in range(2):
                if rig is None:
                    assert gen.camera() is None
                    assert _same_cloud(gen.create_pointcloud_stereo(raw_l, raw_r, S.SEQ, ft), plain[ft])
                    if ft == F.FEATURES_HSV:
                        assert _all_stages(gen, F) == plain_stages
                else:
                    _frame_equals(gen, F, rig, raw_l, raw_r, P, ft)
    # other stereo settings under a rig are welcome, and the table follows them
    other = dict(st, min_disp=7, lr_max=0)
    gen.set_stereo(S.to_struct(F, other))
    _frame_equals(gen, F, rig_a, raw_l, raw_r, G.frame(rig_a, raw_l, raw_r, other), F.FEATURES_RGB)
    gen.close()


# ---- 5. the gate behind a rig frame ------------------------------------------------------------

def test_gate_and_mask_behind_a_rig_frame(pkg):
    """rig B: the mask lies on the raw left grid and follows the left map (a quarter of it leaves the image: masked);
    the gate reads the plane stereo wrote after OUTSIDE.  The background lies at 100.25 * 0.25 / 6 = 4.2 m and the box
    at 1.7 m: a gate from 2 m up drops the box, the jump test what lies beside a step."""
    F = pkg.frontend
    w, h, st, rig, raw_l, raw_r, P = G.case("B")
    gate = GATE.make_gate(2.0, 0.0, 0.2, 1, 0)
    mask = GATE.mask_scene(w, h, 72)
    qu, qv = G.rig_map(rig, 0, w, h)
    dep, flags = GATE.gate(P["depth"], gate, rig["depth_scale"], mask, qu, qv)
    plain_flags = GATE.gate(P["depth"], gate, rig["depth_scale"], mask)[1]
    assert not np.array_equal(flags, plain_flags)             # the map decides
    for k in (GATE.MASKED, GATE.RANGE, GATE.JUMP):
        assert np.count_nonzero(flags & k) >= 1
    assert np.count_nonzero(dep) >= np.count_nonzero(P["depth"]) // 4
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(GATE.to_struct(F, gate))
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_rig(G.to_struct(F, rig))
    gen.set_mask(mask)
    for _ in range(2):
        xyz, feat = gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
        assert gen.read_stage(F.STAGE_UNGATED_DEPTH).tobytes() == P["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == P["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep.tobytes()
        assert gen.read_stage(F.STAGE_GATE).tobytes() == flags.tobytes()
        assert gen.read_stage(F.STAGE_STEREO).tobytes() == P["flags"].tobytes()
        assert gen.read_stage(F.STAGE_STEREO_VALID).tobytes() == P["valid"].tobytes()
        ref = _oracle_cloud(P["rect_l"], dep, _cam(rig), F.FEATURES_RGB, gen.num_want)
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"])) and len(xyz) > 20
    gen.set_depth_gate(None)
    gen.set_mask(None)
    _frame_equals(gen, F, rig, raw_l, raw_r, P, F.FEATURES_RGB)
    gen.close()


# ---- 6. refusals -------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    w, h, st, rig, raw_l, raw_r, P = G.case("A")
    good = G.to_struct(F, rig)
    pinhole = F.CameraModel(*(_cam(rig) + (G.ZERO,)))
    gen = _generator(pkg, w, h)
    with pytest.raises(Err):
        gen.set_stereo_rig(good)                              # without stereo
    assert b"stereo is not set" in F.lib().cvo_fe_last_error(gen._h) and gen.stereo_rig() is None
    gen.set_stereo_rig(None)                                  # clearing what was never set is no error
    gen.set_camera(pinhole)
    gen.set_stereo(S.to_struct(F, st))
    with pytest.raises(Err):
        gen.set_stereo_rig(good)                              # beside a camera model, even one without a lens
    assert gen.stereo_rig() is None and gen.camera() == pinhole
    plain = gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
    gen.set_camera(None)
    for bad in (dict(rig, baseline=0.0), dict(rig, fx=float("nan")), dict(rig, R_left=np.diag([1.0, 1.0, -1.0]).reshape(9))):
        with pytest.raises(Err):
            gen.set_stereo_rig(G.to_struct(F, bad))
        assert gen.stereo_rig() is None
    gen.submit_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.set_stereo_rig(good)                              # while a frame is in flight
    gen.collect()
    assert gen.stereo_rig() is None
    # with a rig set
    gen.set_stereo_rig(good)
    want = _frame_equals(gen, F, rig, raw_l, raw_r, P, F.FEATURES_RGB)
    with pytest.raises(Err):
        gen.set_camera(pinhole)
    assert b"clear the rig first" in F.lib().cvo_fe_last_error(gen._h)
    with pytest.raises(Err):
        gen.set_stereo(None)
    assert b"clear the rig first" in F.lib().cvo_fe_last_error(gen._h)
    assert gen.stereo() == S.to_struct(F, st) and gen.stereo_rig() == good
    with pytest.raises(Err):
        gen.set_stereo_rig(G.to_struct(F, dict(rig, depth_scale=-1.0)))
    assert gen.stereo_rig() == good
    gen.submit_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
    for call in (lambda: gen.set_stereo_rig(None), lambda: gen.set_stereo_rig(G.to_struct(F, dict(rig, cx=40.0)))):
        with pytest.raises(Err):
            call()                                            # while a frame is in flight
    assert _same_cloud(gen.collect(), want) and gen.stereo_rig() == good
    _stages_equal(gen, F, P)
    gen.set_stereo_rig(None)
    gen.set_camera(pinhole)
    assert _same_cloud(gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB), plain)
    gen.set_camera(None)
    gen.set_stereo(None)
    gen.close()


# ---- 7. memory ---------------------------------------------------------------------------------

def test_a_rig_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 1024 x 1024 the two raw images are 6 MiB, the four map planes 16 MiB and the validity plane 1 MiB.
    Refused rigs leave the free device memory where it was, to the 8 MiB such a reading resolves; the first rig is seen
    by the same reading, a second rig takes nothing more, and clearing the rig gives all of it back."""
    import torch
    F = pkg.frontend
    n = 1024
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    lens = (900.0, 900.0, 511.5, 511.5, G.ZERO)
    rig = dict(G.RIG_I, left=lens, right=lens, fx=900.0, fy=900.0, cx=511.5, cy=511.5)
    gen = F.PcdGenerator(n, n)
    gen.set_stereo(F.Stereo(0.25, 8))
    free0 = free()
    for bad in (dict(rig, baseline=0.0), dict(rig, fy=0.0)):
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_stereo_rig(G.to_struct(F, bad))
    gen.set_stereo_rig(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_stereo_rig(G.to_struct(F, rig))
    free2 = free()
    assert free1 - free2 >= 20 * MiB, "the first rig took only %d bytes" % (free1 - free2)
    gen.set_stereo_rig(G.to_struct(F, dict(rig, cx=500.0)))
    free3 = free()
    assert abs(free2 - free3) < 8 * MiB, "a second rig moved the free memory by %d bytes" % (free2 - free3)
    gen.set_stereo_rig(None)
    free4 = free()
    assert free4 - free3 >= 15 * MiB, "clearing the rig gave back only %d bytes" % (free4 - free3)
    gen.close()


# ---- 8. the layers above -----------------------------------------------------------------------

def _rig_192():
    """rig A at twice the size (the same lenses and rotation): 192 x 128, an even width for the C++ demo's file"""
    calib = G.CALIBS["A"][3]
    big = lambda lens: tuple(2.0 * v for v in lens[:4]) + (lens[4],)
    return G.rectify(G.make_calib(big(calib["left"]), big(calib["right"]), (0.010, -0.020, 0.005), (-0.11, 0.0004, -0.0008)),
                     192, 128, G.DEPTH_SCALE)


def _raw_pairs(rig, n):
    """n raw pairs of one texture, the box coming nearer, with their rectified originals' names"""
    return [("%d.5" % (100 + k),) + G.render(rig, 192, 128, 84, box=15.0 + k, back=6.0) for k in range(n)]


def test_run_frames_on_raw_pairs(pkg):
    """run_frames(stereo=, stereo_rig=) on three raw pairs = run_frames without a rig on the pairs rectified by the
    restatement, under the rig's pinhole and baseline (the rig's maps stay inside the raw images: no OUTSIDE): the same
    poses, with and without prefetch"""
    F = pkg.frontend
    w, h = 192, 128
    rig = _rig_192()
    st = S.make_stereo()
    raw = _raw_pairs(rig, 3)
    rect, last = [], None
    for name, raw_l, raw_r in raw:
        last = G.frame(rig, raw_l, raw_r, st)
        assert not (last["flags"] & G.OUTSIDE).any()
        rect.append((name, last["rect_l"], last["rect_r"]))
    pinhole = F.CameraModel(*(_cam(rig) + (G.ZERO,)))
    poses = []
    for frames, kw in ((raw, dict(stereo=S.to_struct(F, st), stereo_rig=G.to_struct(F, rig))),
                       (rect, dict(stereo=S.to_struct(F, dict(st, baseline=rig["baseline"])), camera=pinhole))):
        for prefetch in (False, True):
            reg = pkg.Cvo()
            buf = io.StringIO()
            gen = F.PcdGenerator(w, h, num_want=1500)
            assert F.run_frames(reg, frames, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen,
                                prefetch=prefetch, **kw) == 3
            assert gen.info()["num_points"] > 100
            assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == last["depth"].tobytes()
            assert gen.read_stage(F.STAGE_RECT_BGR).tobytes() == last["rect_l"].tobytes()
            poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
            reg.close(); gen.close()
    for p in poses[1:]:
        assert p[0] == poses[0][0] and np.array_equal(p[1], poses[0][1]) and p[2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 3


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_a_raw_pair(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_stereo_rig / clear_stereo_rig (tests/cpp/cvo_stereo_rig_demo.cpp): the clouds
    the C++ object registers and its pose lines equal the Python path's with the hand-over the object uses"""
    F = pkg.frontend
    w, h = 192, 128
    rig = _rig_192()
    st = S.make_stereo()
    pairs = _raw_pairs(rig, 3)
    frames = [(name, left, np.ascontiguousarray(right).reshape(h, w * 3).view(np.uint16)) for name, left, right in pairs]
    settings = bytes(S.to_struct(F, st)) + bytes(G.to_struct(F, rig))
    got = _demo_lines(tmp_path, "cvo_stereo_rig_demo", frames, w, h, settings, [mode_name], depth_sizes=True)
    acvo = mode_name == "acvo"
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    gen.set_device_output(True)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_rig(G.to_struct(F, rig))
    want = ["refused a rig without settings", "refused a bad rig"]
    sizes = []
    for k, (name, left, right) in enumerate(pairs):
        if k == 2:
            want += ["refused a bad rig", "refused a camera model under a rig", "refused clear_stereo under a rig"]
            gen.set_stereo_rig(None)
            gen.set_stereo_rig(G.to_struct(F, rig))
        gen.submit_stereo(left, right, 4, ftype)
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
    P = G.frame(rig, pairs[0][1], pairs[0][2], st)
    assert sizes[0] == len(_oracle_cloud(P["rect_l"], P["depth"], _cam(rig), ftype, 3000)["positions"]) > 100


# ---- 9. nothing changes without a rig ----------------------------------------------------------

def test_without_a_rig_nothing_changes(pkg):
    """a stereo frame and a depth frame on fresh contexts equal their references, and so they do on a context that had
    a rig and has none any more"""
    F = pkg.frontend
    name = "default-96x64-81"
    w, h = S.CASES[name][:2]
    st, left, right, _ = S.case_inputs(name)
    P = S.case_planes(name)
    rig = G.case("A")[3]
    dep0 = GATE.gate_scene(w, h, 73, "blocks")
    had = _generator(pkg, w, h)
    had.set_stereo(S.to_struct(F, st))
    had.set_stereo_rig(G.to_struct(F, rig))
    had.create_pointcloud_stereo(left, right, 1, F.FEATURES_RGB)
    had.set_stereo_rig(None)
    fresh = _generator(pkg, w, h)
    fresh.set_stereo(S.to_struct(F, st))
    for gen in (fresh, had):
        for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
            xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, ftype)
            for stage, want in ((F.STAGE_GRAY, P["gray_l"]), (F.STAGE_RIGHT_GRAY, P["gray_r"]), (F.STAGE_SGM_SUM, P["sum"]),
                                (F.STAGE_DISPARITY, P["disparity"]), (F.STAGE_STEREO, P["flags"]), (F.STAGE_RECT_DEPTH, P["depth"]),
                                (F.STAGE_RECT_BGR, left), (F.STAGE_RIGHT_BGR, right)):
                assert gen.read_stage(stage).tobytes() == want.tobytes(), stage
            ref = fo.create_pointcloud(left, P["depth"], S.SEQ, ftype, num_want=gen.num_want)
            assert _same_cloud((xyz, feat), (ref["positions"], ref["features"])) and len(xyz) > 20
            with pytest.raises(pkg.capi.CvoHipError):
                gen.read_stage(F.STAGE_STEREO_VALID)
        gen.set_stereo(None)
        for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
            ref = fo.create_pointcloud(left, dep0, 1, ftype, num_want=gen.num_want)
            assert _same_cloud(gen.create_pointcloud(left, dep0, 1, ftype), (ref["positions"], ref["features"]))
            assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep0.tobytes()
            with pytest.raises(pkg.capi.CvoHipError):
                gen.read_stage(F.STAGE_RIGHT_BGR)
        gen.close()
