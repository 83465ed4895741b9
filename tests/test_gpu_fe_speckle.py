"""GPU: the speckle filter of the stereo matcher (cvo_fe_set_stereo_speckle, cvo_fe_filter_speckles; the speckle contract
of include/cvo_frontend.h): the kernels of csrc/cvo_speckle.hip against the restatement tests/fe_speckle_ref.py by bytes --
the filtered plane, SIZE and the count of removed pixels on every plane made on purpose, and every plane of a stereo
frame behind the filter -- and the cloud by bits against the CPU restatement of the front end (oracle/frontend_oracle.c)
on the left image and the filtered depth plane.  Settings alternating on one context (a stale captured graph would
show), a frame under a rig, behind a gate, with eight paths; a context that never made the call; the refusals, what the
setting survives, the memory, run_frames and the C++ objects above.  What the cases reach, and which errors of a tiled
labelling they would show, is asserted in tests/test_fe_speckle_cpu.py."""
import io

import numpy as np
import pytest

import fe_gate_ref as G
import fe_speckle_ref as K
import fe_stereo_paths_ref as P
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
from fe_gpu_common import _demo_lines, _digest, _pose_line_f32, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu


def _generator(pkg, w, h):
    # (an eighth of the pixels wanted, as for the edge cases of test_gpu_fe_stereo.py)
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _stages(F, Q, left, filtered):
    out = [(F.STAGE_GRAY, Q["gray_l"]), (F.STAGE_RIGHT_GRAY, Q["gray_r"]), (F.STAGE_CENSUS_L, Q["census_l"]),
           (F.STAGE_CENSUS_R, Q["census_r"]), (F.STAGE_SGM_SUM, Q["sum"]), (F.STAGE_DISPARITY, Q["disparity"]),
           (F.STAGE_STEREO, Q["flags"]), (F.STAGE_RAW_DEPTH, Q["depth"]), (F.STAGE_UNGATED_DEPTH, Q["depth"]),
           (F.STAGE_RECT_DEPTH, Q["depth"]), (F.STAGE_RECT_BGR, left)]
    return out + [(F.STAGE_SPECKLE_SIZE, Q["sizes"])] if filtered else out


def _stages_equal(gen, stages):
    for stage, want in stages:
        got = gen.read_stage(stage)
        assert got.dtype == want.dtype and got.shape == want.shape, stage
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("stage %d differs at %d places, first at %s: %s against %s"
                                 % (stage, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _frame(gen, F, left, right, Q, ftype=None, filtered=True):
    """one frame: every plane by bytes (Q: the restatement's, behind the filter if one is set), the cloud against the
    front-end oracle on the filtered depth by bits"""
    ftype = F.FEATURES_RGB if ftype is None else ftype
    xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, ftype)
    _stages_equal(gen, _stages(F, Q, left, filtered))
    info = gen.info()
    ref = fo.create_pointcloud(left, Q["depth"], S.SEQ, ftype, num_want=gen.num_want)
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(xyz)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
    assert len(xyz) > 0 or not Q["depth"].any()
    return xyz, feat


# ---- 1. the labelling on planes made on purpose ------------------------------------------------

@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_filter_speckles_on_a_made_plane(pkg, name):
    """the serpentine and the blobs at four shapes, the ramp at both max_diff, the checkerboard, 1 beside 65535, the
    degenerate shapes: the plane, SIZE and `removed` by bytes; the argument is left as it is"""
    F = pkg.frontend
    q, sp, want, sizes, removed = K.made(name)
    keep = q.copy()
    got = F.filter_speckles(q, K.to_struct(F, sp))
    assert np.array_equal(q, keep)
    assert got[0].dtype == np.uint16 and got[1].dtype == np.uint32 and got[0].shape == got[1].shape == q.shape
    assert got[2] == removed
    assert got[1].tobytes() == sizes.tobytes()
    assert got[0].tobytes() == want.tobytes()


def test_filter_speckles_takes_a_row_stride_and_no_sizes(pkg):
    """rows further apart than their pixels: what lies between them stays; `sizes` may be NULL"""
    import ctypes as C
    F = pkg.frontend
    q, sp, want, sizes, removed = K.made("blobs-127x193")
    h, w = q.shape
    wide = np.full((h, w + 5), 777, np.uint16)
    wide[:, :w] = q
    n = C.c_int(-1)
    rc = F.lib().cvo_fe_filter_speckles(0, wide.ctypes.data_as(C.POINTER(C.c_uint16)), (w + 5) * 2, w, h,
                                        C.byref(K.to_struct(F, sp)), None, C.byref(n))
    assert rc == 0 and n.value == removed
    assert np.array_equal(wide[:, :w], want) and (wide[:, w:] == 777).all()


# ---- 2. through a context ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.STEREO_CASES))
def test_a_stereo_frame_behind_the_filter(pkg, name):
    """every plane by bytes, the cloud by bits; the second frame replays the captured graph"""
    F = pkg.frontend
    sp = K.STEREO_CASES[name]
    w, h, st, left, right = P.inputs(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo_speckle(K.to_struct(F, sp))                # (before stereo is set: a setting of its own)
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo_speckle() == F.Speckle(*sp)
    for k in range(2):
        _frame(gen, F, left, right, K.case_frame(name, sp), F.FEATURES_HSV if k else F.FEATURES_RGB)
    gen.close()


def test_settings_alternate_on_one_context(pkg):
    """off, (12, 16), (100, 32), off, (12, 16) on two alternating images: every frame by bytes.  A graph captured
    under other settings, or without the filter, and launched again would give that frame's planes."""
    F = pkg.frontend
    names = K.ALTERNATING_IMAGES
    inputs = [P.inputs(n) for n in names]
    w, h, st = inputs[0][:3]
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    k = 0
    for sp in K.ALTERNATING:
        gen.set_stereo_speckle(K.to_struct(F, sp))
        for _ in range(2):
            _, _, _, left, right = inputs[k % 2]
            Q = P.case_planes(names[k % 2], F.PATHS_4) if sp is None else K.case_frame(names[k % 2], sp)
            _frame(gen, F, left, right, Q, F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB, filtered=sp is not None)
            k += 1
    gen.close()


def test_a_frame_under_a_rig(pkg):
    """rig B of fe_stereo_rig_ref, a quarter of whose maps leave the raw images: the components are those of the plane
    after OUTSIDE (tests/test_fe_speckle_cpu.py: some pixel's SIZE depends on it)"""
    F = pkg.frontend
    w, h, st, rig, raw_l, raw_r, four = RG.case("B")
    Q = K.frame(four, K.RIG_SPECKLE)
    assert np.count_nonzero(Q["flags"] & RG.OUTSIDE) > 0 and np.count_nonzero(Q["flags"] & K.SPECKLE) > 0
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_speckle(K.to_struct(F, K.RIG_SPECKLE))
    gen.set_stereo_rig(RG.to_struct(F, rig))
    assert gen.stereo_speckle() == F.Speckle(*K.RIG_SPECKLE)     # (a rig set: the setting stays)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
        _stages_equal(gen, ((F.STAGE_RECT_BGR, Q["rect_l"]), (F.STAGE_RIGHT_BGR, Q["rect_r"]), (F.STAGE_STEREO_VALID, Q["valid"]),
                            (F.STAGE_SGM_SUM, Q["sum"]), (F.STAGE_DISPARITY, Q["disparity"]), (F.STAGE_STEREO, Q["flags"]),
                            (F.STAGE_RAW_DEPTH, Q["depth"]), (F.STAGE_RECT_DEPTH, Q["depth"]),
                            (F.STAGE_SPECKLE_SIZE, Q["sizes"])))
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(rig["depth_scale"], rig["fx"], rig["fy"], rig["cx"], rig["cy"]))
    assert _same_cloud(plain.create_pointcloud(Q["rect_l"], Q["depth"], 1, F.FEATURES_RGB), cloud) and len(cloud[0]) > 20
    gen.set_stereo_rig(None)
    assert gen.stereo_speckle() == F.Speckle(*K.RIG_SPECKLE)     # (... and cleared)
    plain.close(); gen.close()


def test_the_gate_reads_the_filtered_plane(pkg):
    F = pkg.frontend
    name, sp, mask_bits = K.GATE_CASE
    w, h, st, left, right = P.inputs(name)
    Q = K.case_frame(name, sp, mask_bits)
    gate = G.make_gate(13.0, 0.0, 0.2, 1, 0)
    mask = G.mask_scene(w, h, 72)
    dep, flags = G.gate(Q["depth"], gate, S.SCALE, mask)
    unfiltered = G.gate(P.case_planes(name, mask_bits)["depth"], gate, S.SCALE, mask)
    assert flags.any() and dep.any() and not np.array_equal(unfiltered[0], dep)
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_stereo(S.to_struct(F, st))
    gen.set_mask(mask)
    gen.set_stereo_speckle(K.to_struct(F, sp))
    for _ in range(2):
        xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        _stages_equal(gen, ((F.STAGE_SGM_SUM, Q["sum"]), (F.STAGE_UNGATED_DEPTH, Q["depth"]), (F.STAGE_RAW_DEPTH, Q["depth"]),
                            (F.STAGE_RECT_DEPTH, dep), (F.STAGE_GATE, flags), (F.STAGE_STEREO, Q["flags"]),
                            (F.STAGE_DISPARITY, Q["disparity"]), (F.STAGE_SPECKLE_SIZE, Q["sizes"])))
        ref = fo.create_pointcloud(left, dep, S.SEQ, F.FEATURES_RGB, num_want=gen.num_want)
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"])) and len(xyz) > 20
    gen.close()


def test_with_all_eight_paths(pkg):
    """another S, the same rule"""
    F = pkg.frontend
    name, sp, mask = K.PATHS8_CASE
    w, h, st, left, right = P.inputs(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_paths(mask)
    gen.set_stereo_speckle(K.to_struct(F, sp))
    for _ in range(2):
        _frame(gen, F, left, right, K.case_frame(name, sp, mask))
    gen.close()


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set the filter, ran a frame under it and cleared it: in bytes and in the cloud"""
    F = pkg.frontend
    name = "default-127x193-83"
    w, h, st, left, right = P.inputs(name)
    never, cleared = _generator(pkg, w, h), _generator(pkg, w, h)
    stages = (F.STAGE_SGM_SUM, F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RAW_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_MAP)
    clouds, planes = [], []
    for gen in (never, cleared):
        gen.set_stereo(S.to_struct(F, st))
        if gen is cleared:
            gen.set_stereo_speckle(F.Speckle(100, 16))
            _frame(gen, F, left, right, K.case_frame(name, (100, 16)))
            gen.set_stereo_speckle(None)
        assert gen.stereo_speckle() is None
        clouds.append(_frame(gen, F, left, right, S.case_planes(name), filtered=False))
        planes.append([gen.read_stage(s).tobytes() for s in stages])
    assert _same_cloud(clouds[0], clouds[1]) and planes[0] == planes[1]
    never.close(); cleared.close()


# ---- 3. refusals, and what the setting survives ----------------------------------------------------

def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    name, sp = "d128", K.STEREO_CASES["d128"]
    w, h, st, left, right = P.inputs(name)
    gen = _generator(pkg, w, h)
    for bad in K.bad_speckles():
        with pytest.raises(Err):
            gen.set_stereo_speckle(F.Speckle(*bad))           # without stereo set
        assert gen.stereo_speckle() is None
    assert b"set_stereo_speckle" in F.lib().cvo_fe_last_error(gen._h)
    gen.set_stereo(S.to_struct(F, st))
    with pytest.raises(Err):
        gen.read_stage(F.STAGE_SPECKLE_SIZE)                  # no filter: no such plane
    with pytest.raises(Err):
        F.filter_speckles(np.ones((4, 4), np.uint16), F.Speckle(0, 0))
    with pytest.raises(Err):
        F.filter_speckles(np.ones((4, 4), np.uint16), None)
    gen.set_stereo_speckle(F.Speckle(*sp))
    want = _frame(gen, F, left, right, K.case_frame(name, sp))
    for bad in K.bad_speckles():
        with pytest.raises(Err):
            gen.set_stereo_speckle(F.Speckle(*bad))
        assert gen.stereo_speckle() == F.Speckle(*sp)
    gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    for other in (F.Speckle(100, 32), F.Speckle(*sp), None):
        with pytest.raises(Err):
            gen.set_stereo_speckle(other)                     # while a frame is pending, even the settings in force
    assert _same_cloud(gen.collect(), want) and gen.stereo_speckle() == F.Speckle(*sp)
    assert _same_cloud(_frame(gen, F, left, right, K.case_frame(name, sp)), want)
    gen.set_stereo_speckle(None)
    with pytest.raises(Err):
        gen.read_stage(F.STAGE_SPECKLE_SIZE)
    gen.close()


def test_the_setting_survives_the_stereo_settings(pkg):
    """set with no stereo set; kept by set_stereo(settings), set_stereo(None) and new settings; not read by depth frames"""
    F = pkg.frontend
    name, sp = "noise", K.STEREO_CASES["noise"]
    w, h, st, left, right = P.inputs(name)
    dep0 = G.gate_scene(w, h, 73, "blocks")
    gen, other = _generator(pkg, w, h), _generator(pkg, w, h)
    before = other.create_pointcloud(left, dep0, 1, F.FEATURES_RGB)
    gen.set_stereo_speckle(F.Speckle(*sp))
    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB), before) and len(before[0]) > 20
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo_speckle() == F.Speckle(*sp)
    _frame(gen, F, left, right, K.case_frame(name, sp))
    gen.set_stereo(None)
    assert gen.stereo_speckle() == F.Speckle(*sp)
    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB), before)
    b = dict(st, p1=3, p2=90, max_disp=48)
    gen.set_stereo(S.to_struct(F, b))
    assert gen.stereo_speckle() == F.Speckle(*sp)
    Q = K.frame(S.match(left, right, b, S.FX, S.SCALE), sp)
    _frame(gen, F, left, right, Q)
    gen.set_stereo_speckle(F.Speckle(*sp))                    # the value it has: nothing happens
    _frame(gen, F, left, right, Q)
    gen.close(); other.close()


def test_the_filter_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 2048 x 1024 the three planes of the filter are 24 MiB.  Refused settings leave the free device
    memory where it was, to the 8 MiB such a reading resolves; the first settings are seen by the same reading, other
    settings take nothing more, and clearing the filter gives all of it back."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(2048, 1024)
    free0 = free()
    for bad in K.bad_speckles():
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_stereo_speckle(F.Speckle(*bad))
    gen.set_stereo_speckle(None)
    free1 = free()
    assert free0 - free1 < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_stereo_speckle(F.Speckle(100, 16))
    free2 = free()
    assert free1 - free2 >= 16 * MiB, "the first settings took only %d bytes" % (free1 - free2)
    gen.set_stereo_speckle(F.Speckle(12, 32))
    free3 = free()
    assert abs(free2 - free3) < 8 * MiB, "other settings moved the free memory by %d bytes" % (free2 - free3)
    gen.set_stereo_speckle(None)
    free4 = free()
    assert free4 - free3 >= 16 * MiB, "clearing the filter gave back only %d bytes" % (free4 - free3)
    gen.close()


# ---- 4. the layer above --------------------------------------------------------------------------

RUN_SPECKLE = (4000, 16)     # the box in front of the background goes (some 3700 pixels), and its points with it


def _run_pairs():
    """four pairs of one texture, the box coming nearer (an even width: the C++ demo's file)"""
    return [("%d.5" % (100 + k),) + S.pair(192, 128, 84, box=15.0 + k, back=6.0)[:2] for k in range(4)]


def test_run_frames_takes_the_setting(pkg):
    """run_frames(stereo_speckle=...) = the generator driven by hand: the same poses, and the last frame's plane the
    restatement's"""
    F = pkg.frontend
    w, h = 192, 128
    st = S.make_stereo()
    pairs = _run_pairs()
    plain = S.match(pairs[3][1], pairs[3][2], st, S.FX, S.SCALE)
    last = K.frame(plain, RUN_SPECKLE)
    assert not np.array_equal(last["depth"], plain["depth"]) and last["depth"].any()
    reg, buf = pkg.Cvo(), io.StringIO()
    gen = F.PcdGenerator(w, h, num_want=1500)
    assert F.run_frames(reg, pairs, S.SEQ, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen,
                        stereo=S.to_struct(F, st), stereo_speckle=F.Speckle(*RUN_SPECKLE)) == 4
    assert gen.stereo_speckle() == F.Speckle(*RUN_SPECKLE)
    assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == last["depth"].tobytes()
    assert gen.read_stage(F.STAGE_SPECKLE_SIZE).tobytes() == last["sizes"].tobytes()
    got = (buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations)
    reg.close(); gen.close()
    reg, buf = pkg.Cvo(), io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(w, h, num_want=1500)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_speckle(F.Speckle(*RUN_SPECKLE))
    gen.set_device_output(True)
    for name, left, right in pairs:
        gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        dp, df, n = gen.collect_device()
        reg.run_cvo_device(dp, df, n)
        writer.append(name, reg.accum_transform)
    assert got[0] == buf.getvalue() and np.array_equal(got[1], reg.accum_transform) and got[2] == reg.num_iterations > 0
    assert len(got[0].strip().split("\n")) == 4
    reg.close(); gen.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_setting(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_stereo_speckle (tests/cpp/cvo_stereo_speckle_demo.cpp): the clouds the C++ object
    registers and its pose lines equal the Python path's with the hand-over the object uses (device memory)"""
    F = pkg.frontend
    w, h = 192, 128
    pairs = _run_pairs()
    st = S.make_stereo()
    sp = F.Speckle(*RUN_SPECKLE)
    frames = [(name, left, np.ascontiguousarray(right).reshape(h, w * 3).view(np.uint16)) for name, left, right in pairs]
    got = _demo_lines(tmp_path, "cvo_stereo_speckle_demo", frames, w, h, bytes(S.to_struct(F, st)) + bytes(sp), [mode_name],
                      depth_sizes=True)
    acvo = mode_name == "acvo"
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    gen.set_device_output(True)
    gen.set_stereo(S.to_struct(F, st))
    want = ["refused bad settings"]
    sizes = []
    for k, (name, left, right) in enumerate(pairs):
        gen.set_stereo_speckle(None if k == 2 else sp)
        if k == 3:
            want.append("refused bad settings")
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
    plain = S.match(pairs[0][1], pairs[0][2], st, S.FX, S.SCALE)
    depth = K.frame(plain, RUN_SPECKLE)["depth"]
    unfiltered = S.match(pairs[2][1], pairs[2][2], st, S.FX, S.SCALE)["depth"]
    assert sizes[0] == len(fo.create_pointcloud(pairs[0][1], depth, S.SEQ, ftype)["positions"]) > 100
    assert sizes[0] < len(fo.create_pointcloud(pairs[0][1], plain["depth"], S.SEQ, ftype)["positions"])
    assert sizes[2] == len(fo.create_pointcloud(pairs[2][1], unfiltered, S.SEQ, ftype)["positions"]) > sizes[3]
