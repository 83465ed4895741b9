"""GPU: the path mask of the stereo matcher (cvo_fe_set_stereo_paths, include/cvo_frontend.h): the diagonal launches of
csrc/cvo_stereo.hip against the numpy restatement of step 4 under a mask (tests/fe_stereo_paths_ref.py) by bytes --
the cost sums, and every plane behind them -- and the cloud by bits against the CPU restatement of the front end
(oracle/frontend_oracle.c) on the left image and the reference's depth plane.  Each diagonal alone (under a one-bit
mask CVO_FE_STAGE_SGM_SUM is that direction's L_r), all eight on the shared and the edge cases and on `tall`, a subset,
the default set explicitly, masks alternating on one context (a stale captured graph would show), a frame under a rig,
a frame behind a gate; the refusals, what the mask survives, run_frames and the C++ objects above.  What the cases
reach, and which errors of a diagonal scan they would show, is asserted in tests/test_fe_stereo_paths_cpu.py."""
import io
import struct

import numpy as np
import pytest

import fe_gate_ref as G
import fe_stereo_paths_ref as P
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
from fe_gpu_common import _demo_lines, _digest, _pose_line_f32, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu


def _generator(pkg, w, h):
    # (an eighth of the pixels wanted, as for the edge cases of test_gpu_fe_stereo.py)
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _stages_equal(gen, F, Q, left):
    """every plane of a stereo frame against match()'s, by bytes (without a gate)"""
    for stage, want in ((F.STAGE_GRAY, Q["gray_l"]), (F.STAGE_RIGHT_GRAY, Q["gray_r"]), (F.STAGE_CENSUS_L, Q["census_l"]),
                        (F.STAGE_CENSUS_R, Q["census_r"]), (F.STAGE_SGM_SUM, Q["sum"]), (F.STAGE_DISPARITY, Q["disparity"]),
                        (F.STAGE_STEREO, Q["flags"]), (F.STAGE_RAW_DEPTH, Q["depth"]), (F.STAGE_UNGATED_DEPTH, Q["depth"]),
                        (F.STAGE_RECT_DEPTH, Q["depth"]), (F.STAGE_RECT_BGR, left)):
        got = gen.read_stage(stage)
        assert got.dtype == want.dtype and got.shape == want.shape, stage
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("stage %d differs at %d places, first at %s: %s against %s"
                                 % (stage, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _frame(gen, F, left, right, Q, ftype=None):
    """one frame: every plane by bytes, the cloud against the front-end oracle by bits"""
    ftype = F.FEATURES_RGB if ftype is None else ftype
    xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, ftype)
    _stages_equal(gen, F, Q, left)
    info = gen.info()
    ref = fo.create_pointcloud(left, Q["depth"], S.SEQ, ftype, num_want=gen.num_want)
    assert info["num_selected"] == ref["num_selected"] and info["num_points"] == len(ref["positions"]) == len(xyz)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud((xyz, feat), (ref["positions"], ref["features"]))
    assert len(xyz) > 0 or not Q["depth"].any()
    return xyz, feat


def _case_frame(pkg, name, mask, frames=1):
    F = pkg.frontend
    w, h, st, left, right = P.inputs(name)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo_paths() == F.PATHS_4
    gen.set_stereo_paths(mask)
    assert gen.stereo_paths() == mask
    for k in range(frames):                                   # (a second frame replays the captured graph)
        _frame(gen, F, left, right, P.case_planes(name, mask), F.FEATURES_HSV if k else F.FEATURES_RGB)
    gen.close()


# ---- 1. every plane by bytes and the cloud by bits ---------------------------------------------

@pytest.mark.parametrize("bit", [4, 5, 6, 7])
@pytest.mark.parametrize("name", ["default-96x64-82", "default-127x193-83"])
def test_each_diagonal_alone(pkg, name, bit):
    """w > h and h > w with odd sizes: the sums are that direction's L_r"""
    _case_frame(pkg, name, 1 << bit, frames=2)


@pytest.mark.parametrize("name", S.DEFAULTS + ["d128", "flat", "tall", "seam-128", "seam-72", "narrow", "wide", "p255",
                                               "p255-noise", "p1", "checker", "saturated", "tail"])
def test_all_eight_paths(pkg, name):
    """the shared cases, D 128 (two disparities per lane), a texture-free pair, `tall` (a wrapped line wraps five times),
    and the edge cases: the lane seam, D > w, the widest image, the penalties at both ends of their range, hostile
    images"""
    _case_frame(pkg, name, pkg.frontend.PATHS_8, frames=2 if name in ("tall", "d128") else 1)


def test_a_subset_of_five(pkg):
    """0x35: left to right, top to bottom, and the two diagonals of bits 4 and 5"""
    _case_frame(pkg, "default-127x193-82", 0x35)


def test_the_default_set_explicitly_is_a_context_that_never_made_the_call(pkg):
    F = pkg.frontend
    name = "default-127x193-81"
    w, h, st, left, right = P.inputs(name)
    never, explicit = _generator(pkg, w, h), _generator(pkg, w, h)
    explicit.set_stereo_paths(F.PATHS_4)                      # (before stereo is set: a setting of its own)
    stages = (F.STAGE_SGM_SUM, F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RAW_DEPTH, F.STAGE_MAP)
    clouds, planes = [], []
    for gen in (never, explicit):
        gen.set_stereo(S.to_struct(F, st))
        assert gen.stereo_paths() == F.PATHS_4
        clouds.append(_frame(gen, F, left, right, S.case_planes(name)))
        planes.append([gen.read_stage(s).tobytes() for s in stages])
    assert _same_cloud(clouds[0], clouds[1]) and planes[0] == planes[1]
    never.close(); explicit.close()


# ---- 2. graphs ---------------------------------------------------------------------------------

def test_masks_alternate_on_one_context(pkg):
    """0x0F, 0xFF, 0x10, 0x0F, 0xFF on alternating images of one size, twice round: every frame by bytes.  A graph
    captured under another mask and launched again would give that mask's sums."""
    F = pkg.frontend
    names = ("default-96x64-82", "default-96x64-83")
    inputs = [P.inputs(n) for n in names]
    w, h, st = inputs[0][:3]
    assert inputs[1][:3] == (w, h, st)
    gen = _generator(pkg, w, h)
    gen.set_stereo(S.to_struct(F, st))
    k = 0
    for _ in range(2):
        for mask in (0x0F, 0xFF, 0x10, 0x0F, 0xFF):
            gen.set_stereo_paths(mask)
            for _ in range(2):
                _, _, _, left, right = inputs[k % 2]
                _frame(gen, F, left, right, P.case_planes(names[k % 2], mask), F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB)
                k += 1
    gen.close()


# ---- 3. the rig and the gate read the masked plane ------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_a_frame_under_a_rig_with_all_eight_paths(pkg, name):
    """the rigs of fe_stereo_rig_ref (A stays inside its raw images; a quarter of B's maps leave them, so OUTSIDE is set):
    the rectified pair through eight paths, OUTSIDE ORed in behind; the cloud equals the one a plain context with the
    rig's pinhole gives for (rectified left image, the reference's depth plane)"""
    F = pkg.frontend
    w, h, st, rig, raw_l, raw_r, four = RG.case(name)
    Q = P.rig_frame(RG, rig, raw_l, raw_r, st, F.PATHS_8)
    assert (np.count_nonzero(Q["flags"] & RG.OUTSIDE) > 0) == (name == "B") and not np.array_equal(Q["sum"], four["sum"])
    assert np.array_equal(P.rig_frame(RG, rig, raw_l, raw_r, st, F.PATHS_4)["flags"], four["flags"])
    gen = _generator(pkg, w, h)
    gen.set_stereo_paths(F.PATHS_8)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_rig(RG.to_struct(F, rig))
    assert gen.stereo_paths() == F.PATHS_8                    # (a rig set: the mask stays)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(raw_l, raw_r, 1, F.FEATURES_RGB)
        for stage, want in ((F.STAGE_RECT_BGR, Q["rect_l"]), (F.STAGE_RIGHT_BGR, Q["rect_r"]), (F.STAGE_STEREO_VALID, Q["valid"]),
                            (F.STAGE_SGM_SUM, Q["sum"]), (F.STAGE_DISPARITY, Q["disparity"]), (F.STAGE_STEREO, Q["flags"]),
                            (F.STAGE_RAW_DEPTH, Q["depth"]), (F.STAGE_RECT_DEPTH, Q["depth"])):
            assert gen.read_stage(stage).tobytes() == want.tobytes(), stage
    plain = _generator(pkg, w, h)
    plain.set_camera(F.CameraModel(rig["depth_scale"], rig["fx"], rig["fy"], rig["cx"], rig["cy"]))
    assert _same_cloud(plain.create_pointcloud(Q["rect_l"], Q["depth"], 1, F.FEATURES_RGB), cloud) and len(cloud[0]) > 20
    gen.set_stereo_rig(None)
    assert gen.stereo_paths() == F.PATHS_8                    # (... and cleared)
    plain.close(); gen.close()


def test_the_gate_reads_the_eight_path_plane(pkg):
    F = pkg.frontend
    name = "default-127x193-82"
    w, h, st, left, right = P.inputs(name)
    Q = P.case_planes(name, F.PATHS_8)
    assert not np.array_equal(Q["depth"], S.case_planes(name)["depth"])
    gate = G.make_gate(13.0, 0.0, 0.2, 1, 0)
    mask = G.mask_scene(w, h, 72)
    dep, flags = G.gate(Q["depth"], gate, S.SCALE, mask)
    assert flags.any() and np.count_nonzero(dep) >= np.count_nonzero(Q["depth"]) // 4
    gen = _generator(pkg, w, h)
    gen.set_depth_gate(G.to_struct(F, gate))
    gen.set_stereo(S.to_struct(F, st))
    gen.set_mask(mask)
    gen.set_stereo_paths(F.PATHS_8)
    for _ in range(2):
        xyz, feat = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        assert gen.read_stage(F.STAGE_SGM_SUM).tobytes() == Q["sum"].tobytes()
        assert gen.read_stage(F.STAGE_UNGATED_DEPTH).tobytes() == Q["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == Q["depth"].tobytes()
        assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() == dep.tobytes()
        assert gen.read_stage(F.STAGE_GATE).tobytes() == flags.tobytes()
        assert gen.read_stage(F.STAGE_STEREO).tobytes() == Q["flags"].tobytes()
        assert gen.read_stage(F.STAGE_DISPARITY).tobytes() == Q["disparity"].tobytes()
        ref = fo.create_pointcloud(left, dep, S.SEQ, F.FEATURES_RGB, num_want=gen.num_want)
        assert _same_cloud((xyz, feat), (ref["positions"], ref["features"])) and len(xyz) > 20
    gen.close()


# ---- 4. refusals, and what the mask survives ---------------------------------------------------

def test_refusals_leave_the_context_usable_and_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    name = "default-96x64-82"
    w, h, st, left, right = P.inputs(name)
    gen = _generator(pkg, w, h)
    for bad in (0, 0x100, 0xFFFFFFFF):
        with pytest.raises(Err):
            gen.set_stereo_paths(bad)                         # without stereo set
        assert gen.stereo_paths() == F.PATHS_4
    assert b"set_stereo_paths" in F.lib().cvo_fe_last_error(gen._h)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_paths(0xF0)
    want = _frame(gen, F, left, right, P.case_planes(name, 0xF0))
    for bad in (0, 0x100, 0xFFFFFFFF):
        with pytest.raises(Err):
            gen.set_stereo_paths(bad)
        assert gen.stereo_paths() == 0xF0
    gen.submit_stereo(left, right, S.SEQ, F.FEATURES_RGB)
    for mask in (F.PATHS_8, 0xF0):
        with pytest.raises(Err):
            gen.set_stereo_paths(mask)                        # while a frame is pending, even the mask in force
    assert _same_cloud(gen.collect(), want) and gen.stereo_paths() == 0xF0
    assert _same_cloud(_frame(gen, F, left, right, P.case_planes(name, 0xF0)), want)
    gen.close()


def test_the_mask_survives_the_stereo_settings(pkg):
    """set with no stereo set; kept by set_stereo(settings), set_stereo(None) and new settings; not read by depth frames"""
    F = pkg.frontend
    name = "default-96x64-83"
    w, h, st, left, right = P.inputs(name)
    dep0 = G.gate_scene(w, h, 73, "blocks")
    gen, other = _generator(pkg, w, h), _generator(pkg, w, h)
    before = other.create_pointcloud(left, dep0, 1, F.FEATURES_RGB)
    gen.set_stereo_paths(F.PATHS_8)
    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB), before) and len(before[0]) > 20
    gen.set_stereo(S.to_struct(F, st))
    assert gen.stereo_paths() == F.PATHS_8
    _frame(gen, F, left, right, P.case_planes(name, F.PATHS_8))
    gen.set_stereo(None)
    assert gen.stereo_paths() == F.PATHS_8
    assert _same_cloud(gen.create_pointcloud(left, dep0, 1, F.FEATURES_RGB), before)
    b = dict(st, p1=3, p2=90, max_disp=48)
    gen.set_stereo(S.to_struct(F, b))
    assert gen.stereo_paths() == F.PATHS_8
    _frame(gen, F, left, right, P.match(left, right, b, S.FX, S.SCALE, F.PATHS_8))
    gen.set_stereo_paths(F.PATHS_8)                           # the value it has: nothing happens
    _frame(gen, F, left, right, P.match(left, right, b, S.FX, S.SCALE, F.PATHS_8))
    gen.close(); other.close()


# ---- 5. the layer above ------------------------------------------------------------------------

def _run_pairs():
    """four pairs of one texture, the box coming nearer (an even width: the C++ demo's file)"""
    return [("%d.5" % (100 + k),) + S.pair(192, 128, 84, box=15.0 + k, back=6.0)[:2] for k in range(4)]


def test_run_frames_takes_the_mask(pkg):
    """run_frames(stereo_paths=PATHS_8) = the generator driven by hand: the same poses, and the last frame's plane the
    restatement's"""
    F = pkg.frontend
    w, h = 192, 128
    st = S.make_stereo()
    pairs = _run_pairs()
    last = P.match(pairs[3][1], pairs[3][2], st, S.FX, S.SCALE, F.PATHS_8)
    assert not np.array_equal(last["depth"], S.match(pairs[3][1], pairs[3][2], st, S.FX, S.SCALE)["depth"])
    reg, buf = pkg.Cvo(), io.StringIO()
    gen = F.PcdGenerator(w, h, num_want=1500)
    assert F.run_frames(reg, pairs, S.SEQ, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen,
                        stereo=S.to_struct(F, st), stereo_paths=F.PATHS_8) == 4
    assert gen.stereo_paths() == F.PATHS_8 and gen.read_stage(F.STAGE_RAW_DEPTH).tobytes() == last["depth"].tobytes()
    got = (buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations)
    reg.close(); gen.close()
    reg, buf = pkg.Cvo(), io.StringIO()
    writer = pkg.trajectory.TrajectoryWriter(buf)
    gen = F.PcdGenerator(w, h, num_want=1500)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_paths(F.PATHS_8)
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
def test_cpp_objects_take_the_mask(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_stereo_paths (tests/cpp/cvo_stereo_paths_demo.cpp): the clouds the C++ object
    registers and its pose lines equal the Python path's with the hand-over the object uses (device memory)"""
    F = pkg.frontend
    w, h = 192, 128
    pairs = _run_pairs()
    st = S.make_stereo()
    mask = F.PATHS_8
    frames = [(name, left, np.ascontiguousarray(right).reshape(h, w * 3).view(np.uint16)) for name, left, right in pairs]
    got = _demo_lines(tmp_path, "cvo_stereo_paths_demo", frames, w, h, bytes(S.to_struct(F, st)) + struct.pack("<I", mask),
                      [mode_name], depth_sizes=True)
    acvo = mode_name == "acvo"
    ftype = F.FEATURES_HSV if acvo else F.FEATURES_RGB
    reg = (pkg.Acvo if acvo else pkg.Cvo)()
    gen = F.PcdGenerator(w, h)
    gen.set_device_output(True)
    gen.set_stereo(S.to_struct(F, st))
    want = ["refused a bad mask"]
    sizes = []
    for k, (name, left, right) in enumerate(pairs):
        gen.set_stereo_paths(F.PATHS_4 if k == 2 else mask)
        if k == 3:
            want.append("refused a bad mask")
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
    depth = P.match(pairs[0][1], pairs[0][2], st, S.FX, S.SCALE, mask)["depth"]
    assert sizes[0] == len(fo.create_pointcloud(pairs[0][1], depth, S.SEQ, ftype)["positions"]) > 100
