"""GPU: the selector's depth mode (cvo_fe_set_select_mode, the selection contract of include/cvo_frontend.h) held by
bytes to tests/selector_depth_ref.py -- the map, cvo_fe_info and the cloud of every frame of
tests/selector_depth_cases.py under every hole pattern and budget.  The restatement is fed AG0, AG1, AG2 and RECT_DEPTH
as read back from the device; the walk takes the frames up to 25 000 pixels, the closed form the larger ones.  One
context per size lives through all its cases with the modes alternating (every frame in CVO_FE_SELECT_IMAGE is held
to the restatement with a plane that is valid everywhere), so state left over from a frame would show.  Then: the mode
with full depth against the default, a context that set and cleared the mode against one that never called it, the
refusals, and the plane read -- behind a gate, a depth camera's warp, the stereo matcher and its speckle filter.
Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import fe_depth_ref as D
import fe_gate_ref as G
import fe_stereo_paths_ref as P
import fe_stereo_ref as S
import selector_depth_cases as dc
import selector_depth_ref as dr
import selector_ref_cases as sc
from fe_gpu_common import _demo_lines, _device_path_lines, _four_frames, _same_cloud

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
LARGE = ((640, 480), (1241, 376))
INVALID = -1   # CVO_HIP_ERR_INVALID (asserted against the library below)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pattern():
    return sc.libc_pattern(max(w * h for w, h in LARGE))


@pytest.fixture(scope="module")
def contexts(pkg):
    """One generator per image size, made when its first case runs and kept for the later ones"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[w, h] = pkg.frontend.PcdGenerator(w, h)
        return made[w, h]
    yield get
    for gen in made.values():
        gen.close()


def _set_num_want(pkg, gen, n):
    gen._chk(pkg.frontend.lib().cvo_fe_set_num_want(gen._h, int(n)), "set_num_want")
    gen.num_want = int(n)


def _cam(F, seq):
    c = F.camera(seq)
    return tuple(c[k] for k in ("scaling_factor", "fx", "fy", "cx", "cy"))


def _held(pkg, gen, cloud, budget, cam, pattern, select, memo, where, planes=None):
    """The frame the generator just made against the restatement: thresholds, map, info and cloud by bytes, and the
    consequences of the contract.  Returns (info, map, Z)."""
    F = pkg.frontend
    by_depth = gen.select_mode() == F.SELECT_DEPTH
    if planes is None:
        planes = [gen.read_stage(s) for s in (F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2)]
    Z = gen.read_stage(F.STAGE_RECT_DEPTH)
    valid = (Z != 0) if by_depth else np.ones(Z.shape, bool)
    t = dr.make_maps(*planes, budget, pattern, valid, select, memo=memo)
    info, mp = gen.info(), gen.read_stage(F.STAGE_MAP)
    print("%s: mode %d, selected %d, points %d, potential %d, reselected %d, canny %d"
          % (where, gen.select_mode(), info["num_selected"], info["num_points"], info["pot_used"], info["reselected"],
             info["canny_used"]))
    assert np.array_equal(_bits(gen.read_stage(F.STAGE_THS)), _bits(t["ths_smoothed"])), where
    got = {k: info[k] for k in ("num_selected", "pot_used", "reselected", "canny_used")}
    due = dr.topup_due(t["count"], budget)
    assert got == {"num_selected": t["count"], "pot_used": t["pot_used"], "reselected": t["reselected"],
                   "canny_used": int(due)}, where
    want, added = t["map"], 0
    if due:
        want, added, _ = dr.topup(want, gen.read_stage(F.STAGE_EDGES), valid)
    assert np.array_equal(_bits(mp), _bits(want)), where
    pos, feat = dr.cloud(want, Z, gen.read_stage(F.STAGE_RECT_BGR), gen.read_stage(F.STAGE_DX0),
                         gen.read_stage(F.STAGE_DY0), cam)
    assert info["num_points"] == len(pos) == len(cloud[0]), where
    assert _same_cloud(cloud, (pos, feat)), where
    if by_depth:   # the consequences the contract states
        assert not (mp != 0)[Z == 0].any(), where
        assert info["num_points"] == info["num_selected"] + added, where
        assert added == 0 or due
    return info, mp, Z


def _all_patterns(pkg, gen, frame_name, bgr, budgets, pattern, select, patterns=dc.PATTERNS, seed=0):
    """every hole pattern x budget on one context: a frame in the depth mode, then one in the default mode"""
    F = pkg.frontend
    h, w = bgr.shape[:2]
    cam = _cam(F, 1)
    # the planes and thresholds the hole patterns are made from: a default frame with depth everywhere
    gen.set_select_mode(F.SELECT_IMAGE)
    _set_num_want(pkg, gen, budgets[0])
    gen.create_pointcloud(bgr, dc.depth_of(np.ones((h, w), bool)), 1, F.FEATURES_RGB)
    planes = [gen.read_stage(s) for s in (F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2)]
    sm = gen.read_stage(F.STAGE_THS)
    memo_image = {}
    seen = set()
    for p in patterns:
        dep = dc.depth_of(dc.hole_pattern(p, *planes, sm, seed=seed))
        memo = {}
        for b in budgets:
            _set_num_want(pkg, gen, b)
            where = "%s, %s, num_want %d" % (frame_name, p, b)
            gen.set_select_mode(F.SELECT_DEPTH)
            cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
            info, _, _ = _held(pkg, gen, cloud, b, cam, pattern, select, memo, where, planes)
            seen.add((info["reselected"], info["canny_used"]))
            if p == "all":
                assert (info["num_selected"], info["num_points"], info["pot_used"], info["reselected"]) == (0, 0, 1, 1)
            gen.set_select_mode(F.SELECT_IMAGE)
            cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
            _held(pkg, gen, cloud, b, cam, pattern, select, memo_image, where, planes)
    assert {(1, 0), (1, 1)} <= seen, seen   # (reselected, canny_used); a top-up without a re-selection cannot be


@pytest.mark.parametrize("case", dc.FRAMES, ids=lambda c: c.name)
def test_depth_mode_equals_the_restatement(pkg, case, contexts, pattern):
    """the frames up to 25 000 pixels, through the reference's walk"""
    assert sc.runs_in_python(case)
    bgr, _ = sc.frame(pkg, case)
    _all_patterns(pkg, contexts(case.w, case.h), case.name, bgr, dc.budgets(case.w, case.h), pattern, dr.select_walk,
                  seed=case.seed)


@pytest.mark.parametrize("size", LARGE, ids=["%dx%d" % s for s in LARGE])
def test_large_frames_equal_the_closed_form(pkg, size, contexts, pattern):
    """a VGA frame and a frame of KITTI's size, through the closed form only"""
    w, h = size
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=16, texture=1.0)
    _all_patterns(pkg, contexts(w, h), "tex1_s16_%dx%d" % size, bgr, dc.budgets(w, h), pattern, dr.select_closed, seed=16)


def _stages(gen, F):
    return [gen.read_stage(s) for s in (F.STAGE_MAP, F.STAGE_THS, F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2,
                                        F.STAGE_RECT_DEPTH, F.STAGE_RECT_BGR, F.STAGE_DX0, F.STAGE_DY0, F.STAGE_HSV)]


@pytest.mark.parametrize("kind", ["tex1_s2_96x64", "tex1_s9_127x193", "lowtex_s6_128x192"])
def test_full_depth_is_the_default_mode(pkg, kind):
    """with Z != 0 everywhere the frame is, plane by plane and point by point, the frame of CVO_FE_SELECT_IMAGE -- also
    through the top-up (lowtex) and both feature types"""
    F = pkg.frontend
    case = next(c for c in sc.CASES if c.name == kind)
    bgr, _ = sc.frame(pkg, case)
    dep = dc.depth_of(np.ones((case.h, case.w), bool))
    gen = F.PcdGenerator(case.w, case.h)
    canny = set()
    for b in (50, case.w * case.h // 8, 3000):
        _set_num_want(pkg, gen, b)
        for ftype in (F.FEATURES_RGB, F.FEATURES_HSV):
            out = {}
            for mode in (F.SELECT_IMAGE, F.SELECT_DEPTH):
                gen.set_select_mode(mode)
                assert gen.select_mode() == mode
                out[mode] = (gen.create_pointcloud(bgr, dep, 1, ftype), gen.info(), _stages(gen, F))
            a, b_ = out[F.SELECT_IMAGE], out[F.SELECT_DEPTH]
            assert _same_cloud(a[0], b_[0]) and a[1] == b_[1] and len(a[0][0]) > 0
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b_[2]))
            assert a[1]["num_points"] == np.count_nonzero(a[2][0])
            canny.add(a[1]["canny_used"])
    assert 1 in canny or not kind.startswith("lowtex")
    gen.close()


def test_set_and_cleared_is_never_called(pkg):
    """a context that set the mode, ran a frame and cleared it gives what one that never made the call gives, frames
    with holes included, through create_pointcloud and submit / collect"""
    F = pkg.frontend
    case = next(c for c in sc.CASES if c.name == "tex1_s2_96x64")
    bgr, _ = sc.frame(pkg, case)
    dep = dc.depth_of(dc._blobs(case.w, case.h, 5, 0.3) == 0)
    never, used = F.PcdGenerator(case.w, case.h, num_want=300), F.PcdGenerator(case.w, case.h, num_want=300)
    assert never.select_mode() == used.select_mode() == F.SELECT_IMAGE
    want = never.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    want_info, want_stages = never.info(), _stages(never, F)
    assert _same_cloud(used.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    used.set_select_mode(F.SELECT_DEPTH)
    other = used.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    assert len(other[0]) > len(want[0]) and used.info()["num_selected"] == len(other[0])
    used.set_select_mode(F.SELECT_DEPTH)          # the value it has: nothing happens
    assert _same_cloud(used.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), other)
    used.set_select_mode(F.SELECT_IMAGE)
    for _ in range(2):                            # (the second frame replays the captured graph)
        assert _same_cloud(used.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
        assert used.info() == want_info
        assert all(x.tobytes() == y.tobytes() for x, y in zip(_stages(used, F), want_stages))
    used.submit(bgr, dep, 1, F.FEATURES_RGB)
    assert _same_cloud(used.collect(), want)
    never.close()
    used.close()


def test_refusals_and_what_the_setting_survives(pkg):
    F = pkg.frontend
    L = F.lib()
    case = next(c for c in sc.CASES if c.name == "tex1_s2_96x64")
    bgr, _ = sc.frame(pkg, case)
    dep = dc.depth_of(dc._blobs(case.w, case.h, 5, 0.3) == 0)
    gen = F.PcdGenerator(case.w, case.h, num_want=300)
    assert F.check_select_mode(F.SELECT_IMAGE) and F.check_select_mode(F.SELECT_DEPTH)
    assert (F.SELECT_IMAGE, F.SELECT_DEPTH) == (0, 1)
    mode = C.c_int(-5)
    # a null context, a null result
    assert L.cvo_fe_set_select_mode(None, F.SELECT_DEPTH) == INVALID
    assert L.cvo_fe_get_select_mode(None, C.byref(mode)) == INVALID and mode.value == -5
    assert L.cvo_fe_get_select_mode(gen._h, None) == INVALID
    assert L.cvo_fe_check_stereo_paths(0) == INVALID            # (the code every refusal of a setting gives)
    gen.set_select_mode(F.SELECT_DEPTH)
    want = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    # a bad mode: refused, the context keeps what it had
    for bad in (-1, 2, 3, 255, 2 ** 31 - 1, -2 ** 31):
        assert not F.check_select_mode(bad)
        assert L.cvo_fe_set_select_mode(gen._h, bad) == INVALID
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_select_mode(bad)
        assert gen.select_mode() == F.SELECT_DEPTH
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_select_mode(2 ** 40)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    # a frame submitted and not collected
    gen.submit(bgr, dep, 1, F.FEATURES_RGB)
    assert L.cvo_fe_set_select_mode(gen._h, F.SELECT_IMAGE) == INVALID
    with pytest.raises(pkg.capi.CvoHipError):
        gen.set_select_mode(F.SELECT_IMAGE)
    assert gen.select_mode() == F.SELECT_DEPTH
    assert _same_cloud(gen.collect(), want)
    # it survives every other setter
    gen.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 1))
    gen.set_mask(np.zeros((case.h, case.w), np.uint8))
    gen.set_camera(F.CameraModel(5000.0, 80.0, 80.0, 47.5, 31.5, ZERO))
    gen.set_stereo_paths(F.PATHS_8)
    gen.set_stereo_speckle(F.Speckle(12, 16))
    gen.set_stereo(S.to_struct(F, S.make_stereo()))
    gen.set_device_output(True)
    _set_num_want(pkg, gen, 200)
    assert gen.select_mode() == F.SELECT_DEPTH
    for undo in (gen.set_stereo, gen.set_stereo_speckle, gen.set_camera, gen.set_mask, gen.set_depth_gate):
        undo(None)
    gen.set_device_output(False)
    _set_num_want(pkg, gen, 300)
    assert gen.select_mode() == F.SELECT_DEPTH
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    gen.close()


# ---- the plane read is the final one -----------------------------------------------------------------------------

def test_behind_a_gate_no_selected_pixel_is_out_of_range(pkg, pattern):
    """a range cut of 0.8 to 4 m on a scene with nearer and farther pixels: the default mode selects some of them (and
    they give no point), the depth mode none"""
    F = pkg.frontend
    w, h = 96, 64
    bgr, U = G.frame(w, h, 72), G.gate_scene(w, h, 72, "blocks")
    gen = F.PcdGenerator(w, h, num_want=w * h // 8)
    gen.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 1))
    cam = _cam(F, 1)
    res = {}
    for mode in (F.SELECT_IMAGE, F.SELECT_DEPTH, F.SELECT_IMAGE, F.SELECT_DEPTH):
        gen.set_select_mode(mode)
        cloud = gen.create_pointcloud(bgr, U, 1, F.FEATURES_RGB)
        res[mode] = _held(pkg, gen, cloud, gen.num_want, cam, pattern, dr.select_walk, {}, "gate, mode %d" % mode)
    ungated = gen.read_stage(F.STAGE_UNGATED_DEPTH)
    metres = ungated.astype(np.float32) / np.float32(G.SCALE)
    out_of_range = (ungated == 0) | (metres < np.float32(0.8)) | (metres > np.float32(4.0))
    assert out_of_range.any() and np.array_equal(ungated, U)
    info_i, map_i, _ = res[F.SELECT_IMAGE]
    info_d, map_d, Z = res[F.SELECT_DEPTH]
    assert (map_i != 0)[out_of_range].any() and info_i["num_points"] < info_i["num_selected"]
    assert not (map_d != 0)[out_of_range].any() and not (map_d != 0)[gen.read_stage(F.STAGE_GATE) != 0].any()
    assert info_d["num_points"] == info_d["num_selected"] > info_i["num_points"]
    gen.close()


@pytest.mark.parametrize("name", ["K", "U"])
def test_behind_a_depth_cameras_warp(pkg, pattern, name):
    """the forward warp fills no holes: the plane the selector reads is the registered one"""
    F = pkg.frontend
    w, h, cam, rig = D.RIGS[name]
    gen = F.PcdGenerator(w, h, num_want=w * h // 8)
    gen.set_camera(F.CameraModel(*(cam + (ZERO,))))
    gen.set_depth_camera(D.to_struct(F, rig))
    bgr, _ = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    dep = D.scene(pkg.data, rig, seed=73, holes=0.2)
    res = {}
    for mode in (F.SELECT_DEPTH, F.SELECT_IMAGE):
        gen.set_select_mode(mode)
        cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        res[mode] = _held(pkg, gen, cloud, gen.num_want, cam, pattern, dr.select_walk, {}, "rig %s, mode %d" % (name, mode))
    Z = res[F.SELECT_DEPTH][2]
    assert Z.shape != dep.shape or not np.array_equal(Z, dep)
    assert 0 < np.count_nonzero(Z == 0) < w * h
    assert res[F.SELECT_DEPTH][0]["num_points"] > res[F.SELECT_IMAGE][0]["num_points"]
    gen.close()


@pytest.mark.parametrize("speckle", [None, (12, 16), (100, 32)], ids=["plain", "speckle12", "speckle100"])
@pytest.mark.parametrize("name", ["default-96x64-82", "noise"])
def test_behind_the_matcher_and_the_speckle_filter(pkg, pattern, name, speckle):
    """a small stereo pair: the selected pixels all carry a disparity, with and without the speckle filter"""
    F = pkg.frontend
    w, h, st, left, right = P.inputs(name)
    gen = F.PcdGenerator(w, h, num_want=w * h // 8)
    gen.set_select_mode(F.SELECT_DEPTH)           # (before stereo is set: a setting of its own)
    gen.set_stereo(S.to_struct(F, st))
    gen.set_stereo_speckle(None if speckle is None else F.Speckle(*speckle))
    cam = _cam(F, S.SEQ)
    for mode in (F.SELECT_DEPTH, F.SELECT_IMAGE, F.SELECT_DEPTH):
        if mode != gen.select_mode():
            gen.set_select_mode(mode)
        cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        info, mp, Z = _held(pkg, gen, cloud, gen.num_want, cam, pattern, dr.select_walk, {},
                            "%s, %s, mode %d" % (name, speckle, mode))
        disparity, flags = gen.read_stage(F.STAGE_DISPARITY), gen.read_stage(F.STAGE_STEREO)
        assert np.array_equal(Z != 0, disparity != 0) and np.array_equal(Z != 0, flags == 0) and (Z == 0).any()
        if mode == F.SELECT_DEPTH:
            assert (disparity[mp != 0] != 0).all() and (flags[mp != 0] == 0).all()
        if speckle is not None:
            assert not ((flags & F.STEREO_SPECKLE) != 0)[Z != 0].any()
    gen.close()


# ---- the layers above ------------------------------------------------------------------------------------------------

def _holed_frames(pkg):
    """four VGA frames of a scene in motion whose depth images have blob holes over about 30 %"""
    return _four_frames(pkg, 75, lambda k, dep: np.where(dc._blobs(640, 480, 40 + k, 0.3), 0, dep).astype(np.uint16))


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_mode(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_select_mode (tests/cpp/cvo_select_mode_demo.cpp): the clouds the C++ object
    registers and its pose lines equal the Python path's; the frames in the depth mode hold more points"""
    F = pkg.frontend
    frames = _holed_frames(pkg)
    got = _demo_lines(tmp_path, "cvo_select_mode_demo", frames, 640, 480, b"", [mode_name])
    gen = F.PcdGenerator(640, 480)

    def prepare(k):
        gen.set_select_mode(F.SELECT_IMAGE if k == 2 else F.SELECT_DEPTH)
        return ["refused a bad mode"] if k == 3 else []

    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, frames, prepare)
    assert got == ["refused a bad mode"] + want
    assert sizes[2] < min(sizes[0], sizes[1], sizes[3]) and min(sizes) > 1000
    gen.close()


def test_run_frames_takes_the_mode(pkg):
    """run_frames(select_mode=...) sets the generator's mode and leaves it alone when None"""
    F = pkg.frontend
    frames = _holed_frames(pkg)[:3]
    gen = F.PcdGenerator(640, 480)
    reg = pkg.Cvo()
    assert F.run_frames(reg, frames, 1, generator=gen, select_mode=F.SELECT_DEPTH) == 3
    assert gen.select_mode() == F.SELECT_DEPTH and gen.info()["num_points"] == gen.info()["num_selected"]
    reg.close()
    reg = pkg.Cvo()
    assert F.run_frames(reg, frames, 1, generator=gen) == 3
    assert gen.select_mode() == F.SELECT_DEPTH
    assert F.run_frames(reg, frames[:1], 1, generator=gen, select_mode=F.SELECT_IMAGE) == 1
    assert gen.select_mode() == F.SELECT_IMAGE and gen.info()["num_points"] < gen.info()["num_selected"]
    reg.close()
    gen.close()
