"""GPU: input binning of the front end (cvo_fe_set_input_binning, cvo_fe_bin_image, cvo_fe_bin_depth; the binning contract
of include/cvo_frontend.h): k_fe_bin of csrc/cvo_bin.hip against the restatement tests/fe_binning_ref.py by bytes -- every
factor at every size and input of fe_binning_ref.cases() -- and frames of every kind under every factor: the input-size
planes by bytes against what was handed over, the binned planes by bytes against the restatement, and every later stage,
the info and the cloud, by bytes and bits, against a second context of the working size without binning that was fed
the restatement's images under the same camera, and against the CPU restatement of the front end
(oracle/frontend_oracle.c) on them.  Settings alternating on one context, with and without captured graphs (a stale
graph would show), a context that never made the call, the refusals with their sentences, the memory, the staging
buffers, run_frames and the C++ objects above.  Which errors of a four-pixels-per-thread bin these inputs would show is
asserted in tests/test_fe_binning_cpu.py."""
import ctypes as C
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import fe_binning_ref as B
import fe_depth_ref as D
import fe_depthfmt_ref as KD
import fe_gate_ref as G
import fe_lidar_ref as KL
import fe_rectify_ref as R
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
import fe_unpack_ref as K
from fe_gpu_common import ROOT, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
SIZES = ((64, 64), (96, 64))
IDS = ["%dx%d" % s for s in SIZES]
RULE = b"factor 2, 3 or 4, depth_min in [1, factor^2], pad_ 0"
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


def _frame(pkg, w, h, f, dmin, holes=0.02):
    """(input colour, input depth, binned colour, binned depth) of the synthetic frame at the input size"""
    def make():
        bgr, dep = pkg.data.synthetic_rgbd_frame(width=f * w, height=f * h, seed=72, texture=1.0, holes=holes)
        return bgr, dep, B.bin_colour(bgr, f), B.bin_depth(dep, f, dmin)
    return _ref(("frame", w, h, f, dmin, holes), make)


def _upsample(img, f):
    """an input-size image whose bin is (but for the clipping) `img`: each pixel repeated f x f, and a pattern over the
    block's phases on top that sums to nothing, so that no block is flat"""
    n = f * f
    pattern = np.array([4 * (p % 3 - 1) for p in range(n)])
    pattern[n - 1] -= pattern.sum()
    up = np.repeat(np.repeat(img.astype(np.int32), f, axis=0), f, axis=1)
    yy, xx = np.mgrid[0:up.shape[0], 0:up.shape[1]]
    return np.clip(up + pattern[(yy % f) * f + xx % f][..., None], 0, 255).astype(np.uint8)


def _packed(w, h, f, fmt):
    """(the packed input image, the restatement's unpacked image of the input size, its bin)"""
    def make():
        packed = K.pack(G.frame(f * w, f * h, 72), fmt)
        full = K.unpack(packed, fmt, f * w, f * h)
        return packed, full, B.bin_colour(full, f)
    return _ref(("packed", w, h, f, fmt), make)


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _later_stages(F):
    return (F.STAGE_RECT_BGR, F.STAGE_GRAY, F.STAGE_RECT_DEPTH, F.STAGE_RAW_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_HSV,
            F.STAGE_MAP, F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2, F.STAGE_THS, F.STAGE_DX0, F.STAGE_DY0)


def _same_frame(gen, plain, F, cloud, plain_cloud, what, extra=()):
    """every later stage by bytes, the info, and the cloud by bits: the frame of the context of the working size"""
    for stage in _later_stages(F) + tuple(extra):
        _differ(gen.read_stage(stage), plain.read_stage(stage), "stage %d of %s" % (stage, what))
    assert gen.info() == plain.info(), what
    print("%s: %d points" % (what, len(cloud[0])))
    assert _same_cloud(cloud, plain_cloud) and len(cloud[0]) >= 20, what


def _oracle_cloud(gen, F, cloud, bgr, seq, ftype):
    """the cloud against the front-end oracle on the binned colour image and the plane the cloud is made from"""
    ref = fo.create_pointcloud(bgr, gen.read_stage(F.STAGE_RECT_DEPTH), seq, ftype, num_want=gen.num_want)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud(cloud, (ref["positions"], ref["features"]))


def _no_plane(pkg, gen, stage):
    with pytest.raises(pkg.capi.CvoHipError):
        gen.read_stage(stage)
    assert b"read_stage" in pkg.frontend.lib().cvo_fe_last_error(gen._h)


# ---- 1. the stand-alone entries ----------------------------------------------------------------------

@pytest.mark.parametrize("f", B.FACTORS)
def test_bin_image_by_bytes(pkg, f):
    """every size and input of the factor against the restatement; the source is left as it is (bin_image checks it)"""
    F = pkg.frontend
    for case in B.cases():
        if case[0] != "colour" or case[1] != f:
            continue
        for k, src in enumerate(B.case_inputs(case)):
            _differ(F.bin_image(src, f), B.bin_colour(src, f), "colour %r input %d" % (case, k))


@pytest.mark.parametrize("f", B.FACTORS)
def test_bin_depth_by_bytes(pkg, f):
    F = pkg.frontend
    for case in B.cases():
        if case[0] != "depth" or case[1] != f:
            continue
        for src in B.case_inputs(case):
            want = B.bin_depth(src, f, case[5])
            got, valid = F.bin_depth(src, F.Binning(f, case[5]))
            _differ(got, want, "depth %r" % (case,))
            assert valid == int((want != 0).sum()), case


@pytest.mark.parametrize("f", B.FACTORS)
def test_the_entries_take_a_row_stride(pkg, f):
    """rows further apart than their bytes, row + 5: what lies between them is not read into the image, and stays
    (bin_image / bin_depth check that).  (The kernel's own rows are dense; those that start off a dword come with the odd
    widths of the cases above, 13 f pixels for one.)"""
    F = pkg.frontend
    for w, h in ((13, 7), (66, 18), (130, 34)):
        src = B.colour_input(f, w, h, "random")
        _differ(F.bin_image(src, f, stride=f * w * 3 + 5), B.bin_colour(src, f), "colour %dx%d" % (w, h))
        dep = B.depth_input(f, w, h, "half", 2)
        got, valid = F.bin_depth(dep, F.Binning(f, 2), stride=f * w + 5)
        _differ(got, B.bin_depth(dep, f, 2), "depth %dx%d" % (w, h))
        assert valid == int((got != 0).sum())


# ---- 2. frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_depth_frame(pkg, size, f):
    """FULL_* by bytes against the input, INPUT_BGR and RAW_DEPTH against the restatement, everything behind them as the
    context of the working size gives it on the restatement's images, and as the oracle does; depth_min 1 and f^2, each
    twice: the second frame replays the captured graph"""
    F = pkg.frontend
    w, h = size
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    assert gen.input_binning() is None
    for dmin in (1, f * f):
        bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, dmin)
        gen.set_input_binning(F.Binning(f, dmin))
        assert gen.input_binning() == F.Binning(f, dmin)
        for k in range(2):
            ftype = F.FEATURES_HSV if k else F.FEATURES_RGB
            cloud = gen.create_pointcloud(bgr, dep, 1, ftype)
            _differ(gen.read_stage(F.STAGE_FULL_BGR), bgr, "FULL_BGR")
            _differ(gen.read_stage(F.STAGE_FULL_DEPTH), dep, "FULL_DEPTH")
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
            _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH")
            _differ(gen.read_stage(F.STAGE_RECT_BGR), bbgr, "RECT_BGR")
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, bdep, 1, ftype), "depth frame f %d min %d" % (f, dmin))
            _oracle_cloud(gen, F, cloud, bbgr, 1, ftype)
            _no_plane(pkg, gen, F.STAGE_FULL_RIGHT_BGR)
            _no_plane(pkg, gen, F.STAGE_INPUT_RIGHT_BGR)
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_the_planes_of_a_frame_full_of_holes(pkg, size, f):
    """30 % holes and depth_min f^2: few blocks keep a depth, so the planes are compared and no cloud is asked for"""
    F = pkg.frontend
    w, h = size
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, f * f, holes=0.3)
    gen = _generator(pkg, w, h)
    gen.set_input_binning(F.Binning(f, f * f))
    gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
    _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH")
    _differ(gen.read_stage(F.STAGE_RECT_DEPTH), bdep, "RECT_DEPTH")
    _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
    assert 0 < (bdep != 0).sum() < bdep.size // 2
    gen.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_stereo_frame(pkg, size, f):
    """both images of the pair are binned by one launch, each from its own input"""
    F = pkg.frontend
    w, h = size
    st = S.make_stereo(max_disp=32)
    left, right, _ = _ref(("pair", w, h), lambda: S.pair(w, h, 82))
    fl, fr = _upsample(left, f), _upsample(right, f)
    bl, br = B.bin_colour(fl, f), B.bin_colour(fr, f)
    assert not np.array_equal(bl, br)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    plain.set_stereo(S.to_struct(F, st))
    if f == 3:                                                 # (binning first, stereo behind it ...)
        gen.set_input_binning(F.Binning(f, 1))
        gen.set_stereo(S.to_struct(F, st))
    else:                                                      # (... and the other way round)
        gen.set_stereo(S.to_struct(F, st))
        gen.set_input_binning(F.Binning(f, 1))
    assert gen.stereo() == S.to_struct(F, st) and gen.input_binning() == F.Binning(f, 1)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(fl, fr, S.SEQ, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_FULL_BGR), fl, "FULL_BGR")
        _differ(gen.read_stage(F.STAGE_FULL_RIGHT_BGR), fr, "FULL_RIGHT_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bl, "INPUT_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_RIGHT_BGR), br, "INPUT_RIGHT_BGR")
        _differ(gen.read_stage(F.STAGE_RIGHT_BGR), br, "RIGHT_BGR")
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(bl, br, S.SEQ, F.FEATURES_RGB), "stereo f %d" % f,
                    extra=(F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RIGHT_GRAY))
        _oracle_cloud(gen, F, cloud, bl, S.SEQ, F.FEATURES_RGB)
        _no_plane(pkg, gen, F.STAGE_FULL_DEPTH)
    gen.set_stereo(None)                                       # (the setting survives, and depth frames read it)
    plain.set_stereo(None)
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, 1)
    assert gen.input_binning() == F.Binning(f, 1)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB))
    _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH")
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
def test_a_raw_pair_under_the_binned_rig(pkg, f):
    """rig A, 96 x 64: the raw pair arrives at the input size under the input images' rig; bin_stereo_rig's rig is set, on
    both contexts, and the rectification follows the bin"""
    F = pkg.frontend
    w, h, disp, calib = RG.CALIBS["A"]
    rig = RG.rectify(calib, w, h, RG.DEPTH_SCALE)
    c = 0.5 * (f - 1)
    grow = lambda lens: (lens[0] * f, lens[1] * f, lens[2] * f + c, lens[3] * f + c, lens[4])
    rig_in = dict(rig, left=grow(rig["left"]), right=grow(rig["right"]), fx=rig["fx"] * f, fy=rig["fy"] * f,
                  cx=rig["cx"] * f + c, cy=rig["cy"] * f + c)
    working = F.bin_stereo_rig(RG.to_struct(F, rig_in), f)
    assert abs(working.cx - rig["cx"]) < 1e-3 and abs(working.left.fx - rig["left"][0]) < 1e-3
    st = S.make_stereo(max_disp=disp)
    raw_l, raw_r = _ref(("rig A",), lambda: RG.render(rig, w, h))
    fl, fr = _upsample(raw_l, f), _upsample(raw_r, f)
    bl, br = B.bin_colour(fl, f), B.bin_colour(fr, f)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_stereo(S.to_struct(F, st))
    gen.set_input_binning(F.Binning(f, 1))
    for g in (gen, plain):
        g.set_stereo_rig(working)
    assert gen.input_binning() == F.Binning(f, 1) and gen.stereo_rig() == working
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(fl, fr, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_FULL_RIGHT_BGR), fr, "FULL_RIGHT_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bl, "INPUT_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_RIGHT_BGR), br, "INPUT_RIGHT_BGR")
        assert not np.array_equal(gen.read_stage(F.STAGE_RECT_BGR), bl)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(bl, br, 1, F.FEATURES_RGB), "rig f %d" % f,
                    extra=(F.STAGE_RIGHT_BGR, F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_STEREO_VALID))
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_lidar_frame(pkg, size, f):
    """only the colour image is binned; the scan is projected into the camera of the working image"""
    F = pkg.frontend
    w, h = size
    seq = 4
    cam = tuple(F.camera(seq).values())
    s = KL.setting((1, 7, 1, 0.25), **KL.MOUNT)
    points = _ref(("scan", w, h), lambda: (KL.scan_clutter(w, h, 4097, 52, s, cam),))[0]
    bgr, _, bbgr, _ = _frame(pkg, w, h, f, 1)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_input_binning(F.Binning(f, 1))
    gen.set_lidar(KL.to_struct(F, s)); plain.set_lidar(KL.to_struct(F, s))
    assert gen.input_binning() == F.Binning(f, 1)
    for _ in range(2):
        cloud = gen.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_FULL_BGR), bgr, "FULL_BGR")
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_lidar(bbgr, points, seq, F.FEATURES_RGB), "lidar f %d" % f,
                    extra=(F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR))
        _oracle_cloud(gen, F, cloud, bbgr, seq, F.FEATURES_RGB)
        _no_plane(pkg, gen, F.STAGE_FULL_DEPTH)
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_with_a_depth_camera(pkg, size, f):
    """the depth image keeps the rig's size and its own staging; only the colour image is binned, and FULL_DEPTH is
    refused; the rig before binning at f = 2, behind it otherwise"""
    F = pkg.frontend
    w, h = size
    cam = (5000.0, 77.6, 77.5, (w - 1) / 2.0, (h - 1) / 2.0)
    rig = D.make_rig(80, 56, (1000.0, 70.0, 70.2, 39.1, 27.4), (-0.12, 0.03, 0.001, -0.002, 0.0), D.K_R, D.K_T)
    raw = D.scene(pkg.data, rig)
    bgr, _, bbgr, _ = _frame(pkg, w, h, f, 1)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_camera(F.CameraModel(*(cam + (ZERO,))))
    if f == 2:
        gen.set_depth_camera(D.to_struct(F, rig))
        gen.set_input_binning(F.Binning(f, 1))
    else:
        gen.set_input_binning(F.Binning(f, 1))
        gen.set_depth_camera(D.to_struct(F, rig))
    plain.set_depth_camera(D.to_struct(F, rig))
    assert gen.depth_camera() == D.to_struct(F, rig) and gen.input_binning() == F.Binning(f, 1)
    assert gen.host_buffers()[1].shape == (56, 80) and gen.host_buffers()[0].shape == (f * h, f * w, 3)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
        assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), raw)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, raw, 1, F.FEATURES_RGB), "depth camera f %d" % f)
        _no_plane(pkg, gen, F.STAGE_FULL_DEPTH)
    gen.set_depth_camera(None)                                 # (back on depth images of the input size)
    plain.set_depth_camera(None)
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, 1)
    assert gen.host_buffers()[1].shape == (f * h, f * w)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB))
    _differ(gen.read_stage(F.STAGE_FULL_DEPTH), dep, "FULL_DEPTH")
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_under_a_pixel_format(pkg, size, f):
    """Bayer RGGB and NV12: the unpack runs at the input size, the bin behind it; the format before binning for the
    mosaic, behind it for NV12"""
    F = pkg.frontend
    w, h = size
    _, dep, _, bdep = _frame(pkg, w, h, f, 1)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for fmt in (K.BAYER_RGGB8, K.NV12):
        packed, full, binned = _packed(w, h, f, fmt)
        gen.set_input_binning(None)
        gen.set_pixel_format(K.BGR8)
        if fmt == K.NV12:
            gen.set_input_binning(F.Binning(f, 1))
            gen.set_pixel_format(fmt)
        else:
            gen.set_pixel_format(fmt)
            gen.set_input_binning(F.Binning(f, 1))
        assert gen.pixel_format() == fmt and gen.input_binning() == F.Binning(f, 1)
        assert gen.host_buffers()[0].shape == K.layout(fmt, f * w, f * h) == packed.shape
        for _ in range(2):
            cloud = gen.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_FULL_BGR), full, "FULL_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), binned, "INPUT_BGR under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(binned, bdep, 1, F.FEATURES_RGB), "%s f %d" % (K.NAMES[fmt], f))
            _oracle_cloud(gen, F, cloud, binned, 1, F.FEATURES_RGB)
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_float_depth(pkg, size, f):
    """the conversion runs at the input size, the bin behind it; the format before binning at f = 3, behind it otherwise"""
    F = pkg.frontend
    w, h = size
    bgr, dep, bbgr, _ = _frame(pkg, w, h, f, 2)
    fl = KD.metres(dep, 4999.0, KD.F32)
    plane = KD.convert(fl, KD.F32, 1.0, 5000.0)
    bdep = B.bin_depth(plane, f, 2)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    if f == 3:
        gen.set_depth_format(KD.F32)
        gen.set_input_binning(F.Binning(f, 2))
    else:
        gen.set_input_binning(F.Binning(f, 2))
        gen.set_depth_format(KD.F32)
    assert gen.depth_format() == (KD.F32, 1.0) and gen.input_binning() == F.Binning(f, 2)
    hb = gen.host_buffers()[1]
    assert hb.shape == (f * h, f * w) and hb.dtype == np.float32
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_FULL_DEPTH), plane, "FULL_DEPTH")
        _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH")
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB), "float depth f %d" % f)
    gen.set_depth_format(KD.U16)
    assert gen.input_binning() == F.Binning(f, 2)
    assert _same_cloud(gen.create_pointcloud(bgr, plane, 1, F.FEATURES_RGB), plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB))
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
def test_a_distorting_model(pkg, f):
    """model A (96 x 64) describes the working image: k_fe_rectify resamples what the bin wrote, colour and depth"""
    F = pkg.frontend
    w, h, model = R.SMALL["A"]
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, 1)
    qu, qv = R.rectify_map(model, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_input_binning(F.Binning(f, 1))
    gen.set_camera(F.CameraModel(*model)); plain.set_camera(F.CameraModel(*model))
    assert gen.input_binning() == F.Binning(f, 1) and gen.camera() == F.CameraModel(*model)
    for _ in range(2):
        cloud = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
        _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH")
        _differ(gen.read_stage(F.STAGE_RECT_BGR), R.remap_colour(bbgr, qu, qv), "RECT_BGR")
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB), "model A f %d" % f)
    gen.close(); plain.close()


@pytest.mark.parametrize("f", B.FACTORS)
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_device_input(pkg, size, f):
    """the images in device memory, dense and as slices of wider tensors: the pitched copies go to the input-size buffers"""
    import torch
    F = pkg.frontend
    w, h = size
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, f, 1)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_input_binning(F.Binning(f, 1))
    want = plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB)
    for pad in (0, 3):
        wide_i = np.full((f * h, f * w + pad, 3), 0x5A, np.uint8)
        wide_i[:, :f * w] = bgr
        wide_d = np.full((f * h, f * w + pad), 0x5A5A, np.uint16)
        wide_d[:, :f * w] = dep
        ti, td = torch.from_numpy(wide_i).to("cuda"), torch.from_numpy(wide_d).to("cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            gen.submit_device(ti[:, :f * w], td[:, :f * w], 1, F.FEATURES_RGB)
            cloud = gen.collect()
            _differ(gen.read_stage(F.STAGE_FULL_BGR), bgr, "FULL_BGR")
            _differ(gen.read_stage(F.STAGE_FULL_DEPTH), dep, "FULL_DEPTH")
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR")
            _same_frame(gen, plain, F, cloud, want, "device input f %d pad %d" % (f, pad))
        torch.cuda.synchronize()
        assert ti.cpu().numpy().tobytes() == wide_i.tobytes() and td.cpu().numpy().tobytes() == wide_d.tobytes()
        # an image of the working size is too small for its rows: refused, nothing enqueued
        small = torch.from_numpy(bbgr.copy()).to("cuda")
        with pytest.raises((pkg.capi.CvoHipError, ValueError)):
            gen.submit_device(small, td[:, :f * w], 1, F.FEATURES_RGB)
    gen.close(); plain.close()


# ---- 3. the context ----------------------------------------------------------------------------------

ALTERNATING = ((2, 1), None, (3, 9), (2, 1), (2, 4), (4, 16), None, (3, 1))


def _alternating(pkg):
    """settings a, b and off alternating on one context, two pictures alternating: every frame's planes by bytes and its
    cloud by bits.  A graph captured under another setting, or without one, and launched again would give that frame's."""
    F = pkg.frontend
    w, h = 96, 64
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    k, sizes = 0, []
    for setting in ALTERNATING:
        gen.set_input_binning(None if setting is None else F.Binning(*setting))
        assert gen.input_binning() == (None if setting is None else F.Binning(*setting))
        f, dmin = setting or (1, 1)
        for _ in range(2):
            ftype = F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB
            bgr, dep = pkg.data.synthetic_rgbd_frame(width=f * w, height=f * h, seed=72 + k % 2, texture=1.0)
            bbgr, bdep = (bgr, dep) if setting is None else (B.bin_colour(bgr, f), B.bin_depth(dep, f, dmin))
            cloud = gen.create_pointcloud(bgr, dep, 1, ftype)
            if setting is not None:
                _differ(gen.read_stage(F.STAGE_INPUT_BGR), bbgr, "INPUT_BGR of frame %d" % k)
            _differ(gen.read_stage(F.STAGE_RAW_DEPTH), bdep, "RAW_DEPTH of frame %d" % k)
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bbgr, bdep, 1, ftype), "frame %d" % k)
            sizes.append(len(cloud[0]))
            k += 1
    gen.close(); plain.close()
    return sizes


def test_settings_alternate_on_one_context(pkg):
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    assert len(_alternating(pkg)) == 16


def test_settings_alternate_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_binning as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set binning, ran a frame under it and went back to off: stages by bytes, the cloud by bits,
    and the oracle's; the new stages answer INVALID on both, with a message of their own"""
    F = pkg.frontend
    w, h = 96, 64
    bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)
    never, back = _generator(pkg, w, h), _generator(pkg, w, h)
    big, bigd, _, _ = _frame(pkg, w, h, 2, 1)
    back.set_input_binning(F.Binning(2, 1))
    under = back.create_pointcloud(big, bigd, 1, F.FEATURES_RGB)
    back.set_input_binning(None)
    never.set_input_binning(None)                              # the value it has: nothing happens
    clouds = []
    for gen in (never, back):
        assert gen.input_binning() is None
        for k in range(2):
            clouds.append(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB))
        for stage in (F.STAGE_FULL_BGR, F.STAGE_FULL_RIGHT_BGR, F.STAGE_FULL_DEPTH, F.STAGE_INPUT_BGR):
            _no_plane(pkg, gen, stage)
        with pytest.raises(pkg.capi.CvoHipError):
            gen.read_stage(F.STAGE_FULL_BGR)
        assert b"input binning is not set" in F.lib().cvo_fe_last_error(gen._h)
        assert gen.host_buffers()[0].shape == (h, w, 3) and gen.host_buffers()[1].shape == (h, w)
    _same_frame(back, never, F, clouds[3], clouds[1], "back at off", extra=(F.STAGE_GATE,))
    _differ(never.read_stage(F.STAGE_RECT_BGR), bgr, "the image as uploaded")
    _differ(never.read_stage(F.STAGE_RAW_DEPTH), dep, "the depth image as uploaded")
    _oracle_cloud(never, F, clouds[0], bgr, 1, F.FEATURES_RGB)
    assert _same_cloud(clouds[0], clouds[1]) and _same_cloud(clouds[2], clouds[3]) and not _same_cloud(under, clouds[0])
    never.close(); back.close()


def test_refusals_carry_their_sentence_and_leave_the_context_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    L = F.lib()
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    message = lambda gen: L.cvo_fe_last_error(gen._h)
    w, h = 96, 64
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    bgr, dep, bbgr, bdep = _frame(pkg, w, h, 3, 4)
    want = plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB)
    good = F.Binning(3, 4)
    gen.set_input_binning(good)
    for bad in (F.Binning(1, 1), F.Binning(5, 1), F.Binning(0, 1), F.Binning(-2, 1), F.Binning(3, 0), F.Binning(3, 10),
                F.Binning(2, 5), F.Binning(4, 17), F.Binning(3, 4, 1)):
        with pytest.raises(Err):
            gen.set_input_binning(bad)
        assert message(gen).startswith(b"set_input_binning: " + RULE) and gen.input_binning() == good
        assert not F.check_binning(bad, w, h)
    assert _same_cloud(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), want)
    # a frame in flight: refused, even the setting in force and "off"
    gen.submit(bgr, dep, 1, F.FEATURES_RGB)
    for other in (good, F.Binning(2, 1), None):
        with pytest.raises(Err):
            gen.set_input_binning(other)
        assert b"set_input_binning: a frame is in flight" == message(gen)
    assert _same_cloud(gen.collect(), want) and gen.input_binning() == good
    # strides and sizes speak of the input image
    img, dp = bgr.ctypes.data_as(u8p), dep.ctypes.data_as(u16p)
    fw = 3 * w
    assert L.cvo_fe_submit(gen._h, img, w * 3, dp, fw * 2, 1, F.FEATURES_RGB) == -1 and b"submit" in message(gen)
    assert L.cvo_fe_submit(gen._h, img, fw * 3 - 1, dp, fw * 2, 1, F.FEATURES_RGB) == -1
    assert L.cvo_fe_submit(gen._h, img, fw * 3, dp, fw * 2 - 2, 1, F.FEATURES_RGB) == -1
    assert L.cvo_fe_submit(gen._h, img, fw * 3, dp, fw * 2, 1, F.FEATURES_RGB) == 0
    assert _same_cloud(gen.collect(), want)
    with pytest.raises(ValueError):
        gen.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB)  # images of the working size are not this context's
    assert L.cvo_fe_get_input_binning(gen._h, None, None) == -1 and L.cvo_fe_set_input_binning(None, C.byref(good)) == -1
    gen.close(); plain.close()
    # a size the factor takes over 8192
    wide = F.PcdGenerator(2752, 64)
    for ok_f, bad_f in ((2, 3),):
        with pytest.raises(Err):
            wide.set_input_binning(F.Binning(bad_f, 1))
        assert message(wide).startswith(b"set_input_binning: " + RULE) and b"8192" in message(wide)
        assert wide.input_binning() is None
        wide.set_input_binning(F.Binning(ok_f, 1))
    wide.close()
    # a pixel format in force that does not fit the input size, and, in turn, a format checked at the input size
    odd = F.PcdGenerator(66, 65)
    odd.set_pixel_format(K.YUY2)                               # (an even width: fits 66 x 65)
    odd.set_input_binning(F.Binning(3, 1))                     # (198 x 195: still an even width)
    with pytest.raises(Err):
        odd.set_pixel_format(K.NV12)                           # (an odd height, also at the input size)
    assert b"set_pixel_format" in message(odd) and odd.pixel_format() == K.YUY2
    odd.set_input_binning(F.Binning(2, 1))                     # (132 x 130: NV12 fits now ...)
    odd.set_pixel_format(K.NV12)
    with pytest.raises(Err):
        odd.set_input_binning(F.Binning(3, 1))                 # (... and would not at 198 x 195)
    assert b"set_input_binning: the pixel format in force does not fit the input size" in message(odd)
    with pytest.raises(Err):
        odd.set_input_binning(None)                            # (nor at 66 x 65)
    assert odd.input_binning() == F.Binning(2, 1) and odd.pixel_format() == K.NV12
    packed = K.pack(G.frame(132, 130, 72), K.NV12)
    dep2 = pkg.data.synthetic_rgbd_frame(width=132, height=130, seed=72, texture=1.0)[1]
    odd.create_pointcloud(packed, dep2, 1, F.FEATURES_RGB)
    _differ(odd.read_stage(F.STAGE_INPUT_BGR), B.bin_colour(K.unpack(packed, K.NV12, 132, 130), 2), "INPUT_BGR at 66x65")
    odd.close()
    # the stand-alone entries
    src, out = np.zeros((4, 8, 3), np.uint8), np.zeros((2, 4, 3), np.uint8)
    s, o = src.ctypes.data_as(u8p), out.ctypes.data_as(u8p)
    assert L.cvo_fe_bin_image(0, None, 24, 4, 2, 2, o) == -1 and L.cvo_fe_bin_image(0, s, 24, 4, 2, 2, None) == -1
    assert L.cvo_fe_bin_image(0, s, 23, 4, 2, 2, o) == -1 and L.cvo_fe_bin_image(0, s, 24, 4, 2, 5, o) == -1
    assert L.cvo_fe_bin_image(0, s, 24, 0, 2, 2, o) == -1 and L.cvo_fe_bin_image(0, s, 24, 4, 0, 2, o) == -1
    assert L.cvo_fe_bin_image(0, s, 24, 4097, 2, 2, o) == -1 and L.cvo_fe_bin_image(0, s, 24, 4, 2, 2, o) == 0 and not out.any()
    dsrc, dout, n = np.ones((4, 8), np.uint16), np.zeros((2, 4), np.uint16), C.c_int(-1)
    ds, do = dsrc.ctypes.data_as(u16p), dout.ctypes.data_as(u16p)
    b2 = F.Binning(2, 4)
    assert L.cvo_fe_bin_depth(0, None, 16, 4, 2, C.byref(b2), do, C.byref(n)) == -1
    assert L.cvo_fe_bin_depth(0, ds, 16, 4, 2, None, do, C.byref(n)) == -1 and L.cvo_fe_bin_depth(0, ds, 16, 4, 2, C.byref(b2), do, None) == -1
    assert L.cvo_fe_bin_depth(0, ds, 15, 4, 2, C.byref(b2), do, C.byref(n)) == -1
    assert L.cvo_fe_bin_depth(0, ds, 16, 4, 2, C.byref(F.Binning(2, 5)), do, C.byref(n)) == -1
    assert L.cvo_fe_bin_depth(0, ds, 16, 4, 2, C.byref(b2), do, C.byref(n)) == 0 and n.value == 8 and (dout == 1).all()


def test_binning_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 2048 x 1024 the input images of factor 4 are 96 + 64 MiB on the device, many times the 8 MiB a
    reading of the free device memory resolves.  Refused settings leave it where it was, and at off the device memory
    is that of a context that never made the call."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(2048, 1024)
    free0 = free()
    for bad in (F.Binning(5, 1), F.Binning(4, 17)):
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_input_binning(bad)
    gen.set_input_binning(None)
    free1 = free()
    assert abs(free0 - free1) < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_input_binning(F.Binning(4, 1))
    free2 = free()
    assert free1 - free2 >= 128 * MiB, "the setting took only %d bytes" % (free1 - free2)
    gen.set_input_binning(F.Binning(4, 16))                    # (depth_min alone: nothing is built)
    assert abs(free() - free2) < 8 * MiB
    gen.set_input_binning(F.Binning(2, 1))                     # 24 + 16 MiB in place of 96 + 64
    free3 = free()
    assert free3 - free2 >= 96 * MiB, "a smaller factor gave back only %d bytes" % (free3 - free2)
    gen.set_input_binning(None)
    free4 = free()
    assert abs(free4 - free0) < 8 * MiB, "at off the free memory is %d bytes from where it was" % (free0 - free4)
    gen.close()


# ---- 4. the caller-side paths ------------------------------------------------------------------------

def test_the_staging_buffers_filled_in_place(pkg):
    """host_buffers() under binning are the images of the input size; filled in place and submitted they give the same cloud"""
    F = pkg.frontend
    w, h = 96, 64
    gen = _generator(pkg, w, h)
    for f in (2, 4, 1, 3):
        gen.set_input_binning(None if f == 1 else F.Binning(f, 1))
        bgr, dep = pkg.data.synthetic_rgbd_frame(width=f * w, height=f * h, seed=72, texture=1.0)
        want = gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB)
        img, d = gen.host_buffers()
        assert img.shape == (f * h, f * w, 3) and d.shape == (f * h, f * w) and d.dtype == np.uint16
        img[...] = 0
        d[...] = 0
        gen.create_pointcloud(np.zeros_like(bgr), dep, 1, F.FEATURES_RGB)   # (another frame in between)
        img[...] = bgr
        d[...] = dep
        for _ in range(2):
            assert _same_cloud(gen.create_pointcloud(img, d, 1, F.FEATURES_RGB), want)
            if f > 1:
                _differ(gen.read_stage(F.STAGE_FULL_BGR), bgr, "FULL_BGR from the staging image")
    gen.close()


@pytest.mark.parametrize("with_camera", [False, True], ids=["table row", "camera"])
def test_run_frames_takes_the_binning(pkg, with_camera):
    """run_frames(input_binning=) on frames of 640 x 480 with the INPUT images' camera (the table's row 1, or a model):
    a generator of 320 x 240 is made, and the cloud of frame 0 is that of a generator of that size under bin_camera's
    model on the restatement's images; a first frame that is no multiple of the factor is a ValueError"""
    F = pkg.frontend
    f, dmin = 2, 2
    frames = _four_frames(pkg, 75)[:1]
    row = F.camera(1)
    model = (F.CameraModel(4000.0, 510.0, 512.0, 300.5, 250.25) if with_camera else
             F.CameraModel(row["scaling_factor"], row["fx"], row["fy"], row["cx"], row["cy"]))
    made = []

    class Spy(F.PcdGenerator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def collect(self):
            self.cloud = super().collect()
            self.stages = (self.read_stage(F.STAGE_INPUT_BGR), self.read_stage(F.STAGE_RAW_DEPTH), self.read_stage(F.STAGE_MAP))
            return self.cloud

    reg, buf = pkg.Cvo(), io.StringIO()
    orig = F.PcdGenerator
    F.PcdGenerator = Spy
    try:
        assert F.run_frames(reg, frames[:1], 1, writer=pkg.trajectory.TrajectoryWriter(buf), input_binning=F.Binning(f, dmin),
                            camera=model if with_camera else None, device=False) == 1
        with pytest.raises(ValueError):
            F.run_frames(reg, frames[:1], 1, input_binning=F.Binning(3, 1), device=False)   # 640 is no multiple of 3
    finally:
        F.PcdGenerator = orig
    gen = made[0]
    assert (gen.width, gen.height) == (320, 240) and gen.input_binning() == F.Binning(f, dmin)
    assert gen.camera() == F.bin_camera(model, f)
    name, bgr, dep = frames[0]
    bbgr, bdep = B.bin_colour(bgr, f), B.bin_depth(dep, f, dmin)
    _differ(gen.stages[0], bbgr, "INPUT_BGR"); _differ(gen.stages[1], bdep, "RAW_DEPTH")
    plain = F.PcdGenerator(320, 240)
    plain.set_camera(F.bin_camera(model, f))
    want = plain.create_pointcloud(bbgr, bdep, 1, F.FEATURES_RGB)
    assert _same_cloud(gen.cloud, want) and len(want[0]) >= 20
    _differ(gen.stages[2], plain.read_stage(F.STAGE_MAP), "MAP")
    reg.close(); plain.close()
    for g in made:
        g.close()


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_binning(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_input_binning (tests/cpp/cvo_binning_demo.cpp): the clouds the C++ object
    registers and its pose lines equal those of the Python path at the working size, under bin_camera's model of the
    table's row 1, on the restatement's images"""
    F = pkg.frontend
    w, h, f, dmin = 320, 240, 2, 2
    full = _four_frames(pkg, 75)
    binned = [(name, B.bin_colour(bgr, f), B.bin_depth(dep, f, dmin)) for name, bgr, dep in full]
    mixed = [binned[k] if k == 2 else full[k] for k in range(4)]
    exe = str(tmp_path / "cvo_binning_demo")
    lib = os.path.join(ROOT, "cvo-rgbd_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "cvo_binning_demo.cpp"), "-L", lib, "-lcvo_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=120)
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", 4, w, h) + struct.pack("<ii", f, dmin))
        for name, bgr, dep in mixed:
            fh.write(name.encode().ljust(32, b"\0") + bgr.tobytes() + dep.tobytes())
    got = subprocess.run([exe, path, mode_name], check=True, capture_output=True, text=True, timeout=120).stdout.strip().split("\n")
    row = F.camera(1)
    gen = F.PcdGenerator(w, h)
    gen.set_camera(F.bin_camera(F.CameraModel(row["scaling_factor"], row["fx"], row["fy"], row["cx"], row["cy"]), f))
    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, binned, lambda k: ["refused a bad binning"] if k == 3 else [])
    assert got == ["refused a bad binning"] + want
    assert min(sizes) > 100
    gen.close()
