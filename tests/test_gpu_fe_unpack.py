"""GPU: the pixel formats of the front end (cvo_fe_set_pixel_format, cvo_fe_unpack_image; the unpack contract of
include/cvo_frontend.h): k_fe_unpack of csrc/cvo_unpack.hip against the restatement tests/fe_unpack_ref.py by bytes --
all twelve formats at every size and input of fe_unpack_ref.cases() -- and frames of every kind under every format:
the unpacked images by bytes, and every later stage and the cloud, by bytes and bits, against a second context in BGR8
that was fed the restatement's image, and against the CPU restatement of the front end (oracle/frontend_oracle.c) on
it.  Formats alternating on one context, with and without captured graphs (a stale graph would show), a context that
never made the call, the refusals with their messages, the memory, the staging buffers, run_frames and the C++ objects
above.  Which errors of a tiled, four-pixels-per-thread unpack these inputs would show is asserted in
tests/test_fe_unpack_cpu.py."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_depth_ref as D
import fe_gate_ref as G
import fe_lidar_ref as KL
import fe_rectify_ref as R
import fe_stereo_ref as S
import fe_stereo_rig_ref as RG
import fe_unpack_ref as K
from fe_gpu_common import ROOT, _demo_lines, _device_path_lines, _four_frames, _same_cloud
from oracle import pyoracle_fe as fo

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
SIZES = ((64, 64), (96, 64))
PACKED = tuple(f for f in K.FORMATS if f != K.BGR8)
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


def _picture(w, h, fmt, seed=72):
    """(the packed image of a picture as a generator takes it, the restatement's unpacked image)"""
    def make():
        packed = K.pack(G.frame(w, h, seed), fmt)
        bgr = K.unpack(packed, fmt, w, h)
        return (bgr if fmt == K.BGR8 else packed), bgr
    return _ref(("picture", w, h, fmt, seed), make)


def _depth(pkg, w, h):
    return pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=72, texture=1.0)[1]


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _later_stages(F):
    return (F.STAGE_RECT_BGR, F.STAGE_GRAY, F.STAGE_RECT_DEPTH, F.STAGE_MAP, F.STAGE_AG0, F.STAGE_DX0, F.STAGE_DY0)


def _same_frame(gen, plain, F, cloud, plain_cloud, what, extra=()):
    """every later stage by bytes and the cloud by bits: the frame of the context in BGR8 fed the unpacked image"""
    for stage in _later_stages(F) + tuple(extra):
        _differ(gen.read_stage(stage), plain.read_stage(stage), "stage %d of %s" % (stage, what))
    assert gen.info() == plain.info(), what
    assert _same_cloud(cloud, plain_cloud) and len(cloud[0]) >= 20, what


def _oracle_cloud(gen, F, cloud, bgr, seq, ftype):
    """the cloud against the front-end oracle on the unpacked colour image and the plane the cloud is made from"""
    ref = fo.create_pointcloud(bgr, gen.read_stage(F.STAGE_RECT_DEPTH), seq, ftype, num_want=gen.num_want)
    assert np.array_equal(gen.read_stage(F.STAGE_MAP), ref["map"])
    assert _same_cloud(cloud, (ref["positions"], ref["features"]))


# ---- 1. the stand-alone entry ------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", K.FORMATS, ids=K.NAMES)
def test_unpack_image_by_bytes(pkg, fmt):
    """every size and input of the format against the restatement; the source is left as it is"""
    F = pkg.frontend
    for w, h, kind in K.cases(fmt):
        src = K.make_input(fmt, w, h, kind)
        arg = src.copy()
        got = F.unpack_image(arg, fmt, w, h)
        assert np.array_equal(arg, src), (w, h, kind)
        _differ(got, K.unpack(src, fmt, w, h), "%s %dx%d %s" % (K.NAMES[fmt], w, h, kind))


@pytest.mark.parametrize("fmt", K.FORMATS, ids=K.NAMES)
def test_unpack_image_takes_a_row_stride(pkg, fmt):
    """rows further apart than their bytes: what lies between them is not read into the image, and stays"""
    F = pkg.frontend
    for w, h in ((10, 6), (130, 34)):
        src = K.make_input(fmt, w, h, "random")
        rows, row = src.shape
        buf = np.full((rows, row + 5), 0xA5, np.uint8)
        buf[:, :row] = src
        arg = buf.copy()
        _differ(F.unpack_image(arg, fmt, w, h, stride=row + 5), K.unpack(src, fmt, w, h), "%s %dx%d" % (K.NAMES[fmt], w, h))
        assert np.array_equal(arg, buf)


# ---- 2. frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_a_depth_frame_under_every_format(pkg, size):
    """INPUT_BGR by bytes; every later stage and the cloud as a context in BGR8 gives them on the restatement's image,
    and as the oracle does; every format twice: the second frame replays the captured graph"""
    F = pkg.frontend
    w, h = size
    dep = _depth(pkg, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    assert gen.pixel_format() == F.PIXEL_BGR8
    for fmt in PACKED:
        packed, bgr = _picture(w, h, fmt)
        gen.set_pixel_format(fmt)
        assert gen.pixel_format() == fmt
        for k in range(2):
            ftype = F.FEATURES_HSV if k else F.FEATURES_RGB
            cloud = gen.create_pointcloud(packed, dep, 1, ftype)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_RECT_BGR), bgr, "RECT_BGR under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, dep, 1, ftype), K.NAMES[fmt])
            _oracle_cloud(gen, F, cloud, bgr, 1, ftype)
            with pytest.raises(pkg.capi.CvoHipError):
                gen.read_stage(F.STAGE_INPUT_RIGHT_BGR)        # no stereo: no right image
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_a_stereo_frame_under_every_format(pkg, size):
    """both images of the pair share the format and one launch unpacks them"""
    F = pkg.frontend
    w, h = size
    st = S.make_stereo(max_disp=32)
    left, right, _ = _ref(("pair", w, h), lambda: S.pair(w, h, 82))
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    plain.set_stereo(S.to_struct(F, st))
    gen.set_pixel_format(K.GREY8)                              # (the format first, stereo behind it ...)
    gen.set_stereo(S.to_struct(F, st))
    assert gen.pixel_format() == K.GREY8
    for fmt in (K.GREY8,) + PACKED:
        pl, pr = K.pack(left, fmt), K.pack(right, fmt)
        ul, ur = K.unpack(pl, fmt, w, h), K.unpack(pr, fmt, w, h)
        gen.set_pixel_format(fmt)                              # (... and, from the second on, the format behind stereo)
        assert gen.stereo() == S.to_struct(F, st)
        for _ in range(2):
            cloud = gen.create_pointcloud_stereo(pl, pr, S.SEQ, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), ul, "INPUT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_INPUT_RIGHT_BGR), ur, "INPUT_RIGHT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_RIGHT_BGR), ur, "RIGHT_BGR under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(ul, ur, S.SEQ, F.FEATURES_RGB), K.NAMES[fmt],
                        extra=(F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_RIGHT_GRAY))
            _oracle_cloud(gen, F, cloud, ul, S.SEQ, F.FEATURES_RGB)
    gen.set_stereo(None)                                       # (the setting survives, and depth frames read it)
    assert gen.pixel_format() == PACKED[-1]
    packed, bgr = _picture(w, h, PACKED[-1])
    dep = _depth(pkg, w, h)
    plain.set_stereo(None)
    assert _same_cloud(gen.create_pointcloud(packed, dep, 1, F.FEATURES_RGB), plain.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB))
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_a_lidar_frame_under_every_format(pkg, size):
    F = pkg.frontend
    w, h = size
    seq = 4
    cam = tuple(F.camera(seq).values())
    s = KL.setting((1, 7, 1, 0.25), **KL.MOUNT)
    points = _ref(("scan", w, h), lambda: (KL.scan_clutter(w, h, 4097, 52, s, cam),))[0]
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_lidar(KL.to_struct(F, s)); plain.set_lidar(KL.to_struct(F, s))
    for fmt in PACKED:
        packed, bgr = _picture(w, h, fmt)
        gen.set_pixel_format(fmt)
        assert gen.lidar() == KL.to_struct(F, s)
        for _ in range(2):
            cloud = gen.create_pointcloud_lidar(packed, points, seq, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud_lidar(bgr, points, seq, F.FEATURES_RGB), K.NAMES[fmt],
                        extra=(F.STAGE_LIDAR_DEPTH, F.STAGE_LIDAR))
            _oracle_cloud(gen, F, cloud, bgr, seq, F.FEATURES_RGB)
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_a_depth_frame_with_a_depth_camera_under_every_format(pkg, size):
    """the depth image keeps its own size and its own staging; only the colour image is packed"""
    F = pkg.frontend
    w, h = size
    cam = (5000.0, 77.6, 77.5, (w - 1) / 2.0, (h - 1) / 2.0)
    rig = D.make_rig(80, 56, (1000.0, 70.0, 70.2, 39.1, 27.4), (-0.12, 0.03, 0.001, -0.002, 0.0), D.K_R, D.K_T)
    raw = D.scene(pkg.data, rig)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_camera(F.CameraModel(*(cam + (ZERO,))))
        g.set_depth_camera(D.to_struct(F, rig))
    for fmt in PACKED:
        packed, bgr = _picture(w, h, fmt)
        gen.set_pixel_format(fmt)
        for _ in range(2):
            cloud = gen.create_pointcloud(packed, raw, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR under " + K.NAMES[fmt])
            assert np.array_equal(gen.read_stage(F.STAGE_RAW_DEPTH), raw)
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, raw, 1, F.FEATURES_RGB), K.NAMES[fmt])
    gen.close(); plain.close()


def test_the_unpack_runs_in_front_of_a_distorting_model(pkg):
    """model C (an odd width): RECT_BGR is fe_rectify_ref of the unpacked image, which differs from INPUT_BGR"""
    F = pkg.frontend
    w, h, model = R.SMALL["C"]
    dep = _depth(pkg, w, h)
    qu, qv = R.rectify_map(model, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    gen.set_camera(F.CameraModel(*model)); plain.set_camera(F.CameraModel(*model))
    for fmt in PACKED:
        if not K.fits(fmt, w, h):
            with pytest.raises(pkg.capi.CvoHipError):
                gen.set_pixel_format(fmt)
            continue
        packed, bgr = _picture(w, h, fmt)
        rect = R.remap_colour(bgr, qu, qv)
        assert not np.array_equal(rect, bgr)
        gen.set_pixel_format(fmt)
        assert gen.camera() == F.CameraModel(*model)
        for _ in range(2):
            cloud = gen.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_RECT_BGR), rect, "RECT_BGR under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB), K.NAMES[fmt])
    gen.close(); plain.close()


def test_the_unpack_runs_in_front_of_a_stereo_rig(pkg):
    """rig A: both rectified images follow from the unpacked raw pair"""
    F = pkg.frontend
    w, h, disp, calib = RG.CALIBS["A"]
    rig = RG.rectify(calib, w, h, RG.DEPTH_SCALE)
    st = S.make_stereo(max_disp=disp)
    raw_l, raw_r = _ref(("rig A",), lambda: RG.render(rig, w, h))
    (qul, qvl), (qur, qvr) = RG.rig_map(rig, 0, w, h), RG.rig_map(rig, 1, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_stereo(S.to_struct(F, st))
        g.set_stereo_rig(RG.to_struct(F, rig))
    for fmt in PACKED:
        pl, pr = K.pack(raw_l, fmt), K.pack(raw_r, fmt)
        ul, ur = K.unpack(pl, fmt, w, h), K.unpack(pr, fmt, w, h)
        gen.set_pixel_format(fmt)
        for _ in range(2):
            cloud = gen.create_pointcloud_stereo(pl, pr, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_INPUT_BGR), ul, "INPUT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_INPUT_RIGHT_BGR), ur, "INPUT_RIGHT_BGR under " + K.NAMES[fmt])
            _differ(gen.read_stage(F.STAGE_RECT_BGR), R.remap_colour(ul, qul, qvl), "the rectified left image")
            _differ(gen.read_stage(F.STAGE_RIGHT_BGR), R.remap_colour(ur, qur, qvr), "the rectified right image")
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(ul, ur, 1, F.FEATURES_RGB), K.NAMES[fmt],
                        extra=(F.STAGE_DISPARITY, F.STAGE_STEREO, F.STAGE_STEREO_VALID))
    gen.close(); plain.close()


# ---- 3. the context ----------------------------------------------------------------------------------

ALTERNATING = (K.BAYER_GRBG8, K.BGR8, K.NV12, K.BAYER_GRBG8, K.YUY2, K.BGRA8, K.BGR8, K.GREY8)


def _alternating(pkg):
    """formats alternating with BGR8 on two alternating pictures: every frame's unpacked image by bytes and its cloud by
    bits.  A graph captured under another format, or under BGR8, and launched again would give that frame's."""
    F = pkg.frontend
    w, h = 96, 64
    dep = _depth(pkg, w, h)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    k, sizes = 0, []
    for fmt in ALTERNATING:
        gen.set_pixel_format(fmt)
        assert gen.pixel_format() == fmt
        for _ in range(2):
            ftype = F.FEATURES_HSV if k % 3 == 0 else F.FEATURES_RGB
            packed, bgr = _picture(w, h, fmt, seed=72 + k % 2)
            cloud = gen.create_pointcloud(packed, dep, 1, ftype)
            if fmt != K.BGR8:
                _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR of frame %d" % k)
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, dep, 1, ftype), "frame %d" % k)
            sizes.append(len(cloud[0]))
            k += 1
    gen.close(); plain.close()
    return sizes


def test_formats_alternate_on_one_context(pkg):
    assert os.environ.get("CVO_FE_NO_GRAPH") is None
    assert len(_alternating(pkg)) == 16


def test_formats_alternate_without_captured_graphs():
    """... and in a session that has CVO_FE_NO_GRAPH in its environment from the start (the library reads it once)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import __graft_entry__ as ge, test_gpu_fe_unpack as T\n"
            "print('sizes', T._alternating(ge.load_package()))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, CVO_FE_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "sizes [" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_a_context_that_never_made_the_call(pkg):
    """... equals one that set a format, ran a frame under it and went back to BGR8: stages by bytes, the cloud by bits,
    and the oracle's; the new stages answer INVALID on both"""
    F = pkg.frontend
    w, h = 96, 64
    bgr = G.frame(w, h, 72)
    dep = _depth(pkg, w, h)
    never, back = _generator(pkg, w, h), _generator(pkg, w, h)
    back.set_pixel_format(K.BAYER_RGGB8)
    packed, unpacked = _picture(w, h, K.BAYER_RGGB8)
    under = back.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
    back.set_pixel_format(K.BGR8)
    never.set_pixel_format(K.BGR8)                             # the value it has: nothing happens
    clouds = []
    for gen in (never, back):
        assert gen.pixel_format() == K.BGR8
        for k in range(2):
            clouds.append(gen.create_pointcloud(bgr, dep, 1, F.FEATURES_RGB))
        for stage in (F.STAGE_INPUT_BGR, F.STAGE_INPUT_RIGHT_BGR):
            with pytest.raises(pkg.capi.CvoHipError):
                gen.read_stage(stage)
            assert b"read_stage" in F.lib().cvo_fe_last_error(gen._h)
        assert gen.host_buffers()[0].shape == (h, w, 3)
    _same_frame(back, never, F, clouds[3], clouds[1], "back in BGR8", extra=(F.STAGE_RAW_DEPTH, F.STAGE_GATE))
    _differ(never.read_stage(F.STAGE_RECT_BGR), bgr, "the image as uploaded")
    _oracle_cloud(never, F, clouds[0], bgr, 1, F.FEATURES_RGB)
    assert _same_cloud(clouds[0], clouds[1]) and _same_cloud(clouds[2], clouds[3]) and not _same_cloud(under, clouds[0])
    never.close(); back.close()


def test_refusals_carry_their_message_and_leave_the_context_unchanged(pkg):
    F = pkg.frontend
    Err = pkg.capi.CvoHipError
    L = F.lib()
    u8p = C.POINTER(C.c_uint8)
    dep = lambda w, h: _depth(pkg, w, h)
    message = lambda gen: L.cvo_fe_last_error(gen._h)
    # formats a size does not fit
    odd_w, odd_h = F.PcdGenerator(65, 64), F.PcdGenerator(64, 65)
    for gen, bad, good in ((odd_w, (K.YUY2, K.UYVY, K.NV12), K.BAYER_RGGB8), (odd_h, (K.NV12,), K.YUY2)):
        for fmt in bad:
            with pytest.raises(Err):
                gen.set_pixel_format(fmt)
            assert b"set_pixel_format" in message(gen) and gen.pixel_format() == K.BGR8
        gen.set_pixel_format(good)
        w, h = gen.width, gen.height
        packed = K.pack(G.frame(w, h, 72), good)
        gen.create_pointcloud(packed, dep(w, h), 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_INPUT_BGR), K.unpack(packed, good, w, h), "INPUT_BGR at %dx%d" % (w, h))
        gen.close()
    w, h = 96, 64
    gen = _generator(pkg, w, h)
    d = dep(w, h)
    for bad in (-1, 12, 2 ** 31 - 1):
        with pytest.raises(Err):
            gen.set_pixel_format(bad)
        assert b"set_pixel_format" in message(gen) and gen.pixel_format() == K.BGR8
    with pytest.raises(Err):
        gen.set_pixel_format(2 ** 31)
    packed, bgr = _picture(w, h, K.YUY2)
    gen.set_pixel_format(K.YUY2)
    want = gen.create_pointcloud(packed, d, 1, F.FEATURES_RGB)
    for bad in (-1, 12, K.BGR8 - 13):
        with pytest.raises(Err):
            gen.set_pixel_format(bad)
        assert gen.pixel_format() == K.YUY2
    # a set while a frame is pending, even to the format in force
    gen.submit(packed, d, 1, F.FEATURES_RGB)
    for other in (K.BGR8, K.YUY2, K.GREY8):
        with pytest.raises(Err):
            gen.set_pixel_format(other)
        assert b"in flight" in message(gen)
    assert _same_cloud(gen.collect(), want) and gen.pixel_format() == K.YUY2
    # a stride below row_bytes (2w here: w * 3 - 1 would pass under BGR8's rule only by being larger), null pointers
    img, dp = packed.ctypes.data_as(u8p), d.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.cvo_fe_submit(gen._h, img, 2 * w - 1, dp, 2 * w, 1, F.FEATURES_RGB) == -1 and b"submit" in message(gen)
    assert L.cvo_fe_submit(gen._h, None, 2 * w, dp, 2 * w, 1, F.FEATURES_RGB) == -1 and b"submit" in message(gen)
    assert L.cvo_fe_submit(gen._h, img, 2 * w, None, 2 * w, 1, F.FEATURES_RGB) == -1 and b"submit" in message(gen)
    assert L.cvo_fe_submit(gen._h, img, 2 * w, dp, 2 * w, 1, F.FEATURES_RGB) == 0      # the dense stride is taken
    assert _same_cloud(gen.collect(), want)
    gen.set_pixel_format(K.BGRA8)                              # a row of 4w: BGR8's 3w is now too little
    wide = K.pack(bgr, K.BGRA8)
    assert L.cvo_fe_submit(gen._h, wide.ctypes.data_as(u8p), 3 * w, dp, 2 * w, 1, F.FEATURES_RGB) == -1
    assert _same_cloud(gen.create_pointcloud(wide, d, 1, F.FEATURES_RGB), want)
    with pytest.raises(ValueError):
        gen.create_pointcloud(bgr, d, 1, F.FEATURES_RGB)      # h x w x 3 bytes are not this format's
    assert L.cvo_fe_get_pixel_format(gen._h, None) == -1
    gen.close()
    # the stand-alone entry
    one = np.zeros((2, 16), np.uint8)
    for bad_w, bad_h in ((0, 2), (2, 0), (8193, 1), (1, 8193)):
        with pytest.raises((Err, ValueError)):
            F.unpack_image(np.zeros(max(bad_w, 1) * max(bad_h, 1), np.uint8), K.GREY8, bad_w, bad_h)
    out = np.zeros((2, 4, 3), np.uint8)
    o, s = out.ctypes.data_as(u8p), one.ctypes.data_as(u8p)
    assert L.cvo_fe_unpack_image(0, None, 16, 4, 2, K.GREY8, o) == -1 and L.cvo_fe_unpack_image(0, s, 16, 4, 2, K.GREY8, None) == -1
    assert L.cvo_fe_unpack_image(0, s, 3, 4, 2, K.GREY8, o) == -1 and L.cvo_fe_unpack_image(0, s, 16, 4, 2, 12, o) == -1
    assert L.cvo_fe_unpack_image(0, s, 16, 3, 2, K.YUY2, o) == -1 and L.cvo_fe_unpack_image(0, s, 16, 4, 1, K.NV12, o) == -1
    assert L.cvo_fe_unpack_image(0, s, 16, 4, 2, K.GREY8, o) == 0 and not out.any()


def test_the_format_takes_memory_only_once_set_and_gives_it_back(pkg):
    """On a context of 4096 x 2048 a packed BGRA image is 32 MiB, four times the 8 MiB a reading of the free device
    memory resolves.  Refused formats leave it where it was, the first format is seen by the same reading, and back in
    BGR8 the device memory is that of a context that never made the call."""
    import torch
    F = pkg.frontend
    MiB = 1024 * 1024

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    gen = F.PcdGenerator(4096, 2048)
    free0 = free()
    for bad in (-1, 12):
        with pytest.raises(pkg.capi.CvoHipError):
            gen.set_pixel_format(bad)
    gen.set_pixel_format(K.BGR8)
    free1 = free()
    assert abs(free0 - free1) < 8 * MiB, "refused calls took %d bytes" % (free0 - free1)
    gen.set_pixel_format(K.BGRA8)
    free2 = free()
    assert free1 - free2 >= 24 * MiB, "the first format took only %d bytes" % (free1 - free2)
    gen.set_pixel_format(K.GREY8)                              # 8 MiB in place of 32
    free3 = free()
    assert free3 - free2 >= 16 * MiB, "a smaller format gave back only %d bytes" % (free3 - free2)
    gen.set_pixel_format(K.BGR8)
    free4 = free()
    assert abs(free4 - free0) < 8 * MiB, "back in BGR8 the free memory is %d bytes from where it was" % (free0 - free4)
    gen.close()


# ---- 4. the caller-side paths ------------------------------------------------------------------------

def test_the_staging_buffers_filled_in_place(pkg):
    """host_buffers() under a format is the packed image, rows x row_bytes; filled in place and submitted it gives the
    same cloud, for a depth frame under every format"""
    F = pkg.frontend
    w, h = 96, 64
    dep = _depth(pkg, w, h)
    gen = _generator(pkg, w, h)
    for fmt in (K.NV12, K.BGRA8, K.BAYER_BGGR8, K.BGR8):
        packed, bgr = _picture(w, h, fmt)
        gen.set_pixel_format(fmt)
        want = gen.create_pointcloud(packed, dep, 1, F.FEATURES_RGB)
        img, d = gen.host_buffers()
        assert img.shape == ((h, w, 3) if fmt == K.BGR8 else K.layout(fmt, w, h)) == packed.shape and d.shape == (h, w)
        img[...] = 0
        gen.create_pointcloud(np.zeros_like(packed), dep, 1, F.FEATURES_RGB)   # (another frame in between)
        img[...] = packed.reshape(img.shape)
        d[...] = dep
        for _ in range(2):
            assert _same_cloud(gen.create_pointcloud(img, d, 1, F.FEATURES_RGB), want)
            if fmt != K.BGR8:
                _differ(gen.read_stage(F.STAGE_INPUT_BGR), bgr, "INPUT_BGR from the staging image")
    gen.close()


RUN_FORMATS = {"cvo": K.BAYER_RGGB8, "acvo": K.NV12}


def _frames(pkg, fmt):
    """(the four frames packed in fmt, the same with the restatement's unpacked images)"""
    frames = _four_frames(pkg, 75)
    packed = [(name, K.pack(bgr, fmt), dep) for name, bgr, dep in frames]
    unpacked = [(name, _ref(("run", fmt, k), lambda: (K.unpack(p, fmt, 640, 480),))[0], dep) for k, (name, p, dep) in enumerate(packed)]
    return packed, unpacked


def test_run_frames_takes_the_format(pkg):
    """run_frames(pixel_format=) on the packed frames = run_frames without it on the restatement's images: the same poses"""
    F = pkg.frontend
    fmt = K.YUY2
    packed, unpacked = _frames(pkg, fmt)
    poses = []
    for fr, f in ((packed, fmt), (unpacked, None)):
        reg, buf = pkg.Cvo(), io.StringIO()
        gen = F.PcdGenerator(640, 480)
        assert F.run_frames(reg, fr, 1, writer=pkg.trajectory.TrajectoryWriter(buf), generator=gen, pixel_format=f) == 4
        assert gen.pixel_format() == (K.BGR8 if f is None else f)
        _differ(gen.read_stage(F.STAGE_RECT_BGR), unpacked[3][1], "the last frame's image")
        poses.append((buf.getvalue(), reg.accum_transform.copy(), reg.num_iterations))
        reg.close(); gen.close()
    assert poses[1][0] == poses[0][0] and np.array_equal(poses[1][1], poses[0][1]) and poses[1][2] == poses[0][2] > 0
    assert len(poses[0][0].strip().split("\n")) == 4


@pytest.mark.parametrize("mode_name", ["cvo", "acvo"])
def test_cpp_objects_take_the_format(pkg, tmp_path, mode_name):
    """include/cvo.hpp registration::set_pixel_format (tests/cpp/cvo_pixel_format_demo.cpp): the clouds the C++ object
    registers and its pose lines equal those of the Python path in BGR8 on the restatement's images"""
    F = pkg.frontend
    w, h = 640, 480
    fmt = RUN_FORMATS[mode_name]
    packed, unpacked = _frames(pkg, fmt)
    mixed = [unpacked[k] if k == 2 else packed[k] for k in range(4)]
    got = _demo_lines(tmp_path, "cvo_pixel_format_demo", mixed, w, h, np.int32(fmt).tobytes(), [mode_name])
    gen = F.PcdGenerator(w, h)
    want, sizes, _ = _device_path_lines(pkg, mode_name, gen, unpacked, lambda k: ["refused a bad format"] if k == 3 else [])
    assert got == ["refused a bad format"] + want
    assert min(sizes) > 100
    gen.close()
