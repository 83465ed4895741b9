"""GPU: the depth formats of the front end (cvo_fe_set_depth_format, cvo_fe_convert_depth; the depth-format contract of
include/cvo_frontend.h): k_fe_depth_convert of csrc/cvo_depthfmt.hip against the restatement tests/fe_depthfmt_ref.py by
bytes -- both float formats at every shape, pitch and input of fe_depthfmt_ref.cases() -- and depth frames under a float
format: RAW_DEPTH by bytes, and every later stage and the cloud, by bytes and bits, against a second context in U16 fed
the restatement's plane.  Which errors of a conversion these inputs would show is asserted in
tests/test_fe_depthfmt_cpu.py."""
import numpy as np
import pytest

import fe_depth_ref as D
import fe_depthfmt_ref as K
import fe_gate_ref as G
import fe_stereo_ref as S
from fe_gpu_common import _same_cloud

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (96, 72))
IDS = ["%dx%d" % s for s in SIZES]
LENS = (0.05, -0.02, 0.001, 0.001, 0.0)
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


def _differ(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s differs at %d places, first at %s: %s against %s"
                             % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _generator(pkg, w, h):
    return pkg.frontend.PcdGenerator(w, h, num_want=w * h // 8)


def _scene(w, h, fmt, src_scale, unit=1.0, seed=72):
    """(colour image, the float depth plane a network would hand over): the gate scene's depth -- holes, a near box, a
    far strip -- in `unit` metres, stretched by 3 parts in 10^4 so that the products are no integers"""
    def make():
        dep = G.gate_scene(w, h, seed)
        with np.errstate(all="ignore"):
            fl = (dep.astype(np.float32) / np.float32(src_scale)) * np.float32(1.0003) / np.float32(unit)
        fl[1, 1], fl[2, 2], fl[3, 3] = np.nan, -1.0, np.inf
        return G.frame(w, h, seed), fl.astype(K.DTYPES[fmt])
    return _ref(("scene", w, h, fmt, src_scale, unit, seed), make)


def _same_frame(gen, plain, F, cloud, plain_cloud, what, extra=()):
    """every later stage by bytes and the cloud by bits: the frame of the context in U16 fed the converted plane"""
    for stage in (F.STAGE_RECT_BGR, F.STAGE_RAW_DEPTH, F.STAGE_RECT_DEPTH, F.STAGE_UNGATED_DEPTH, F.STAGE_MAP, F.STAGE_AG0) + tuple(extra):
        _differ(gen.read_stage(stage), plain.read_stage(stage), "stage %d of %s" % (stage, what))
    assert gen.info() == plain.info(), what
    assert _same_cloud(cloud, plain_cloud) and len(cloud[0]) >= 20, what


# ---- 1. the stand-alone entry ------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", K.FLOATS, ids=[K.NAMES[f] for f in K.FLOATS])
def test_convert_depth_by_bytes(pkg, fmt):
    """every shape, pitch and input of the format against the restatement; the source and the gaps are left as they are"""
    F = pkg.frontend
    for w, h, pad, kind in K.cases(fmt):
        plane, unit, scale = K.make_input(fmt, w, h, kind)
        buf, pitch = K.padded(plane, pad)
        arg = buf.copy()
        got = F.convert_depth(arg, fmt, w, h, unit, scale, stride=pitch)
        assert np.array_equal(arg, buf), (w, h, pad, kind)
        _differ(got, K.convert(plane, fmt, unit, scale), "%s %dx%d pad %d %s" % (K.NAMES[fmt], w, h, pad, kind))


def test_the_named_values_on_the_device(pkg):
    """what the contract's table says, value by value, from the kernel"""
    F = pkg.frontend
    for config in K.CONFIGS:
        unit, scale, vals, want = K.named_values(config)
        got = F.convert_depth(vals.reshape(1, -1), K.F32, len(vals), 1, unit, scale)[0]
        assert got.tolist() == want.tolist(), config


# ---- 2. frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_of_the_tables_camera(pkg, size):
    """RAW_DEPTH is the restatement's plane; the frame is that of a U16 context fed it; each format twice (the second
    frame replays the captured graph), in metres and in millimetres"""
    F = pkg.frontend
    w, h = size
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    assert gen.depth_format() == (F.DEPTH_U16, 1.0)
    for fmt in K.FLOATS:
        for unit in (1.0, 0.001):
            bgr, fl = _scene(w, h, fmt, 5000.0, unit)
            want = K.convert(fl, fmt, unit, K.frame_scale(5000.0))
            assert (want != 0).sum() > w * h // 2 and (want == 0).sum() > 10
            gen.set_depth_format(fmt, unit)
            assert gen.depth_format() == (fmt, float(np.float32(unit)))
            for k in range(2):
                ftype = F.FEATURES_HSV if k else F.FEATURES_RGB
                cloud = gen.create_pointcloud(bgr, fl, 1, ftype)
                _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want, "RAW_DEPTH under %s unit %g" % (K.NAMES[fmt], unit))
                _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, ftype), K.NAMES[fmt])
    # back to U16: the context takes uint16 again
    gen.set_depth_format(F.DEPTH_U16)
    cloud = gen.create_pointcloud(bgr, want, 1, F.FEATURES_RGB)
    _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB), "U16 again")
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_of_a_camera_with_a_lens(pkg, size):
    """a custom camera whose scale is its own: the plane lands in the raw buffer and is rectified behind the conversion"""
    F = pkg.frontend
    w, h = size
    model = F.CameraModel(2500.0, 77.6, 77.5, (w - 1) / 2.0, (h - 1) / 2.0, LENS)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_camera(model)
    for fmt in K.FLOATS:
        bgr, fl = _scene(w, h, fmt, 2500.0)
        want = K.convert(fl, fmt, 1.0, K.frame_scale(2500.0))
        assert want.tobytes() != K.convert(fl, fmt, 1.0, 5000.0).tobytes()
        gen.set_depth_format(fmt)
        for _ in range(2):
            cloud = gen.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want, "RAW_DEPTH under " + K.NAMES[fmt])
            assert gen.read_stage(F.STAGE_RECT_DEPTH).tobytes() != want.tobytes()
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB), K.NAMES[fmt])
    gen.close(); plain.close()


def _rig():
    c = K.RIG_CASE
    return D.make_rig(c["width"], c["height"], (c["rig_scale"], 70.0, 70.2, 39.1, 29.4), (-0.12, 0.03, 0.001, -0.002, 0.0), D.K_R, D.K_T)


def _rig_scene(pkg, fmt):
    def make():
        rig = _rig()
        raw = D.scene(pkg.data, rig)
        with np.errstate(all="ignore"):
            fl = (raw.astype(np.float32) / np.float32(rig["depth_scale"])) * np.float32(1.0003)
        return (fl.astype(K.DTYPES[fmt]),)
    return _ref(("rig scene", fmt), make)[0]


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_frame_of_a_depth_camera_in_either_order(pkg, size):
    """a depth camera of 80 x 60 with a scale of its own: `scale` is the rig's, not the colour camera's; the format
    survives set_depth_camera, and the float staging follows the rig's size, whichever is set first"""
    F = pkg.frontend
    w, h = size
    c = K.RIG_CASE
    rig = _rig()
    first, second, plain = _generator(pkg, w, h), _generator(pkg, w, h), _generator(pkg, w, h)
    plain.set_depth_camera(D.to_struct(F, rig))
    for fmt in K.FLOATS:
        fl = _rig_scene(pkg, fmt)
        bgr = G.frame(w, h, 72)
        want = K.convert(fl, fmt, 1.0, K.frame_scale(c["colour_scale"], c["rig_scale"]))
        assert want.shape == (60, 80) and (want != 0).sum() > 1000
        assert want.tobytes() != K.convert(fl, fmt, 1.0, K.frame_scale(c["colour_scale"])).tobytes()
        first.set_depth_camera(None); second.set_depth_camera(None)
        first.set_depth_format(fmt)                        # the format, then the rig
        first.set_depth_camera(D.to_struct(F, rig))
        second.set_depth_format(F.DEPTH_U16)
        second.set_depth_camera(D.to_struct(F, rig))       # the rig, then the format
        second.set_depth_format(fmt)
        reference = plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB)
        for gen in (first, second):
            assert gen.depth_format() == (fmt, 1.0) and gen.depth_camera() == D.to_struct(F, rig)
            assert gen.host_buffers()[1].shape == (60, 80) and gen.host_buffers()[1].dtype == K.DTYPES[fmt]
            for _ in range(2):
                cloud = gen.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
                _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want, "RAW_DEPTH under " + K.NAMES[fmt])
                _same_frame(gen, plain, F, cloud, reference, K.NAMES[fmt])
    # the rig goes, the format stays: the staging is the context's size again
    first.set_depth_camera(None)
    assert first.depth_format()[0] == K.F16 and first.host_buffers()[1].shape == (h, w)
    bgr, fl = _scene(w, h, K.F16, 5000.0)
    plain.set_depth_camera(None)
    want = K.convert(fl, K.F16, 1.0, 5000.0)
    cloud = first.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
    _same_frame(first, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB), "without the rig")
    first.close(); second.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_median_and_gate_behind_the_conversion(pkg, size):
    F = pkg.frontend
    w, h = size
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_depth_median(F.DepthMedian(1, 3))
        g.set_depth_gate(F.DepthGate(0.8, 4.0, 0.05, 1, 0))
    for fmt in K.FLOATS:
        bgr, fl = _scene(w, h, fmt, 5000.0)
        want = K.convert(fl, fmt, 1.0, 5000.0)
        gen.set_depth_format(fmt)
        for _ in range(2):
            cloud = gen.create_pointcloud(bgr, fl, 1, F.FEATURES_RGB)
            _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want, "RAW_DEPTH under " + K.NAMES[fmt])
            _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB), K.NAMES[fmt],
                        extra=(F.STAGE_UNFILTERED_DEPTH, F.STAGE_MEDIAN, F.STAGE_GATE))
        assert gen.read_stage(F.STAGE_GATE).any() and gen.read_stage(F.STAGE_MEDIAN).any()
    gen.close(); plain.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_host_buffers_filled_in_place(pkg, size):
    """the float staging image, filled by the caller and handed back: no copy, the same frame"""
    F = pkg.frontend
    w, h = size
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for fmt in K.FLOATS:
        bgr, fl = _scene(w, h, fmt, 5000.0)
        want = K.convert(fl, fmt, 1.0, 5000.0)
        gen.set_depth_format(fmt)
        img, dep = gen.host_buffers()
        assert dep.dtype == K.DTYPES[fmt] and dep.shape == (h, w) and img.shape == (h, w, 3)
        img[:] = bgr
        dep[:] = fl
        cloud = gen.create_pointcloud(img, dep, 1, F.FEATURES_RGB)
        _differ(gen.read_stage(F.STAGE_RAW_DEPTH), want, "RAW_DEPTH under " + K.NAMES[fmt])
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud(bgr, want, 1, F.FEATURES_RGB), K.NAMES[fmt])
    gen.set_depth_format(F.DEPTH_U16)
    assert gen.host_buffers()[1].dtype == np.uint16
    gen.close(); plain.close()


def test_a_stereo_frame_does_not_read_the_format(pkg):
    """the format may be set beside stereo and is kept; the pair's frame is what it is without"""
    F = pkg.frontend
    w, h = 64, 64
    left, right, _ = S.pair(w, h, 81)
    gen, plain = _generator(pkg, w, h), _generator(pkg, w, h)
    for g in (gen, plain):
        g.set_stereo(S.to_struct(F, S.make_stereo(max_disp=8)))
    gen.set_depth_format(F.DEPTH_F16, 0.001)
    for _ in range(2):
        cloud = gen.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB)
        _same_frame(gen, plain, F, cloud, plain.create_pointcloud_stereo(left, right, S.SEQ, F.FEATURES_RGB), "stereo",
                    extra=(F.STAGE_DISPARITY, F.STAGE_STEREO))
    assert gen.depth_format() == (F.DEPTH_F16, float(np.float32(0.001)))
    gen.close(); plain.close()


# ---- 3. the setter -----------------------------------------------------------------------------------

def test_refusals_keep_what_the_context_had(pkg):
    F = pkg.frontend
    w, h = 64, 64
    gen = _generator(pkg, w, h)
    gen.set_depth_format(F.DEPTH_F32, 0.001)
    for fmt, unit in ((3, 1.0), (-1, 1.0), (F.DEPTH_F32, float("nan")), (F.DEPTH_F32, 2.0 ** 21), (F.DEPTH_F16, 2.0 ** -21),
                      (F.DEPTH_U16, 0.001), (F.DEPTH_F32, 0.0), (F.DEPTH_F32, -1.0), (F.DEPTH_F32, float("inf"))):
        with pytest.raises(pkg.capi.CvoHipError, match="set_depth_format"):
            gen.set_depth_format(fmt, unit)
        assert gen.depth_format() == (F.DEPTH_F32, float(np.float32(0.001)))
    bgr, fl = _scene(w, h, K.F32, 5000.0, 0.001)
    gen.submit(bgr, fl, 1, F.FEATURES_RGB)
    with pytest.raises(pkg.capi.CvoHipError, match="in flight"):
        gen.set_depth_format(F.DEPTH_F16)
    cloud = gen.collect()
    assert gen.depth_format() == (F.DEPTH_F32, float(np.float32(0.001))) and len(cloud[0]) >= 20
    # a stride that is no multiple of the value size, and one below the row
    import ctypes as C
    L = F.lib()
    p8, p16 = bgr.ctypes.data_as(C.POINTER(C.c_uint8)), fl.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.cvo_fe_submit(gen._h, p8, w * 3, p16, w * 4 + 2, 1, 1) == -1
    assert L.cvo_fe_submit(gen._h, p8, w * 3, p16, w * 4 - 4, 1, 1) == -1
    gen.set_depth_format(F.DEPTH_F16)
    assert L.cvo_fe_submit(gen._h, p8, w * 3, p16, w * 2 + 1, 1, 1) == -1
    with pytest.raises(ValueError):
        gen.create_pointcloud(bgr, fl[:, :-1], 1, F.FEATURES_RGB)
    gen.close()
