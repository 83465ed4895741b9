"""CPU: the host-only half of the depth-format contract (cvo_fe_check_depth_format, the refusals of
cvo_fe_convert_depth and its host copy under U16, null contexts) against tests/fe_depthfmt_ref.py; the values the contract
states about its own arithmetic; what the inputs of the GPU test are; and which errors of a device implementation
(tests/fe_depthfmt_mutants.py) they tell from the restatement.  No GPU: tests/test_gpu_fe_depth_format.py holds
k_fe_depth_convert to the same restatement by bytes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fe_depthfmt_mutants as M
import fe_depthfmt_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_the_constants_and_the_symbols(pkg):
    F = pkg.frontend
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for k, name in enumerate(K.NAMES):
        assert getattr(F, "DEPTH_" + name) == k == getattr(K, name)
        assert re.search(r"\bCVO_FE_DEPTH_%s = %d\b" % (name, k), text), name
    for name in ("cvo_fe_check_depth_format", "cvo_fe_set_depth_format", "cvo_fe_get_depth_format", "cvo_fe_convert_depth"):
        assert name in F.SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    assert "depth_format" in inspect.signature(F.run_frames).parameters
    assert callable(F.PcdGenerator.set_depth_format) and callable(F.PcdGenerator.depth_format)
    assert "THE DEPTH-FORMAT CONTRACT" in text and "images are\n * copied in" not in text


def test_check_depth_format_against_the_restatement(pkg):
    F = pkg.frontend
    units = (1.0, 0.001, 2.0 ** -20, 2.0 ** 20, np.nextafter(f32(2.0 ** -20), f32(0)), np.nextafter(f32(2.0 ** 20), f32(np.inf)),
             0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-30, 1e30, 2.0, 0.5)
    for fmt in (-1, 0, 1, 2, 3, 2 ** 31 - 1):
        for unit in units:
            assert F.check_depth_format(fmt, unit) == K.check(fmt, unit), (fmt, unit)
    assert F.check_depth_format(F.DEPTH_U16) and F.check_depth_format(F.DEPTH_F32, 0.001) and F.check_depth_format(F.DEPTH_F16, 1.0)
    assert not F.check_depth_format(F.DEPTH_U16, 0.001) and not F.check_depth_format(3, 1.0)
    assert not F.check_depth_format(F.DEPTH_F32, float("nan")) and not F.check_depth_format(F.DEPTH_F32, 2.0 ** 21)


def test_convert_depth_refuses_before_a_device_is_asked_for(pkg):
    L = pkg.frontend.lib()
    src = (C.c_float * 64)()
    out = (C.c_uint16 * 64)()
    p, o = C.cast(src, C.c_void_p), C.cast(out, C.POINTER(C.c_uint16))
    ok = dict(src=p, stride=16, w=4, h=2, fmt=K.F32, unit=1.0, scale=5000.0, out=o)
    bad = (dict(src=None), dict(out=None), dict(w=0), dict(h=0), dict(w=8193, stride=8193 * 4), dict(h=8193), dict(w=-1),
           dict(fmt=3), dict(fmt=-1), dict(unit=float("nan")), dict(unit=0.0), dict(unit=2.0 ** 21), dict(unit=-1.0),
           dict(scale=0.0), dict(scale=-5000.0), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(stride=15), dict(stride=12), dict(stride=18), dict(stride=17),
           dict(fmt=K.F16, stride=7), dict(fmt=K.F16, stride=9), dict(fmt=K.F16, stride=6),
           dict(fmt=K.U16, unit=0.001), dict(fmt=K.U16, stride=9), dict(fmt=K.U16, stride=6))
    for change in bad:
        a = dict(ok, **change)
        # (device 99 does not exist: a call that got as far as asking for it would not answer -1)
        got = L.cvo_fe_convert_depth(99, a["src"], a["stride"], a["w"], a["h"], a["fmt"], a["unit"], a["scale"], a["out"])
        assert got == -1, change
    assert L.cvo_fe_convert_depth(99, p, 16, 4, 2, K.F32, 1.0, 5000.0, o) not in (0, -1)   # (the arguments pass: no such device)


def test_u16_is_a_copy_on_the_host(pkg):
    """under U16 the stand-alone entry is a copy: no device is asked for"""
    F = pkg.frontend
    for w, h, stride in ((1, 1, None), (5, 3, None), (5, 3, 22), (64, 2, 200)):
        pitch = w * 2 if stride is None else stride
        rng = np.random.default_rng(w)
        plane = rng.integers(0, 65536, (h, w), dtype=np.uint16)
        buf, _ = K.padded(plane, (pitch - w * 2) // 2)
        keep = buf.copy()
        got = F.convert_depth(buf, K.U16, w, h, 1.0, 5000.0, device=99, stride=stride)
        assert got.dtype == np.uint16 and np.array_equal(got, plane) and np.array_equal(buf, keep), (w, h, stride)
        assert np.array_equal(got, K.convert(plane, K.U16, 1.0, 5000.0))


def test_null_contexts_are_refused(pkg):
    L = pkg.frontend.lib()
    fmt, unit = C.c_int(7), C.c_float(7.0)
    assert L.cvo_fe_set_depth_format(None, K.F32, 1.0) == -1
    assert L.cvo_fe_get_depth_format(None, C.byref(fmt), C.byref(unit)) == -1 and (fmt.value, unit.value) == (7, 7.0)
    assert L.cvo_fe_submit_device(None, 4096, 192, 8192, 128, 1, 1) == -1
    assert L.cvo_fe_submit_stereo_device(None, 4096, 192, 8192, 192, 4, 1) == -1


@pytest.mark.parametrize("config", K.CONFIGS)
def test_the_named_values(config):
    """every named value gives what the table says, by the restatement; the worked values of the contract are among them"""
    unit, scale, vals, want = K.named_values(config)
    got = K.convert(vals.reshape(1, -1), K.F32, unit, scale)[0]
    assert got.tolist() == want.tolist(), [(float(v), int(g), int(w)) for v, g, w in zip(vals, got, want) if g != w]


def test_the_worked_values_of_the_contract():
    one = lambda v, unit, scale: int(K.convert(np.array([[v]], np.float32), K.F32, unit, scale)[0, 0])
    assert one(0.8, 1.0, 5000.0) == 4000 and one(0.7998, 1.0, 5000.0) == 3999
    assert [one(x / 1024, 1.0, 1024.0) for x in (62.5, 63.5, 0.5, 1.5, 65534.5, 65535.5)] == [62, 64, 0, 2, 65534, 0]
    assert one(K.ORDER_VALUE, 0.001, 5000.0) == 14736
    assert int(M.other_order(np.array([[K.ORDER_VALUE]], np.float32), K.F32, 0.001, 5000.0)[0, 0]) == 14735
    # a float16 is widened exactly: 0.7998046875 is the float16 nearest 0.8
    assert int(K.convert(np.array([[0.8]], np.float16), K.F16, 1.0, 5000.0)[0, 0]) == 3999


def test_the_inputs_of_the_gpu_test():
    assert {(1, 1), (5, 3), (63, 2), (64, 2), (65, 3), (67, 5), (259, 2)} <= {(w, h) for w, h, _ in K.SHAPES}
    assert (5, 3, 1) in K.SHAPES
    for fmt in K.FLOATS:
        item = np.dtype(K.DTYPES[fmt]).itemsize
        pitches = {(w + pad) * item for w, h, pad in K.SHAPES if pad}
        assert any(p % 16 for p in pitches) and (fmt != K.F16 or any(p % 4 for p in pitches))
        kinds = {kind for _, _, _, kind in K.cases(fmt)}
        assert kinds == {"random"} | set(K.CONFIGS) | ({"all-patterns"} if fmt == K.F16 else set())
        for w, h, pad, kind in K.cases(fmt):
            (a, ua, sa), (b, ub, sb) = K.make_input(fmt, w, h, kind), K.make_input(fmt, w, h, kind)
            assert a.shape == (h, w) and a.dtype == K.DTYPES[fmt] and a.tobytes() == b.tobytes() and (ua, sa) == (ub, sb)
    plane, unit, scale = K.all_patterns()
    assert np.array_equal(plane.view(np.uint16).ravel(), np.arange(65536))
    # the random plane crosses both ends of the range and has holes of every kind
    v, unit, scale = K.random_plane(K.F32, 67, 5)
    out = K.convert(v, K.F32, unit, scale)
    assert (out == 0).any() and (out > 60000).any() and (out < 1000).any() and np.isnan(v).any() and (v < 0).any() and (v > 13.2).any()


@pytest.mark.parametrize("mutant", M.MUTANTS, ids=[m[0] for m in M.MUTANTS])
def test_an_input_of_the_gpu_test_tells_the_mutant_from_the_restatement(mutant):
    """for every format the mutant applies to, at least one (shape, input) of the GPU test differs"""
    name, formats, wrong = mutant
    assert formats
    for fmt in formats:
        told = []
        for w, h, pad, kind in K.cases(fmt):
            plane, unit, scale = K.make_input(fmt, w, h, kind)
            if wrong(plane, fmt, unit, scale).tobytes() != K.convert(plane, fmt, unit, scale).tobytes():
                told.append((w, h, kind))
        print(name, K.NAMES[fmt], "told by", len(told), "inputs, first", told[:1], "kinds", sorted({t[2] for t in told}))
        assert told, (name, K.NAMES[fmt])


def test_the_depth_cameras_scale_is_told_from_the_colour_cameras():
    """the frame test's depth camera has a scale of its own: a frame converted with the colour camera's differs"""
    c = K.RIG_CASE
    assert K.frame_scale(c["colour_scale"]) == f32(5000.0) and K.frame_scale(c["colour_scale"], c["rig_scale"]) == f32(1000.0)
    assert M.colour_scale_under_a_rig(c["colour_scale"], c["rig_scale"]) != K.frame_scale(c["colour_scale"], c["rig_scale"])
    v, unit, _ = K.random_plane(K.F32, c["width"], c["height"])
    right = K.convert(v, K.F32, unit, K.frame_scale(c["colour_scale"], c["rig_scale"]))
    wrong = K.convert(v, K.F32, unit, M.colour_scale_under_a_rig(c["colour_scale"], c["rig_scale"]))
    assert right.tobytes() != wrong.tobytes() and (right != 0).sum() > 1000
