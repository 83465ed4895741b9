"""Wrong versions of tests/fe_depthfmt_ref.py, one per way a depth conversion can go wrong.  Each is (name, the formats
it applies to, a function (plane, fmt, unit, scale) -> uint16 plane).  tests/test_fe_depthfmt_cpu.py shows that every
one differs from the restatement on an input the GPU test runs; byte equality on the device then rules all of them out.
The last one is a mistake of a frame, not of the arithmetic: which camera's depth_scale is `scale`."""
import numpy as np

import fe_depthfmt_ref as K

f32 = np.float32


def _finish(ok, q, lo=None, hi=None):
    """the contract's last line, or a clamp in place of either "no depth" """
    with np.errstate(all="ignore"):
        inside = (q >= f32(1.0)) & (q <= f32(65535.0))
        out = np.where(ok & inside, q, f32(0.0))
        if hi is not None:
            out = np.where(ok & (q > f32(65535.0)), f32(hi), out)
        if lo is not None:
            out = np.where(ok & (q < f32(1.0)), f32(lo), out)
        return out.astype(np.uint16)


def _front(plane, fmt, unit, widen=K.widen, admit=None):
    """v, t and the validity of the contract's first three lines"""
    with np.errstate(all="ignore"):
        v = widen(plane, fmt)
        ok = np.isfinite(v) & (v >= K.TINY)
        t = v * f32(unit)
        ok &= t >= K.TINY
        if admit is not None:
            ok = admit(v, t)
        return v, t, ok


def other_order(plane, fmt, unit, scale):
    """v * (unit * scale): one multiplication per pixel saved, another rounding"""
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit)
        return _finish(ok, np.rint(v * (f32(unit) * f32(scale))))


def truncates(plane, fmt, unit, scale):
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit)
        return _finish(ok, np.trunc(t * f32(scale)))


def half_up(plane, fmt, unit, scale):
    """floor(x + 0.5) in place of ties to even"""
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit)
        return _finish(ok, np.floor(t * f32(scale) + f32(0.5)))


def clamps_far(plane, fmt, unit, scale):
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit)
        return _finish(ok, np.rint(t * f32(scale)), hi=65535)


def clamps_near(plane, fmt, unit, scale):
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit)
        return _finish(ok, np.rint(t * f32(scale)), lo=1)


def nan_has_depth(plane, fmt, unit, scale):
    """`if (v < tiny) none` lets a NaN through, and a saturating cast makes a depth of it"""
    out = K.convert(plane, fmt, unit, scale)
    out[np.isnan(K.widen(plane, fmt))] = 1
    return out


def inf_has_depth(plane, fmt, unit, scale):
    """no finiteness test and a clamp: +inf is the farthest depth"""
    out = K.convert(plane, fmt, unit, scale)
    out[np.isposinf(K.widen(plane, fmt))] = 65535
    return out


def magnitude(plane, fmt, unit, scale):
    """|v| in place of v"""
    with np.errstate(all="ignore"):
        return K.convert(np.abs(np.asarray(plane)), fmt, unit, scale)


def subnormals_admitted(plane, fmt, unit, scale):
    """v > 0 and t > 0 in place of the two `>= 2^-126` rules (on a host that keeps subnormals)"""
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit, admit=lambda v, t: np.isfinite(v) & (v > 0) & (t > 0))
        return _finish(ok, np.rint(t * f32(scale)))


def half_as_bfloat(plane, fmt, unit, scale):
    """the 16 bits read as a bfloat16: the upper half of a float32"""
    def widen(p, _):
        return (np.asarray(p, np.float16).view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    with np.errstate(all="ignore"):
        v, t, ok = _front(plane, fmt, unit, widen=widen)
        return _finish(ok, np.rint(t * f32(scale)))


MUTANTS = (
    ("other-order", K.FLOATS, other_order),
    ("truncates", K.FLOATS, truncates),
    ("half-up", K.FLOATS, half_up),
    ("clamps-far", K.FLOATS, clamps_far),
    ("clamps-near", K.FLOATS, clamps_near),
    ("nan-has-depth", K.FLOATS, nan_has_depth),
    ("inf-has-depth", K.FLOATS, inf_has_depth),
    ("magnitude", K.FLOATS, magnitude),
    ("subnormals-admitted", (K.F32,), subnormals_admitted),   # (no float16 is a float32 subnormal)
    ("half-as-bfloat", (K.F16,), half_as_bfloat),
)


def colour_scale_under_a_rig(colour_scale, rig_scale=None):
    """the colour camera's depth_scale although a depth camera reads the image first"""
    return f32(colour_scale)
